"""Test infrastructure of the differentiable ground-contact read-out (dsim_ground_contacts / dsim_ground_contacts_backward):

* the entry points of the lane-serial host harness for this phase code (tests/emu/dsim_emu_con.cpp; tests/emu_lib.py loads the
  harness), for the shipped layouts and for the two user models of tests/golden/user_*.npz;
* a float64 numpy statement of the contact forward (on the frames and twists of kin_lib.fk, or on recorded ones) and of its
  adjoint, chained with kin_lib.fk_adjoint: the reference for `point` and `vel`, which the reference simulator has no tensor
  of, and for models it has no recording of.
"""
import ctypes as C

import numpy as np

from diffrl_amd.capi import make_desc
from emu_lib import ROOT  # noqa: F401
from emu_lib import emu, emu_user, f32, mode, ptr
import kin_lib
from kin_lib import rot

ENVS = ("ant", "humanoid", "snu", "hopper", "cheetah")   # the models with ground contacts
EDGE = 1e-4   # |point.y| below which fp32 rounding may flip the active set of a contact


def emu_con_forward(t, q, qd, static=False, waves=1, user=False, want=(True, True, True, True)):
    """-> (point, vel, force, link_wrench); an output not wanted is passed as NULL and returned as None.  The buffers start as
    NaN: what comes back was written."""
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q, qd = f32(q), f32(qd)
    N, L, Cn = q.shape[0], t.n_links, t.n_contacts
    outs = [np.full((N, Cn, 3), np.nan, np.float32) if w else None for w in want[:3]]
    outs.append(np.full((N, L, 6), np.nan, np.float32) if want[3] else None)
    with mode(lib, static, waves):
        rc = lib.dsim_emu_ground_contacts(C.byref(desc), C.c_int(N), ptr(q), ptr(qd), *[ptr(o) for o in outs])
    assert rc == 0, rc
    return tuple(outs)


def emu_con_backward(t, q, qd, gpoint, gvel, gforce, glw, static=False, waves=1, user=False):
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q, qd, gpoint, gvel, gforce, glw = f32(q), f32(qd), f32(gpoint), f32(gvel), f32(gforce), f32(glw)
    N = q.shape[0]
    gq = np.full((N, t.n_q), np.nan, np.float32)
    gqd = np.full((N, t.n_qd), np.nan, np.float32)
    with mode(lib, static, waves):
        rc = lib.dsim_emu_ground_contacts_backward(C.byref(desc), C.c_int(N), ptr(q), ptr(qd), ptr(gpoint), ptr(gvel), ptr(gforce),
                                                   ptr(glw), ptr(gq), ptr(gqd))
    assert rc == 0, rc
    return gq, gqd


# ---- float64 statement ----------------------------------------------------------------------------------------------
def contacts(t, Xsc, v):
    """one environment, float64, on given link frames Xsc [L][7] and twists v [L][6]: point, vel, force [C][3], link_wrench
    [L][6] and, per contact, what the adjoint and the tests ask about it (active, vn, a1, a2, x = the body-fixed point)"""
    Cn, L = t.n_contacts, t.n_links
    point, vel, force, lw = np.zeros((Cn, 3)), np.zeros((Cn, 3)), np.zeros((Cn, 3)), np.zeros((L, 6))
    aux = dict(active=np.zeros(Cn, bool), vn=np.zeros(Cn), a1=np.zeros(Cn), a2=np.zeros(Cn), x=np.zeros((Cn, 3)))
    for k in range(Cn):
        b = int(t.contact_body[k])
        ke, kd, kf, mu = (float(m) for m in t.contact_material[k])
        x = Xsc[b, :3] + rot(Xsc[b, 3:], np.asarray(t.contact_point[k], np.float64))
        p = x - np.array([0.0, float(t.contact_dist[k]), 0.0])
        dp = v[b, 3:] + np.cross(v[b, :3], p)
        point[k], vel[k], aux["x"][k] = p, dp, x
        c = p[1]
        if c >= 0.0:
            continue
        vn = dp[1]
        vt = np.array([dp[0], 0.0, dp[2]])
        lt = np.linalg.norm(vt)
        a1, a2 = kf * lt, -mu * c * ke
        ft = (vt / lt) * min(a1, a2) if lt > 0.0 else np.zeros(3)
        F = ft + np.array([0.0, c * ke + min(vn, 0.0) * kd * (-c), 0.0])
        force[k] = F
        lw[b] += np.concatenate([np.cross(p, F), F])
        aux["active"][k], aux["vn"][k], aux["a1"][k], aux["a2"][k] = True, vn, a1, a2
    return point, vel, force, lw, aux


def forward(t, q, qd):
    """one environment, float64 -> (point, vel, force, link_wrench, aux)"""
    Xsc, _, v, _ = kin_lib.fk(t, np.asarray(q, np.float64), np.asarray(qd, np.float64))
    return contacts(t, Xsc, v)


def contacts_adjoint(t, Xsc, v, gpoint, gvel, gforce, glw):
    """cotangents of the four outputs (float64, one environment) -> cotangents (gXsc [L][7], gv [L][6]) of the link frames and
    twists: per contact the pose wrench (x x a_p, a_p), written as the frame cotangent that kin_lib.fk_adjoint turns back into
    it, and the twist cotangent (p x a_dp, a_dp).  The branch rules are the step adjoint's."""
    Cn, L = t.n_contacts, t.n_links
    point, vel, force, _, aux = contacts(t, Xsc, v)
    gX, gv = np.zeros((L, 7)), np.zeros((L, 6))
    for k in range(Cn):
        b = int(t.contact_body[k])
        ke, kd, kf, mu = (float(m) for m in t.contact_material[k])
        p, dp, F, x = point[k], vel[k], force[k], aux["x"][k]
        w = v[b, :3]
        a_p, a_dp = np.array(gpoint[k], np.float64), np.array(gvel[k], np.float64)
        if aux["active"][k]:
            A = np.asarray(glw[b], np.float64)
            c, vn = p[1], dp[1]
            a_F = np.asarray(gforce[k], np.float64) + A[3:] + np.cross(A[:3], p)
            a_p += np.cross(F, A[:3])
            vt = np.array([dp[0], 0.0, dp[2]])
            lt = np.linalg.norm(vt)
            a_c = (ke - min(vn, 0.0) * kd) * a_F[1]
            if vn < 0.0:
                a_dp[1] += kd * (-c) * a_F[1]
            if lt > 0.0:
                nh = vt / lt
                a_ft = np.array([a_F[0], 0.0, a_F[2]])
                a_s = nh @ a_ft
                smin = min(aux["a1"][k], aux["a2"][k])
                a_vt = (a_ft - nh * (nh @ a_ft)) * (smin / lt)
                if aux["a1"][k] < aux["a2"][k]:
                    a_vt += nh * (kf * a_s)
                else:
                    a_c += -mu * ke * a_s
                a_dp += a_vt
            a_p[1] += a_c
        a_p += np.cross(a_dp, w)
        gv[b] += np.concatenate([np.cross(p, a_dp), a_dp])
        gX[b, :3] += a_p
        tau = np.cross(x - Xsc[b, :3], a_p)
        gX[b, 3:] += 2.0 * kin_lib.qmul(np.concatenate([tau, [0.0]]), Xsc[b, 3:])
    return gX, gv


def adjoint(t, q, qd, gpoint, gvel, gforce, glw):
    """one environment, float64 -> (gq without radial parts, gqd); a cotangent may be None (= zeros)"""
    q, qd = np.asarray(q, np.float64), np.asarray(qd, np.float64)
    Cn, L = t.n_contacts, t.n_links
    z = lambda g, shape: np.zeros(shape) if g is None else np.asarray(g, np.float64).reshape(shape)  # noqa: E731
    Xsc, _, v, _ = kin_lib.fk(t, q, qd)
    gX, gv = contacts_adjoint(t, Xsc, v, z(gpoint, (Cn, 3)), z(gvel, (Cn, 3)), z(gforce, (Cn, 3)), z(glw, (L, 6)))
    return kin_lib.fk_adjoint(t, q, qd, gX, np.zeros((L, 7)), gv)


def forward_batch(t, q, qd):
    out = [forward(t, a, b)[:4] for a, b in zip(q, qd)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def adjoint_batch(t, q, qd, gpoint, gvel, gforce, glw):
    pick = lambda g, b: None if g is None else g[b]  # noqa: E731
    out = [adjoint(t, q[b], qd[b], pick(gpoint, b), pick(gvel, b), pick(gforce, b), pick(glw, b)) for b in range(len(q))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def switch_margin(t, q, qd):
    """distance of the state's contacts from the regime switches of the model, the smallest over the contacts: |point.y|, and for
    an active contact |vn|, |vt| and |a1 - a2| / max(a1, a2)"""
    point, vel, _, _, aux = forward(t, q, qd)
    m = np.abs(point[:, 1]).min() if t.n_contacts else np.inf
    for k in np.nonzero(aux["active"])[0]:
        lt = np.hypot(vel[k, 0], vel[k, 2])
        m = min(m, abs(aux["vn"][k]), lt, abs(aux["a1"][k] - aux["a2"][k]) / max(aux["a1"][k], aux["a2"][k], 1e-300))
    return float(m)


def coverage(t, q, qd):
    """counts over a batch of states: active contacts, and of those a1 < a2, a1 >= a2, vn < 0, vn >= 0"""
    n = dict(active=0, a1_lt_a2=0, a1_ge_a2=0, vn_lt_0=0, vn_ge_0=0)
    for a, b in zip(q, qd):
        aux = forward(t, a, b)[4]
        act = aux["active"]
        n["active"] += int(act.sum())
        n["a1_lt_a2"] += int((aux["a1"][act] < aux["a2"][act]).sum())
        n["a1_ge_a2"] += int((aux["a1"][act] >= aux["a2"][act]).sum())
        n["vn_lt_0"] += int((aux["vn"][act] < 0).sum())
        n["vn_ge_0"] += int((aux["vn"][act] >= 0).sum())
    return n


def gather_link_wrench(t, point, force):
    """[N][L][6]: per link the sum in contact order of (point x force, force), float64"""
    N = point.shape[0]
    lw = np.zeros((N, t.n_links, 6))
    p, f = np.asarray(point, np.float64), np.asarray(force, np.float64)
    for k in range(t.n_contacts):
        lw[:, int(t.contact_body[k])] += np.concatenate([np.cross(p[:, k], f[:, k]), f[:, k]], axis=1)
    return lw
