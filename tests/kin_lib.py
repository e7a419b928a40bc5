"""Test infrastructure of the differentiable body kinematics (dsim_body_kinematics / dsim_body_kinematics_backward):

* the entry points of the lane-serial host harness for this phase code (tests/emu/dsim_emu_kin.cpp; tests/emu_lib.py loads the
  harness), for the shipped layouts and for the two user models of tests/golden/user_*.npz;
* a float64 numpy statement of the forward kinematics and of the four steps of its adjoint (include/dsim.h, DESIGN.md
  section 3), the reference for models the reference simulator has no recording of.
"""
import ctypes as C

import numpy as np

from diffrl_amd.capi import make_desc
from emu_lib import ENVS, USER_MODELS, waves_of  # noqa: F401
from emu_lib import f32, ptr, emu, emu_user, mode


def emu_kin_forward(t, q, qd, static=False, waves=1, user=False, want_xsm=True):
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q, qd = f32(q), f32(qd)
    N, L = q.shape[0], t.n_links
    xsc = np.full((N, L, 7), np.nan, np.float32)
    xsm = np.full((N, L, 7), np.nan, np.float32) if want_xsm else None
    vs = np.full((N, L, 6), np.nan, np.float32) if qd is not None else None
    with mode(lib, static, waves):
        rc = lib.dsim_emu_body_kinematics(C.byref(desc), C.c_int(N), ptr(q), ptr(qd), ptr(xsc), ptr(xsm), ptr(vs))
    assert rc == 0, rc
    return xsc, xsm, vs


def emu_kin_backward(t, q, qd, gxsc, gxsm, gvs, static=False, waves=1, user=False):
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q, qd, gxsc, gxsm, gvs = f32(q), f32(qd), f32(gxsc), f32(gxsm), f32(gvs)
    N = q.shape[0]
    gq = np.full((N, t.n_q), np.nan, np.float32)
    gqd = np.full((N, t.n_qd), np.nan, np.float32) if qd is not None else None
    with mode(lib, static, waves):
        rc = lib.dsim_emu_body_kinematics_backward(C.byref(desc), C.c_int(N), ptr(q), ptr(qd), ptr(gxsc), ptr(gxsm), ptr(gvs), ptr(gq), ptr(gqd))
    assert rc == 0, rc
    return gq, gqd


# ---- float64 statement ----------------------------------------------------------------------------------------------
def qmul(a, b):
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def qconj(a):
    return np.array([-a[0], -a[1], -a[2], a[3]])


def rot(r, v):
    return qmul(qmul(r, np.concatenate([v, [0.0]])), qconj(r))[:3]


def xmul(A, B):
    return np.concatenate([A[:3] + rot(A[3:], B[:3]), qmul(A[3:], B[3:])])


_ND = {0: 1, 1: 1, 2: 3, 3: 0, 4: 6}   # prismatic, revolute, ball, fixed, free


def fk(t, q, qd):
    """one environment, float64: X_sc, X_sm [L][7], v_s [L][6], and (X_sj, S, vj) for the adjoint"""
    L = t.n_links
    Xsc, Xsm, Xsj, v, vj = np.zeros((L, 7)), np.zeros((L, 7)), np.zeros((L, 7)), np.zeros((L, 6)), np.zeros((L, 6))
    S = np.zeros((t.n_qd, 6))
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    for i in range(L):
        ty, p, cs, ds = int(t.joint_type[i]), int(t.joint_parent[i]), int(t.joint_q_start[i]), int(t.joint_qd_start[i])
        ax = np.asarray(t.joint_axis[i], np.float64)
        Xsj[i] = xmul(Xsc[p] if p >= 0 else ident, np.asarray(t.joint_X_pj[i], np.float64))
        if ty == 0:
            Xjc = np.concatenate([ax * q[cs], [0, 0, 0, 1.0]])
        elif ty == 1:
            Xjc = np.concatenate([[0, 0, 0], ax * np.sin(q[cs] / 2), [np.cos(q[cs] / 2)]])
        elif ty == 2:
            Xjc = np.concatenate([[0, 0, 0], q[cs:cs + 4]])
        elif ty == 4:
            Xjc = q[cs:cs + 7].copy()
        else:
            Xjc = ident
        Xsc[i] = xmul(Xsj[i], Xjc)
        Xsm[i] = xmul(Xsc[i], np.asarray(t.joint_X_cm[i], np.float64))
        pj, rj = Xsj[i][:3], Xsj[i][3:]

        def tw(w, u):   # a joint-frame twist in the world, about the world origin
            return np.concatenate([rot(rj, w), rot(rj, u) + np.cross(pj, rot(rj, w))])
        if ty == 0:
            S[ds] = tw(np.zeros(3), ax)
        elif ty == 1:
            S[ds] = tw(ax, np.zeros(3))
        elif ty == 2:
            for k in range(3):
                S[ds + k] = tw(np.eye(3)[k], np.zeros(3))
        elif ty == 4:
            S[ds:ds + 6] = np.eye(6)
        nd = _ND[ty]
        vj[i] = S[ds:ds + nd].T @ qd[ds:ds + nd] if nd else 0
        v[i] = (v[p] if p >= 0 else 0) + vj[i]
    return Xsc, Xsm, v, dict(Xsj=Xsj, S=S, vj=vj)


def tq(g, r):
    """torque of a quaternion cotangent: <g, 1/2 (dth, 0) (x) r> = dth . tq"""
    return 0.5 * qmul(g, qconj(r))[:3]


def fk_adjoint(t, q, qd, gXsc, gXsm, gv):
    """the four steps of the adjoint (one environment, float64) -> gq (no component along the quaternions), gqd"""
    L = t.n_links
    Xsc, Xsm, v, aux = fk(t, q, qd)
    S, vj, Xsj = aux["S"], aux["vj"], aux["Xsj"]
    W = np.zeros((L, 6))   # 1. pose wrenches (torque about the world origin, force)
    for i in range(L):
        W[i, 3:] = gXsc[i, :3] + gXsm[i, :3]
        W[i, :3] = (np.cross(Xsc[i, :3], gXsc[i, :3]) + np.cross(Xsm[i, :3], gXsm[i, :3]) + tq(gXsc[i, 3:], Xsc[i, 3:])
                    + tq(gXsm[i, 3:], Xsm[i, 3:]))
    A = np.array(gv, np.float64)   # 2. subtree sums of the twist cotangents
    for i in range(L - 1, 0, -1):
        if t.joint_parent[i] >= 0:
            A[int(t.joint_parent[i])] += A[i]
    for i in range(L):             # 3. the motion subspace of a non-free joint rides on the parent link
        p, ty = int(t.joint_parent[i]), int(t.joint_type[i])
        if p >= 0 and ty != 4:
            W[p, :3] += np.cross(vj[i, :3], A[i, :3]) + np.cross(vj[i, 3:], A[i, 3:])
            W[p, 3:] += np.cross(vj[i, :3], A[i, 3:])
    Wt = W.copy()                  # 4. subtree sums of the wrenches, joint-motion transpose
    for i in range(L - 1, 0, -1):
        if t.joint_parent[i] >= 0:
            Wt[int(t.joint_parent[i])] += Wt[i]
    gq, gqd = np.zeros(t.n_q), np.zeros(t.n_qd)
    for i in range(L):
        ty, cs, ds = int(t.joint_type[i]), int(t.joint_q_start[i]), int(t.joint_qd_start[i])
        for k in range(_ND[ty]):
            gqd[ds + k] = S[ds + k] @ A[i]
        rj = Xsj[i][3:]
        if ty in (0, 1):
            gq[cs] = S[ds] @ Wt[i]
        elif ty == 2:
            tau = Wt[i, :3] - np.cross(Xsj[i][:3], Wt[i, 3:])
            gq[cs:cs + 4] = 2.0 * qmul(np.concatenate([rot(qconj(rj), tau), [0.0]]), q[cs:cs + 4])
        elif ty == 4:
            gq[cs:cs + 3] = rot(qconj(rj), Wt[i, 3:])
            tau = Wt[i, :3] - np.cross(Xsc[i][:3], Wt[i, 3:])
            gq[cs + 3:cs + 7] = 2.0 * qmul(np.concatenate([rot(qconj(rj), tau), [0.0]]), q[cs + 3:cs + 7])
    return gq, gqd


def fk_batch(t, q, qd):
    out = [fk(t, np.asarray(a, np.float64), np.asarray(b, np.float64))[:3] for a, b in zip(q, qd)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def fk_adjoint_batch(t, q, qd, gXsc, gXsm, gv):
    z7, z6 = np.zeros((t.n_links, 7)), np.zeros((t.n_links, 6))
    out = [fk_adjoint(t, np.asarray(q[b], np.float64), np.asarray(qd[b], np.float64),
                      np.asarray(gXsc[b], np.float64) if gXsc is not None else z7,
                      np.asarray(gXsm[b], np.float64) if gXsm is not None else z7,
                      np.asarray(gv[b], np.float64) if gv is not None else z6) for b in range(len(q))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def radial_part(t, q, g):
    """max |component of g along the quaternion blocks of q| / max |g|"""
    from oracle_lib import project_tangent
    g = np.asarray(g, np.float64).reshape(-1, t.n_q)
    return float(np.abs(g - project_tangent(t, q, g)).max() / (np.abs(g).max() + 1e-30))
