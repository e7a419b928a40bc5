"""Test infrastructure of the model-parameter gradients of the step (dsim_model_set_params / dsim_step_backward_params):

* the host harness for this phase code, tests/emu/dsim_emu_par.cpp (a translation unit that includes dsim_emu.cpp), compiled here
  with the flags of tests/emu/Makefile to tests/emu/libdsim_emu_par.so when it is older than its sources, and its entry points;
* the folds from what the kernels return -- per dof [N][5][nd], per contact slot [N][C][4] -- to what the reference records per
  environment: per link, per coordinate (target) and per SHAPE (contact_material of <env>_model.npz is the shape of each slot);
* the bounds the two test tiers share.
"""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np

from diffrl_amd.capi import make_desc
from emu_lib import EMU_DIR, f32, mode, ptr
from oracle_lib import golden, template_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = ("ant", "humanoid", "snu", "hopper", "cartpole", "cheetah")
FIELDS = ("target_ke", "target_kd", "limit_ke", "limit_kd", "target", "contact_material")   # order of DSIM_PARAM_*
DOF_ROWS = ("target_ke", "target_kd", "target", "limit_ke", "limit_kd")                     # rows of g_dof
PARAM_TENSORS = ("g_target_ke", "g_target_kd", "g_target", "g_limit_ke", "g_limit_kd", "g_shape_materials")
# forward outputs and state gradients: the bounds of the step tests (tests/test_emu_phases.py, tests/test_gpu_parity.py)
STATE_BOUND, GRAD_BOUND = 1e-4, 1e-3
HINGE = (0, 1)
_lib = None


def _make_var(name):
    src = open(os.path.join(EMU_DIR, "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^%s\s*\??=\s*(.*)$" % name, src, re.M).group(1).strip()


def _harness():
    """libdsim_emu_par.so: rebuilt when older than a source of the harness, loaded once"""
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libdsim_emu_par.so")
        deps = [os.path.normpath(os.path.join(EMU_DIR, s)) for s in _make_var("SRC").split()] + [os.path.join(EMU_DIR, "dsim_emu_par.cpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            cxx = os.environ.get("CXX") or _make_var("CXX")
            tmp = so + ".%d.tmp" % os.getpid()
            subprocess.check_call([cxx] + shlex.split(_make_var("CXXFLAGS")) + ["-shared", "-o", tmp, "dsim_emu_par.cpp"], cwd=EMU_DIR)
            os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.dsim_emu_ckpt_floats.restype = C.c_longlong
    return _lib


def _params(p):
    """dict field -> array (missing: the template's) -> (array of six pointers or None, keepalive)"""
    if not p:
        return None, None
    arrs = [f32(p[k]) if p.get(k) is not None else None for k in FIELDS]
    return (C.c_void_p * 6)(*[ptr(a) for a in arrs]), arrs


def emu_par_forward(t, q, qd, act, mact, dt, substeps, mm_freq, params=None, static=False, waves=1, lean=False):
    """-> (q_out, qd_out, ckpt); buffers start as NaN"""
    lib = _harness()
    desc, keep = make_desc(t)
    q, qd, act = f32(q), f32(qd), f32(act)
    N = q.shape[0]
    mact = f32(mact) if mact is not None else np.zeros((N, 0), np.float32)
    pp, keep2 = _params(params)
    qo, qdo = np.full_like(q, np.nan), np.full_like(qd, np.nan)
    with mode(lib, static, waves, lean):
        ck = np.zeros((N, int(lib.dsim_emu_ckpt_floats(C.byref(desc), C.c_int(substeps), C.c_int(mm_freq)))), np.float32)
        rc = lib.dsim_emu_par_forward(C.byref(desc), pp, C.c_int(N), ptr(q), ptr(qd), ptr(act), ptr(mact), C.c_float(dt),
                                      C.c_int(substeps), C.c_int(mm_freq), ptr(qo), ptr(qdo), ptr(ck))
    assert rc == 0, rc
    return qo, qdo, ck


def emu_par_backward(t, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, params=None, static=False, waves=1, lean=False,
                     want=(True, True), want_act=True):
    """want = (g_dof, g_contact); both False: the plain step adjoint.  -> dict(gq, gqd, gact, gmact, g_dof, g_contact); an output
    not wanted is passed as NULL and returned as None; the buffers start as NaN: what comes back was written."""
    lib = _harness()
    desc, keep = make_desc(t)
    ckpt, act, gq_out, gqd_out = f32(ckpt), f32(act), f32(gq_out), f32(gqd_out)
    N, nd, Cn, M = act.shape[0], t.n_qd, t.n_contacts, t.n_muscles
    mact = f32(mact) if mact is not None else np.zeros((N, 0), np.float32)
    pp, keep2 = _params(params)
    nan = lambda *s: np.full(s, np.nan, np.float32)  # noqa: E731
    gq, gqd = nan(N, t.n_q), nan(N, nd)
    ga = nan(N, nd) if want_act else None
    gm = nan(N, M) if (want_act and M) else None
    g_dof = nan(N, 5, nd) if want[0] else None
    g_con = nan(N, Cn, 4) if want[1] else None
    with mode(lib, static, waves, lean):
        rc = lib.dsim_emu_par_backward(C.byref(desc), pp, C.c_int(N), ptr(ckpt), ptr(act), ptr(mact), C.c_float(dt), C.c_int(substeps),
                                       C.c_int(mm_freq), ptr(gq_out), ptr(gqd_out), ptr(gq), ptr(gqd), ptr(ga), ptr(gm), ptr(g_dof),
                                       ptr(g_con))
    assert rc == 0, rc
    return dict(gq=gq, gqd=gqd, gact=ga, gmact=gm, g_dof=g_dof, g_contact=g_con)


# ---- folds -------------------------------------------------------------------------------------------------------------
def dof_maps(t):
    """(link of every dof [nd], coordinate of every hinge / slider dof or -1 [nd])"""
    link, coord = np.zeros(t.n_qd, np.int64), np.full(t.n_qd, -1, np.int64)
    for i in range(t.n_links):
        d0, d1 = int(t.joint_qd_start[i]), int(t.joint_qd_start[i + 1])
        link[d0:d1] = i
        if int(t.joint_type[i]) in HINGE:
            coord[d0] = int(t.joint_q_start[i])
    return link, coord


def fold(t, name, g_dof, g_contact):
    """per environment, in the reference's shapes: g_target_ke / kd, g_limit_ke / kd [N, L], g_target [N, n_q],
    g_shape_materials [N, shapes, 4] (None without contacts); float64 sums"""
    link, coord = dof_maps(t)
    out = {}
    if g_dof is not None:
        g = np.asarray(g_dof, np.float64)
        N = g.shape[0]
        for r, k in enumerate(DOF_ROWS):
            if k == "target":
                a = np.zeros((N, t.n_q))
                np.add.at(a, (slice(None), coord[coord >= 0]), g[:, r, coord >= 0])
            else:
                a = np.zeros((N, t.n_links))
                np.add.at(a, (slice(None), link), g[:, r, :])
            out["g_" + k] = a
    if g_contact is not None and t.n_contacts:
        m = golden(name + "_model")
        shape = np.asarray(m["contact_material"], np.int64)
        gc = np.asarray(g_contact, np.float64)
        a = np.zeros((gc.shape[0], m["shape_materials"].shape[0], 4))
        np.add.at(a, (slice(None), shape), gc)
        out["g_shape_materials"] = a
    return out


def param_bound(noise):
    """10 x the tensor's recorded +-1 ulp noise of the reference, floor 1e-4, ceiling 1e-3 (no recorded tensor's 10 x noise is above
    the ceiling: the largest is SNUHumanoid's shape_materials, 8.1e-4)"""
    return float(np.clip(10.0 * float(noise), 1e-4, 1e-3))


def case(name):
    """(template, fixture, actuation as (act, mact))"""
    t, g = template_from_golden(name), golden(name + "_par")
    N = g["q_in"].shape[0]
    if t.n_muscles > 0:
        return t, g, (np.zeros((N, t.n_qd), np.float32), g["muscle_act_in"])
    return t, g, (g["act_in"], None)


def perturbed_params(t, seed=5):
    """every field scaled by seeded factors in [0.8, 1.25] (targets moved by +-0.1), as float32"""
    rs = np.random.RandomState(seed)
    s = lambda a: (np.asarray(a, np.float32) * rs.uniform(0.8, 1.25, np.shape(a))).astype(np.float32)  # noqa: E731
    return dict(target_ke=s(t.joint_target_ke), target_kd=s(t.joint_target_kd), limit_ke=s(t.joint_limit_ke), limit_kd=s(t.joint_limit_kd),
                target=(t.joint_target + rs.uniform(-0.1, 0.1, t.n_q)).astype(np.float32), contact_material=s(t.contact_material))


def with_params(t, p):
    """a template with these values in place of its own"""
    import copy
    t2 = copy.deepcopy(t)
    for k, attr in (("target_ke", "joint_target_ke"), ("target_kd", "joint_target_kd"), ("limit_ke", "joint_limit_ke"),
                    ("limit_kd", "joint_limit_kd"), ("target", "joint_target"), ("contact_material", "contact_material")):
        setattr(t2, attr, np.ascontiguousarray(p[k], np.float32))
    return t2
