"""Test infrastructure of the step Jacobian (dsim_step_backward_multi / dsim_step_jacobian):

* the entry points of the lane-serial host harness for the block mapping (dsim_core.hpp: dsim_multi_slot) around the step
  adjoint (tests/emu/dsim_emu_jac.cpp; tests/emu_lib.py loads the harness and has the single sweep, step_forward / step_backward);
* the comparison against tests/golden/<env>_lin.npz (tools/gen_linearise_golden.py), shared by the host and the GPU tier.

Bounds.  Every Jacobian block (J_qq, J_q_qd, J_qd_q, J_qd_qd, J_act, J_muscle) is compared in ITS OWN max-norm relative error,
the q_in columns after project_tangent, against BOUND = 1e-3, the project's one-step gradient tolerance (BASELINE.md section 4,
tests/test_gpu_parity.py).  The fixtures record the reference's own deviation under +-1 ulp of (q, qd) per block; a block whose
recorded noise exceeds EXCLUDE = 1e-4 cannot be held to 1e-3 by any re-association of the arithmetic and is not compared (it must
still be finite and pass the bit-equality with the single sweeps) -- at most ONE block per model: where the recording puts several
blocks over the threshold, the noisiest one is excluded and the others are compared at 1e-3 all the same.  The recordings:
  cartpole   J_qd_q 1.5e-4 (excluded; every other block <= 2.8e-6)
  snu        J_qq 1.8e-3 (excluded), J_qd_q 5.1e-4 (compared); the first states of its step fixture sit on a joint-limit / contact
             switch (tests/dyn_lib.py)
  ant, humanoid, hopper, cheetah: every block <= 9.5e-6, nothing excluded.
"""
import ctypes as C

import numpy as np

from diffrl_amd.capi import make_desc
from emu_lib import ENVS, waves_of  # noqa: F401
from emu_lib import f32, ptr, emu, mode, step_backward, step_forward
from oracle_lib import golden, project_tangent, template_from_golden

BOUND, EXCLUDE, MAX_EXCLUDED = 1e-3, 1e-4, 1
RADIAL = 1e-4   # |J[:, quaternion block] . quat_in| <= RADIAL * max |J|: the step tests' own radial bound
BLOCKS = ("J_qq", "J_q_qd", "J_qd_q", "J_qd_qd", "J_act", "J_muscle")
_cases = {}


def emu_forward(t, q, qd, act, mact, dt, S, mm, static=False, waves=1, lean=False):
    """-> (q_out, qd_out, ckpt)"""
    return step_forward(t, q, qd, act, mact, dt, S, mm, static=static, waves=waves, lean=lean)


def _outputs(t, shape):
    M = t.n_muscles
    return (np.full(shape + (t.n_q,), np.nan, np.float32), np.full(shape + (t.n_qd,), np.nan, np.float32),
            np.full(shape + (t.n_qd,), np.nan, np.float32), np.full(shape + (M,), np.nan, np.float32) if M else None)


def emu_backward(t, ck, act, mact, dt, S, mm, gq_out, gqd_out, static=False, waves=1, lean=False):
    """one sweep per environment, the pointer arithmetic of dsim_bwd_kernel -> (gq_in, gqd_in, gact, gmact | None)"""
    r = step_backward(t, ck, act, mact, dt, S, mm, gq_out, gqd_out, static=static, waves=waves, lean=lean)
    return r["gq"], r["gqd"], r["gact"], r["gmact"]


def emu_backward_multi(t, ck, act, mact, dt, S, mm, gq_out, gqd_out, shared, static=False, waves=1, lean=False):
    """every block of the device launch through dsim_multi_slot -> (gq_in [N, K, nq], gqd_in, gact, gmact | None)"""
    desc, keep = make_desc(t)
    ck, act, gq_out, gqd_out = f32(ck), f32(act), f32(gq_out), f32(gqd_out)
    mact = f32(mact) if t.n_muscles else None
    N, K = ck.shape[0], gq_out.shape[-2]
    assert gq_out.shape == ((K, t.n_q) if shared else (N, K, t.n_q))
    out = _outputs(t, (N, K))
    with mode(emu(), static, waves, lean) as lib:
        rc = lib.dsim_emu_step_backward_multi(C.byref(desc), C.c_int(N), C.c_int(K), C.c_int(1 if shared else 0), ptr(ck), ptr(act),
                                              ptr(mact), C.c_float(dt), C.c_int(S), C.c_int(mm), ptr(gq_out), ptr(gqd_out),
                                              *[ptr(o) for o in out])
    assert rc == 0, rc
    return out


def emu_jacobian(t, ck, act, mact, dt, S, mm, static=False, waves=1, lean=False):
    """-> (J_state [N, K, K], J_act [N, K, nd], J_muscle [N, K, M] | None)"""
    desc, keep = make_desc(t)
    ck, act = f32(ck), f32(act)
    mact = f32(mact) if t.n_muscles else None
    N, K, M = ck.shape[0], t.n_q + t.n_qd, t.n_muscles
    J = np.full((N, K, K), np.nan, np.float32)
    Ja = np.full((N, K, t.n_qd), np.nan, np.float32)
    Jm = np.full((N, K, M), np.nan, np.float32) if M else None
    with mode(emu(), static, waves, lean) as lib:
        rc = lib.dsim_emu_step_jacobian(C.byref(desc), C.c_int(N), ptr(ck), ptr(act), ptr(mact), C.c_float(dt), C.c_int(S), C.c_int(mm),
                                        ptr(J), ptr(Ja), ptr(Jm))
    assert rc == 0, rc
    return J, Ja, Jm


# ---- the fixtures -----------------------------------------------------------------------------------------------------------
def case(name):
    """(template, inputs of the recorded states, the recording): computed once, shared, never modified"""
    if name not in _cases:
        t, g, lin = template_from_golden(name), golden(name + "_step"), golden(name + "_lin")
        rows = lin["states"]
        inp = dict(q=g["q_in"][rows], qd=g["qd_in"][rows], act=g["act_in"][rows],
                   mact=g["muscle_act_in"][rows] if "muscle_act_in" in g else None,
                   dt=float(g["dt"]), S=int(g["substeps"]), mm=int(g["mm_freq"]))
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[name] = (t, inp, lin)
    return _cases[name]


def blocks_of(t, q, J, Ja, Jm):
    """our (J_state, J_act, J_muscle) in the fixture's blocks, the q_in columns projected onto the tangent space"""
    nq, nd = t.n_q, t.n_qd
    B, K = J.shape[0], nq + nd
    Jq = project_tangent(t, np.repeat(np.asarray(q), K, axis=0), np.asarray(J, np.float64)[:, :, :nq].reshape(B * K, nq)).reshape(B, K, nq)
    Jd = np.asarray(J, np.float64)[:, :, nq:]
    out = dict(J_qq=Jq[:, :nq], J_q_qd=Jd[:, :nq], J_qd_q=Jq[:, nq:], J_qd_qd=Jd[:, nq:], J_act=np.asarray(Ja, np.float64))
    if Jm is not None:
        out["J_muscle"] = np.asarray(Jm, np.float64)
    return out


def excluded_blocks(lin):
    """the blocks of this recording that are not compared: noise over EXCLUDE, the noisiest MAX_EXCLUDED of them"""
    over = sorted(((float(lin["noise_" + k]), k) for k in BLOCKS if k in lin and float(lin["noise_" + k]) > EXCLUDE), reverse=True)
    return [k for _, k in over[:MAX_EXCLUDED]]


def compare(name, label, t, q, lin, J, Ja, Jm):
    """prints every block's error next to the recorded reference noise, then asserts the bound on the compared blocks"""
    got = blocks_of(t, q, J, Ja, Jm)
    skip = excluded_blocks(lin)
    errs = {}
    for k in BLOCKS:
        if k not in lin:
            continue
        assert np.isfinite(got[k]).all(), k
        ref = np.asarray(lin[k], np.float64)
        errs[k] = float(np.abs(got[k] - ref).max() / (np.abs(ref).max() + 1e-30))
        print("%s %s %-8s err %.2e  reference noise %.2e  %s" % (name, label, k, errs[k], float(lin["noise_" + k]),
                                                                  "EXCLUDED" if k in skip else "bound %.0e" % BOUND))
    bad = {k: e for k, e in errs.items() if k not in skip and not e < BOUND}
    assert not bad, (name, label, bad)
    return errs


def quat_blocks(t):
    out = []
    for i in range(t.n_links):
        ty, cs = int(t.joint_type[i]), int(t.joint_q_start[i])
        if ty == 4:
            out.append(slice(cs + 3, cs + 7))
        elif ty == 2:
            out.append(slice(cs, cs + 4))
    return out


def radial(t, q, J):
    """max over the quaternion blocks and rows of |J[:, block] . quat_in| / max |J|"""
    J, q = np.asarray(J, np.float64), np.asarray(q, np.float64)
    worst = 0.0
    for sl in quat_blocks(t):
        worst = max(worst, float(np.abs(np.einsum("bkj,bj->bk", J[:, :, sl], q[:, sl])).max()))
    return worst / (np.abs(J).max() + 1e-30)
