"""Test infrastructure: the step adjoint and the fused environment adjoint on ONE checkpoint, shared by the host tier
(tests/test_emu_sweep_drivers.py) and the GPU tier (tests/test_gpu_sweep_drivers.py).

Both launches run dsim_bwd_sweep (dsim_core.hpp) and differ in their prologues and epilogues only.  The fused forward with no
episode block writes a checkpoint whose rows and inverses are those of the step forward on the joint_act / muscle activations
that dsim_env_load_actions derives from the actions; with zero cotangents on obs and rew the observation adjoint adds zeros, so
the fused adjoint's gq_in and gqd_in must be the step adjoint's BIT FOR BIT, at every refresh schedule and in every kernel mode.
The action gradient is scaled in another place (the fused epilogue multiplies by act_scale, the test does so for the step's
gact / gmact): held to the 1e-3 max-norm relative that tests/test_gpu_envs.py states for gradients.

Inputs: the first N = 3 states of tests/mm_sched.py (S = 7 substeps), actions from default_rng(23) strictly inside (-1, 1) (the
clip is the identity and passes the gradient), cotangents from mm_sched.  mm in {1, 3, 7}: a group per substep | groups 3, 3, 1
(a middle group and a trailing group of one) | one group.
"""
import contextlib
import os

import numpy as np

import mm_sched as M
from emu_lib import env_spec_for
from oracle_lib import relerr

N = 3
MMS = [1, 3, 7]
GACT_TOL = 1e-3
MODE_VARS = ("DSIM_HELPER", "DSIM_PAIR", "DSIM_FORCE_GENERIC")
_cases = {}


@contextlib.contextmanager
def switches(**kw):
    """the project's own DSIM_* switches (read when a model is created) set to exactly kw inside, restored afterwards -- as
    tests/test_gpu_mm_schedules.py::_switches does"""
    saved = {k: os.environ.get(k) for k in MODE_VARS}
    try:
        for k in MODE_VARS:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def case(env):
    """dict: t, spec (host act_scale), scale, q, qd, gq, gqd [N, .], actions [N, n_act], and what dsim_env_load_actions makes of
    them: act [N, nd], mact [N, M] | None"""
    if env not in _cases:
        c = M.case(env)
        t = c["t"]
        spec, scale = env_spec_for(env, t)
        na, off = int(spec.n_act), int(spec.act_offset)
        actions = np.random.default_rng(23).uniform(-0.9, 0.9, size=(N, na)).astype(np.float32)
        act, mact = np.zeros((N, t.n_qd), np.float32), None
        if spec.act_muscle:
            mact = (actions * np.float32(0.5) + np.float32(0.5)) * scale
        else:
            act[:, off:off + na] = actions * scale
        assert act.dtype == np.float32 and (mact is None or (mact.dtype == np.float32 and mact.shape == (N, t.n_muscles)))
        d = dict(t=t, spec=spec, scale=scale, q=c["q"][:N].copy(), qd=c["qd"][:N].copy(), gq=c["gq"][:N].copy(),
                 gqd=c["gqd"][:N].copy(), actions=actions, act=act, mact=mact)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)   # (shared by every case of both tiers)
        _cases[env] = d
    return _cases[env]


def assert_drivers_agree(env, step, fused, label=""):
    """step = (gq, gqd, gact, gmact | None), fused = (gq, gqd, gactions), host arrays [N, .]"""
    c = case(env)
    spec, na, off = c["spec"], int(c["spec"].n_act), int(c["spec"].act_offset)
    want = 0.5 * c["scale"] * step[3] if spec.act_muscle else c["scale"] * step[2][:, off:off + na]
    e = relerr(fused[2], want)
    print("sweep drivers %s %s: gq equal %s  gqd equal %s  gactions %.2e" % (label, env, np.array_equal(step[0], fused[0]),
                                                                            np.array_equal(step[1], fused[1]), e))
    for a in tuple(step[:3]) + tuple(fused):
        assert np.isfinite(a).all()
    assert np.abs(step[0]).max() > 0 and np.abs(want).max() > 0
    assert np.array_equal(step[0], fused[0]), "gq_in"
    assert np.array_equal(step[1], fused[1]), "gqd_in"
    assert e < GACT_TOL, e
