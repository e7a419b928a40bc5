"""Test infrastructure of the parameter gradients through the fused env.step (dsim_env_step_backward_params):

* the fused step under given parameter values and its adjoint with g_dof / g_contact on the lane-serial host harness
  (dsim_emu_env_forward_params / dsim_emu_env_backward_params of tests/emu/dsim_emu_envpar.cpp; emu_lib loads the harness);
* the rollout of a tests/golden/<env>_envpar.npz recording (tools/gen_env_param_golden.py) through any pair of such functions --
  the host harness here, the device library in tests/test_gpu_env_step_params.py -- and its comparison with the recording;
* the bound both tiers share.
"""
import ctypes as C

import numpy as np

import emu_lib
import par_lib
from emu_lib import _nan, _params, f32, make_desc, make_episode, ptr
from oracle_lib import golden, template_from_golden

LIB = "libdsim_emu_envpar.so"
# the step geometry of the recordings: sim_substeps = 4 at the environment's own substep length, mass matrix every 2nd substep
SUBSTEPS, MM = 4, 2
# termination rules of the reference's environments: (height termination, invalid-state checks)
RULES = {"ant": (True, False), "humanoid": (True, True), "snu": (True, True), "hopper": (True, False),
         "cheetah": (False, False), "cartpole": (False, False)}


# The two entry points only THIS build of the harness has, bound by name: tests/test_emu_harness.py holds every `.dsim_emu_*`
# attribute that a *_lib.py module spells out against libdsim_emu.so, the library emu_lib.emu() loads, and these two are not in
# it by design.  tests/test_emu_env_step_params.py holds them -- and every other entry point -- against libdsim_emu_envpar.so.
ENTRY_POINTS = ("dsim_emu_env_forward_params", "dsim_emu_env_backward_params")


def lib():
    return emu_lib._harness(LIB)


def _env_forward_params():
    return getattr(lib(), ENTRY_POINTS[0])


def _env_backward_params():
    return getattr(lib(), ENTRY_POINTS[1])


def env_forward(t, spec, q, qd, actions, dt, substeps, mm_freq, episode=None, params=None, static=False, waves=1, lean=False):
    """-> (q_out, qd_out, obs, rew, ckpt); the outputs start as NaN (the checkpoint as zeros: its rows have padding words)"""
    L = lib()
    desc, keep = make_desc(t)
    q, qd, actions = f32(q), f32(qd), f32(actions)
    N = q.shape[0]
    pp, keep2 = _params(params)
    qo, qdo, obs, rew = _nan(*q.shape), _nan(*qd.shape), _nan(N, spec.n_obs), _nan(N)
    with emu_lib.mode(L, static, waves, lean):
        ck = np.zeros((N, int(L.dsim_emu_ckpt_floats(C.byref(desc), C.c_int(substeps), C.c_int(mm_freq)))), np.float32)
        rc = _env_forward_params()(C.byref(desc), pp, C.byref(spec), C.c_int(N), ptr(q), ptr(qd), ptr(actions), C.c_float(dt),
                                           C.c_int(substeps), C.c_int(mm_freq), ptr(qo), ptr(qdo), ptr(obs), ptr(rew), ptr(ck),
                                           C.byref(episode) if episode is not None else None)
    assert rc == 0, rc
    return qo, qdo, obs, rew, ck


def _cots(cots):
    return [f32(a) if a is not None else None for a in cots]


def env_backward(t, spec, ck, actions, dt, substeps, mm_freq, gq_out, gqd_out, gobs, grew, gobs_before=None, static=False, waves=1,
                 lean=False):
    """dsim_emu_env_backward (the plain context) of the same harness -> (gq, gqd, ga), NaN-filled before the call"""
    L = lib()
    desc, keep = make_desc(t)
    ck, actions = f32(ck), f32(actions)
    N = actions.shape[0]
    g = _cots((gq_out, gqd_out, gobs, grew, gobs_before))
    gq, gqd, ga = _nan(N, t.n_q), _nan(N, t.n_qd), _nan(*actions.shape)
    with emu_lib.mode(L, static, waves, lean):
        rc = L.dsim_emu_env_backward(C.byref(desc), C.byref(spec), C.c_int(N), ptr(ck), ptr(actions), C.c_float(dt), C.c_int(substeps),
                                     C.c_int(mm_freq), *[ptr(a) for a in g], ptr(gq), ptr(gqd), ptr(ga))
    assert rc == 0, rc
    return gq, gqd, ga


def env_backward_params(t, spec, ck, actions, dt, substeps, mm_freq, gq_out, gqd_out, gobs, grew, gobs_before=None, params=None,
                        static=False, waves=1, lean=False, want=(True, True)):
    """dsim_emu_env_backward_params -> dict(gq, gqd, ga, g_dof, g_contact); want = (g_dof, g_contact): an output not wanted is passed
    as NULL and returned as None.  Every buffer starts as NaN: what comes back was written."""
    L = lib()
    desc, keep = make_desc(t)
    ck, actions = f32(ck), f32(actions)
    N = actions.shape[0]
    g = _cots((gq_out, gqd_out, gobs, grew, gobs_before))
    pp, keep2 = _params(params)
    gq, gqd, ga = _nan(N, t.n_q), _nan(N, t.n_qd), _nan(*actions.shape)
    g_dof = _nan(N, 5, t.n_qd) if want[0] else None
    g_con = _nan(N, t.n_contacts, 4) if want[1] else None
    with emu_lib.mode(L, static, waves, lean):
        rc = _env_backward_params()(C.byref(desc), pp, C.byref(spec), C.c_int(N), ptr(ck), ptr(actions), C.c_float(dt),
                                            C.c_int(substeps), C.c_int(mm_freq), *[ptr(a) for a in g], ptr(gq), ptr(gqd), ptr(ga),
                                            ptr(g_dof), ptr(g_con))
    assert rc == 0, rc
    return dict(gq=gq, gqd=gqd, ga=ga, g_dof=g_dof, g_contact=g_con)


def step_backward(t, ck, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, **kw):
    """dsim_emu_step_backward of the same harness with both parameter outputs (emu_lib.step_backward)"""
    return emu_lib.step_backward(t, ck, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, want=(True, True), lib=lib(), **kw)


def joint_actuation(t, spec, scale, actions):
    """(act [N, nd], mact [N, M] | None) as the fused step forms them from raw actions (include/dsim.h: dsim_env_spec)"""
    a = np.clip(f32(actions), np.float32(-1.0), np.float32(1.0))
    N = a.shape[0]
    act = np.zeros((N, t.n_qd), np.float32)
    if spec.act_muscle:
        return act, ((a * np.float32(0.5) + np.float32(0.5)) * f32(scale)[None]).astype(np.float32)
    act[:, spec.act_offset:spec.act_offset + spec.n_act] = a * f32(scale)[None]
    return act, (np.zeros((N, t.n_muscles), np.float32) if t.n_muscles else None)


# ---- the recordings ------------------------------------------------------------------------------------------------------
def case(name):
    """(template, recording, env spec, keepalive of the spec's act_scale)"""
    t, g = template_from_golden(name), golden(name + "_envpar")
    spec, keep = emu_lib.env_spec_for(name, t)
    return t, g, spec, keep


def bound(noise):
    """per tensor: max(1e-4, 10 x the recorded +-1 ulp noise of the reference), in the tensor's max-norm -- the margin of
    par_lib.param_bound against the reference's own noise, without its ceiling"""
    return max(1e-4, 10.0 * float(noise))


class EpisodeArrays:
    """the episode block of one step as host arrays: progress [n] int64 and reset_count [n] int32 in / out, done [n] int64 and
    obs_before [n, n_obs] out, the pool of start states [1, n, .], the termination rules"""

    def __init__(self, progress, done, obs_before, reset_q, reset_qd, reset_count, episode_length, height_terminate, check_invalid):
        self.progress, self.done, self.obs_before, self.reset_q, self.reset_qd = progress, done, obs_before, reset_q, reset_qd
        self.reset_count, self.episode_length = reset_count, episode_length
        self.height_terminate, self.check_invalid = height_terminate, check_invalid

    def host(self):
        """the capi.Episode over these arrays (the host harness)"""
        return make_episode(self.progress, self.done, self.obs_before, self.reset_q, self.reset_qd, self.reset_count,
                            self.episode_length, self.height_terminate, self.check_invalid)


def rollout(name, t, g, spec, forward, backward):
    """The recorded rollout: H steps with the episode bookkeeping of the recording, then the reverse chain of the recorded loss
    (weights w_rew [H, n] on the rewards, w_before [H, n, n_obs] on obs_before_reset, w_obs [n, n_obs] on the LAST observation).
    forward(q, qd, actions, ep) -> (q, qd, obs, rew, ckpt), where ep holds the episode block as host arrays (EpisodeArrays: the
    callback updates progress / reset_count and fills done / obs_before); backward(ckpt, actions, gq, gqd, gobs, grew,
    gobs_before) -> dict(gq, gqd, ga, g_dof, g_contact) of numpy arrays.
    -> (per step records, grad_actions [H, n, n_act], g_dof summed over the steps [n, 5, nd], g_contact [n, C, 4])"""
    H, n = g["actions"].shape[:2]
    q, qd = g["q0"].copy(), g["qd0"].copy()
    pool_q, pool_qd = g["reset_q"][None].copy(), g["reset_qd"][None].copy()
    prog, cnt = g["progress0"].astype(np.int64).copy(), np.zeros(n, np.int32)
    tape, rec = [], dict(obs=[], rew=[], done=[], obs_before=[])
    for s in range(H):
        done, ob = np.zeros(n, np.int64), np.zeros((n, spec.n_obs), np.float32)
        ep = EpisodeArrays(prog, done, ob, pool_q, pool_qd, cnt, int(g["episode_length"]), *RULES[name])
        q, qd, obs, rew, ck = forward(q, qd, g["actions"][s], ep)
        tape.append(ck)
        for k, v in (("obs", obs), ("rew", rew), ("done", done), ("obs_before", ob)):
            rec[k].append(np.array(v, copy=True))
    gq, gqd = np.zeros_like(q), np.zeros_like(qd)
    ga = np.zeros_like(g["actions"])
    g_dof = np.zeros((n, 5, t.n_qd), np.float64)
    g_con = np.zeros((n, t.n_contacts, 4), np.float64)
    for s in reversed(range(H)):
        r = backward(tape[s], g["actions"][s], gq, gqd, g["w_obs"] if s == H - 1 else None, g["w_rew"][s], g["w_before"][s])
        gq, gqd, ga[s] = r["gq"], r["gqd"], r["ga"]
        g_dof += r["g_dof"]
        if t.n_contacts:
            g_con += r["g_contact"]
    return {k: np.stack(v) for k, v in rec.items()}, ga, g_dof, g_con


def check_recording(name, t, g, rec, ga, g_dof, g_con, show=print):
    """the rollout above against the recording: episode flags exactly, observations / rewards / action gradients at the bounds of
    the episode tests, every parameter tensor within bound(noise) in its max-norm.  Prints each figure before it asserts."""
    from oracle_lib import relerr
    np.testing.assert_array_equal(rec["done"], g["done"])
    for k in ("obs", "obs_before"):
        assert relerr(rec[k], g[k]) < 1e-3, k
    assert np.abs(rec["rew"] - g["rew"]).max() < 1e-3 * max(1.0, np.abs(g["rew"]).max())
    assert relerr(ga, g["grad_actions"]) < 1e-3
    got = par_lib.fold(t, name, g_dof, g_con if t.n_contacts else None)
    failed = []
    for k in par_lib.PARAM_TENSORS:
        if k not in got:
            continue   # (a tensor the model does not have: the contact materials of CartPole)
        if "noise_" + k not in g:   # the reference records an all-zero tensor (joint_target where every target_ke is 0): so do we
            show("%-9s %-18s all zero in the recording" % (name, k))
            if np.asarray(g[k]).any() or got[k].any():
                failed.append((k, float(np.abs(got[k]).max()), 0.0))
            continue
        ref = np.asarray(g[k], np.float64)
        err = np.abs(got[k] - ref).max() / np.abs(ref).max()
        b = bound(g["noise_" + k])
        show("%-9s %-18s err %.2e  bound %.2e  (recorded noise %.2e)" % (name, k, err, b, float(g["noise_" + k])))
        if not err < b:
            failed.append((k, err, b))
    assert not failed, failed
