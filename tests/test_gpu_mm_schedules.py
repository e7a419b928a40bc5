"""-m gpu: the step kernels across mass-matrix refresh schedules.  `mm_freq` decides the checkpoint layout ([substeps] rows +
ceil(S / mm) inverses + tail), when the adjoint swaps the inverse and zeroes the H accumulator, when the composite-body pass
runs, and what the row / inverse prefetch pipelines request one and two substeps ahead -- and every executor (helper wave, four
waves, inverse in registers, plain wave, pair forward, lean recompute) has its own copy of that logic.  The golden recordings
only reach one group per step, one substep per group and SNUHumanoid's six even groups; here every shipped model runs S = 7
substeps at mm in {1, 2, 3, 4, 6, 7, 9} (tests/mm_sched.py: inputs, oracle results, why seven) and H = 3 environment steps at
frequencies that leave an uneven last group, against the scalar oracle, in every kernel mode.

Bounds: BASELINE.md section 4 -- state 1e-4, gradients 1e-3 max-norm relative (joint_q after project_tangent, except the
literal call), rollout cosine > 0.9999.  Nothing here is probed: the host harness sits at <= 2.5e-4 (gradients) / 2.0e-5 (state)
on exactly these inputs, so a GPU figure over the bound is a finding.  Every checkpoint is the one Engine.forward / the
environment allocates."""
import contextlib
import os

import numpy as np
import pytest
import torch

import mm_sched as M
from oracle_lib import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE_VARS = ("DSIM_HELPER", "DSIM_PAIR", "DSIM_FORCE_GENERIC")
_engines = {}


@contextlib.contextmanager
def _switches(**kw):
    """the project's own DSIM_* switches (read when a model is created) set to exactly kw inside, restored afterwards"""
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


def _engine(env, ckpt_mode="full", **kw):
    """one Engine per (model, checkpoint mode, switches) for the whole module, not one per schedule"""
    key = (env, ckpt_mode) + tuple(sorted(kw.items()))
    if key not in _engines:
        from diffrl_amd.engine import Engine
        with _switches(**kw):
            _engines[key] = Engine(M.case(env)["t"], DEV, ckpt_mode=ckpt_mode)
    return _engines[key]


def _T(a):
    return torch.tensor(a, device=DEV).reshape(-1) if a is not None else None


def _np(x, n):
    return x.cpu().numpy().reshape(n, -1) if x is not None else None


def _run(eng, mm, c=None, env=None, literal=False):
    """forward + adjoint of the schedule inputs (or of c: dict q, qd, act, mact, gq, gqd) at (S, mm) -> dict of host arrays"""
    c = c or M.case(env)
    n = c["q"].shape[0]
    act, mact = _T(c["act"]), _T(c["mact"])
    qo, qdo, ck = eng.forward(_T(c["q"]), _T(c["qd"]), act, mact, M.DT, M.S, mm, True)
    r = eng.backward(ck, act, mact, M.DT, M.S, mm, _T(c["gq"]), _T(c["gqd"]), literal=literal)
    torch.cuda.synchronize()
    eng.status()
    out = dict(q=_np(qo, n), qd=_np(qdo, n), gq=_np(r[0], n), gqd=_np(r[1], n), gact=_np(r[2], n), ckpt=ck.cpu().numpy())
    if r[3] is not None:
        out["gmact"] = _np(r[3], n)
    for k, v in out.items():
        if k != "ckpt":      # (checkpoint rows carry alignment padding nothing writes)
            assert np.isfinite(v).all(), k
    return out


def _same(a, b, keys):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), k


OUT = ("q", "qd", "gq", "gqd", "gact", "gmact")


# ---- a. / b.: oracle parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", M.MMS)
@pytest.mark.parametrize("env", M.ENVS)
def test_step_vs_oracle_at_every_schedule(env, mm):
    """the kernels a default Engine picks (helper wave where the model has one, four waves for SNUHumanoid): q, qd, projected gq,
    gqd, gact (and gmact) against oracle_backward"""
    eng = _engine(env)
    assert eng.variant > 0, "a shipped model must run its specialised kernel set"
    M.assert_step(env, mm, _run(eng, mm, env=env), label="gpu")


@pytest.mark.parametrize("mm", [3, 9])
@pytest.mark.parametrize("env", ["ant", "snu", "cartpole"])
def test_generic_kernels_vs_oracle(env, mm):
    eng = _engine(env, DSIM_FORCE_GENERIC="1")
    assert eng.variant == 0
    M.assert_step(env, mm, _run(eng, mm, env=env), label="gpu generic")


# ---- c.: kernel modes agree bit for bit at every schedule ---------------------------------------------------------------------
@pytest.mark.parametrize("mm", M.MMS)
@pytest.mark.parametrize("env", ["ant", "humanoid", "hopper", "cheetah"])
def test_helper_wave_matches_single_wave(env, mm):
    """DSIM_HELPER=1 against 0: same arithmetic in the same order, the checkpoint included"""
    a = _run(_engine(env, DSIM_HELPER="1"), mm, env=env)
    b = _run(_engine(env, DSIM_HELPER="0"), mm, env=env)
    _same(a, b, OUT + ("ckpt",))


def _pair_inputs(env):
    """the schedule states tiled to an odd n = 7 (the last pair wave carries one environment), every environment its own actions"""
    c = M.case(env)
    n = 7
    tile = lambda a: np.ascontiguousarray(np.tile(a, (2, 1))[:n])  # noqa: E731
    rng = np.random.default_rng(5)
    act = tile(c["act"])
    act = (act + 0.1 * rng.normal(size=act.shape)).astype(np.float32)
    return dict(q=tile(c["q"]), qd=tile(c["qd"]), act=act, mact=None, gq=rng.normal(size=(n, c["t"].n_q)).astype(np.float32),
                gqd=rng.normal(size=(n, c["t"].n_qd)).astype(np.float32))


@pytest.mark.parametrize("mm", M.MMS)
@pytest.mark.parametrize("env", ["ant", "hopper", "cheetah", "cartpole"])
def test_pair_forward_matches_one_environment_per_wave(env, mm):
    """DSIM_HELPER=0 DSIM_PAIR=1 against DSIM_PAIR=0: the pair kernel writes the rows and the inverses of every group the
    (one-environment) adjoint reads"""
    c = _pair_inputs(env)
    a = _run(_engine(env, DSIM_HELPER="0", DSIM_PAIR="1"), mm, c=c)
    b = _run(_engine(env, DSIM_HELPER="0", DSIM_PAIR="0"), mm, c=c)
    _same(a, b, OUT)


@pytest.mark.parametrize("mm", M.MMS)
@pytest.mark.parametrize("env", ["ant", "humanoid", "snu"])
def test_lean_checkpoints_match_full(env, mm):
    """the lean adjoint recomputes the forward phases per substep: identical outputs, and both checkpoints have the library's size"""
    res = {}
    for mode in ("full", "lean"):
        eng = _engine(env, ckpt_mode=mode)
        res[mode] = _run(eng, mm, env=env)
        assert res[mode]["ckpt"].shape[1] == int(eng._lib.dsim_ckpt_floats_mm(eng._h, M.S, mm)), mode
    _same(res["full"], res["lean"], OUT)
    assert res["lean"]["ckpt"].shape[1] < res["full"]["ckpt"].shape[1]


# ---- d.: many cotangents per environment from one checkpoint ------------------------------------------------------------------
@pytest.mark.parametrize("ckpt_mode", ["full", "lean"])
@pytest.mark.parametrize("mm", [2, 3, 6])
@pytest.mark.parametrize("env", ["ant", "snu", "hopper"])
def test_multi_cotangent_sweep_equals_sequential_backward(env, mm, ckpt_mode):
    c = M.case(env)
    t, n, K = c["t"], M.N_STATES, 3
    eng = _engine(env, ckpt_mode=ckpt_mode)
    act, mact = _T(c["act"]), _T(c["mact"])
    qo, qdo, ck = eng.forward(_T(c["q"]), _T(c["qd"]), act, mact, M.DT, M.S, mm, True)
    rng = np.random.default_rng(31)
    gq, gqd = rng.normal(size=(K, t.n_q)).astype(np.float32), rng.normal(size=(K, t.n_qd)).astype(np.float32)
    multi = eng.backward_multi(ck, act, mact, M.DT, M.S, mm, torch.tensor(gq, device=DEV), torch.tensor(gqd, device=DEV), shared=True)
    for k in range(K):
        one = eng.backward(ck, act, mact, M.DT, M.S, mm, _T(np.repeat(gq[k:k + 1], n, 0)), _T(np.repeat(gqd[k:k + 1], n, 0)))
        for m, o in zip(multi, one):
            assert (m is None and o is None) or (torch.isfinite(o).all() and torch.equal(m[:, k].reshape(-1), o)), k
    torch.cuda.synchronize()
    eng.status()


@pytest.mark.parametrize("env", ["ant", "cartpole"])
def test_step_jacobian_rows_equal_identity_seeds(env):
    mm = 3
    c = M.case(env)
    t, n = c["t"], M.N_STATES
    nq, K = t.n_q, t.n_q + t.n_qd
    eng = _engine(env)
    act = _T(c["act"])
    qo, qdo, ck = eng.forward(_T(c["q"]), _T(c["qd"]), act, None, M.DT, M.S, mm, True)
    J, Ja, Jm = eng.step_jacobian(ck, act, None, M.DT, M.S, mm)
    assert Jm is None and torch.isfinite(J).all() and torch.isfinite(Ja).all()
    eye = np.eye(K, dtype=np.float32)
    for k in range(K):
        gq, gqd, ga, _ = eng.backward(ck, act, None, M.DT, M.S, mm, _T(np.repeat(eye[k:k + 1, :nq], n, 0)), _T(np.repeat(eye[k:k + 1, nq:], n, 0)))
        assert torch.equal(J[:, k, :nq].reshape(-1), gq) and torch.equal(J[:, k, nq:].reshape(-1), gqd), k
        assert torch.equal(Ja[:, k].reshape(-1), ga), k


# ---- e.: the literal cotangent reads the FIRST group's inverse and H accumulator ---------------------------------------------
@pytest.mark.parametrize("mm", [3, 6, 9])
@pytest.mark.parametrize("env", ["ant", "humanoid", "snu"])
def test_literal_backward_vs_oracle(env, mm):
    """un-projected gq against the oracle's at the bound of test_gpu_parity.py::test_literal_backward_vs_oracle_batch (1e-3), in both
    checkpoint modes; every other output is the plain call's, bit for bit"""
    o = M.oracle(env, mm)
    for mode in ("full", "lean"):
        eng = _engine(env, ckpt_mode=mode)
        plain, lit = _run(eng, mm, env=env), _run(eng, mm, env=env, literal=True)
        e = relerr(lit["gq"], o["gq"])
        print("mm-schedule gpu literal %s %s S=%d mm=%d: gq_unprojected %.2e  (plain call %.2e)" % (mode, env, M.S, mm, e, relerr(plain["gq"], o["gq"])))
        assert e < M.GRAD_TOL, (mode, e)
        _same(plain, lit, ("q", "qd", "gqd", "gact", "gmact"))


# ---- f.: environment level, H = 3 steps at the environments' own substep counts -----------------------------------------------
def _make(env, n, mm, no_grad=False):
    from diffrl_amd import envs
    cls = {"cartpole": envs.CartPoleSwingUpEnv, "ant": envs.AntEnv, "humanoid": envs.HumanoidEnv, "snu": envs.SNUHumanoidEnv,
           "hopper": envs.HopperEnv, "cheetah": envs.CheetahEnv}[env]
    kw = dict(num_envs=n, device=DEV, render=False, seed=0, episode_length=1000, no_grad=no_grad, stochastic_init=False,
              MM_caching_frequency=mm)
    if env in ("cartpole", "ant", "hopper", "cheetah"):
        kw["early_termination"] = False
    return cls(**kw)


def _rollout(env, mm, fused, q0, qd0, actions, no_grad=False):
    """-> (obs [H, n, .], rew [H, n], d(-sum rew)/d actions | None) through the DFlexEnv surface"""
    n = actions.shape[1]
    e = _make(env, n, mm, no_grad)
    assert e.sim_substeps == M.ENV_SUBSTEPS[env]
    e.fused = fused
    e.clear_grad()
    e.reset()
    e.reset_with_state(_T(q0), _T(qd0))
    e.initialize_trajectory()
    acts = torch.tensor(actions, device=DEV, requires_grad=not no_grad)
    loss, obs_l, rew_l = 0.0, [], []
    for s in range(M.H):
        obs, rew, done, info = e.step(acts[s])
        assert int(done.sum()) == 0
        assert no_grad or (obs.grad_fn is not None and rew.grad_fn is not None)
        obs_l.append(obs.detach().cpu().numpy().copy())
        rew_l.append(rew.detach().cpu().numpy().copy())
        loss = loss - rew.sum()
    if not no_grad:
        loss.backward()
    torch.cuda.synchronize()
    e.model.engine().status()
    return np.stack(obs_l), np.stack(rew_l), None if no_grad else acts.grad.cpu().numpy().copy()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("env,mm", M.ENV_MM)
def test_rollout_vs_oracle_at_uneven_groups(env, mm, fused):
    """obs and rew per step and d(-sum rew)/d actions against the torch surface on the scalar oracle at the same
    MM_caching_frequency; the no_grad run (no checkpoint, no group bookkeeping to write) returns the same obs / rew bit for bit"""
    c = M.rollout_case(env)
    with _switches():
        obs, rew, ga = _rollout(env, mm, fused, c["q0"], c["qd0"], c["actions"])
        obs_ng, rew_ng, _ = _rollout(env, mm, fused, c["q0"], c["qd0"], c["actions"], no_grad=True)
    M.assert_rollout(env, mm, obs, rew, ga, label="gpu fused" if fused else "gpu unfused")
    assert np.array_equal(obs, obs_ng) and np.array_equal(rew, rew_ng)


def test_ant_rollout_kernel_modes_agree_at_uneven_groups():
    """AntEnv(MM_caching_frequency=5), five environments (an odd count: the last pair wave carries one): the single-wave kernels and
    the pair forward give the helper-wave run's obs, rew and action gradients per environment, bit for bit"""
    c = M.rollout_case("ant")
    n = 5
    idx = np.arange(n) % c["q0"].shape[0]
    q0, qd0 = c["q0"][idx], c["qd0"][idx]
    acts = np.ascontiguousarray(c["actions"][:, idx])
    acts[:, 4] = c["actions"][:, 1]          # (the fifth environment: the first one's start state, its own actions)
    res = {}
    for name, kw in (("helper", dict(DSIM_HELPER="1")), ("single", dict(DSIM_HELPER="0", DSIM_PAIR="0")),
                     ("default beyond the helper capacity", dict(DSIM_HELPER="0")), ("pair", dict(DSIM_HELPER="0", DSIM_PAIR="1"))):
        with _switches(**kw):
            res[name] = _rollout("ant", 5, True, q0, qd0, acts)
        assert all(np.isfinite(x).all() for x in res[name]), name
    for name, r in res.items():
        for x, y in zip(r, res["helper"]):
            assert np.array_equal(x, y), name
    # and the helper run is the oracle's rollout on the recorded four environments
    M.assert_rollout("ant", 5, res["helper"][0][:, :4], res["helper"][1][:, :4], res["helper"][2][:, :4], label="gpu fused n=5")
