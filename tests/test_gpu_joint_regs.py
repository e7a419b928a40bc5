"""-m gpu: the Ant joint-space phases with their launch-invariant operands in registers (dsim_core.hpp: DsimJointRegs -- the dof
lane's row of H^-1 kept from refresh to refresh, the joint constants and act kept for the launch) and H^-1 x by row broadcast
(DevExec::row_matvec).  What can go wrong: a stale row after a refresh, a constant cached across something that changes it, a
wrong broadcast lane.  So: every refresh schedule of S = 4 substeps (mm = 1, 2, 3 -- uneven groups 3 + 1 -- and 4) at N = 1 and
N = 3 environments (odd: a half-filled pair wave), operator level and through the fused AntEnv, against the generic kernels of the
same library (which run none of the new code) and the scalar oracle; launches that follow one another with other actions and
other joint gains (Engine.set_params), eagerly and as a graph replay, against fresh models; the kernel modes against each other;
hinges outside their limits.

Tolerances are those of tests/test_gpu_quad_joint.py (tests/test_gpu_parity.py): state 1e-4, gradients 1e-3 max-norm relative
against the recording and the oracle; specialised against generic kernels 1e-5 (test_specialised_kernels_match_generic);
everything between two kernels of this library's specialised set, and between a reused and a fresh model, is bit for bit."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = [1, 3]
S4 = 4
MMS = [1, 2, 3, 4]
KEYS = ("q", "qd", "gq", "gqd", "gact")
MODE_VARS = ("DSIM_HELPER", "DSIM_PAIR", "DSIM_FORCE_GENERIC")
MODES = {"helper": dict(DSIM_HELPER="1"), "single": dict(DSIM_HELPER="0", DSIM_PAIR="0"), "pair": dict(DSIM_HELPER="0", DSIM_PAIR="1")}
_engines = {}
_oracle = {}


@contextlib.contextmanager
def _switches(**kw):
    """the project's DSIM_* switches (read when a model is created) set to exactly kw inside, restored afterwards"""
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


@pytest.fixture(scope="module")
def t():
    return template_from_golden("ant")


def _engine(t, ckpt_mode="full", fresh=False, **kw):
    from diffrl_amd.engine import Engine
    key = (ckpt_mode,) + tuple(sorted(kw.items()))
    if fresh or key not in _engines:
        with _switches(**kw):
            eng = Engine(t, torch.device(DEV), ckpt_mode=ckpt_mode)
        if fresh:
            return eng
        _engines[key] = eng
    return _engines[key]


def _T(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV).reshape(-1)


def _case(n):
    """the recorded step's first n start states with cotangents of its own recording"""
    g = golden("ant_step")
    sl = slice(0, n)
    return dict(q=g["q_in"][sl], qd=g["qd_in"][sl], act=g["act_in"][sl], gq=g["gq_out"][sl], gqd=g["gqd_out"][sl], dt=float(g["dt"]))


def _run(eng, c, S, mm):
    n = c["q"].shape[0]
    ta = _T(c["act"])
    qo, qdo, ck = eng.forward(_T(c["q"]), _T(c["qd"]), ta, None, c["dt"], S, mm, True)
    r = eng.backward(ck, ta, None, c["dt"], S, mm, _T(c["gq"]), _T(c["gqd"]))
    torch.cuda.synchronize()
    eng.status()
    out = dict(q=qo.cpu().numpy().reshape(n, -1), qd=qdo.cpu().numpy().reshape(n, -1), gq=r[0].cpu().numpy().reshape(n, -1),
               gqd=r[1].cpu().numpy().reshape(n, -1), gact=r[2].cpu().numpy().reshape(n, -1), ckpt=ck.cpu().numpy())
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def _oracle_run(t, c, S, mm, tag):
    """the scalar oracle on a case, once per (case tag, S, mm), shared and never modified"""
    key = (tag, c["q"].shape[0], S, mm)
    if key not in _oracle:
        _oracle[key] = oracle_backward(t, c["q"], c["qd"], c["act"], None, c["dt"], S, mm, c["gq"], c["gqd"])
    return _oracle[key]


def _errors(t, c, r, o):
    return dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
                gq=relerr(project_tangent(t, c["q"], r["gq"]), project_tangent(t, c["q"], o["gq"])),
                gqd=relerr(r["gqd"], o["gqd"]), gact=relerr(r["gact"], o["gact"]))


def _assert_vs_oracle(t, c, r, o, label):
    e = _errors(t, c, r, o)
    print("%s: " % label + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4, e
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3, e


def _ckpt_words(t, ck, S, mm):
    """the words of a full checkpoint that the forward launch defines: per substep the saved block q .. qdd (f_tot and qdd, which
    the joint-space phase writes, are its last fields), then every group's inverse.  The alignment padding between and behind the
    blocks is never written, and the tail (end state, episode flags) is the fused environment kernels' alone"""
    from emu_lib import layout
    off, _ = layout(t)
    nd, nq = t.n_qd, t.n_q
    L, row = t.n_links, off["qdd"] + nd - off["q"]
    stride, hw, groups = (row + 3) & ~3, (nd * nd + 3) & ~3, (S + mm - 1) // mm
    assert ck.shape[1] >= S * stride + groups * hw
    # (fields are aligned: there are unwritten words between them; the free root's six rows of S are the identity and not stored)
    fields = [("q", 0, nq), ("qd", 0, nd), ("xsc", 0, 7 * L), ("S", 36, 6 * nd), ("v", 0, 6 * L), ("a", 0, 6 * L), ("i10", 0, 10 * L),
              ("ftot", 0, 6 * L), ("qdd", 0, nd)]
    parts = [ck[:, s * stride + off[f] - off["q"] + lo:s * stride + off[f] - off["q"] + hi] for s in range(S) for f, lo, hi in fields]
    parts += [ck[:, S * stride + g * hw:S * stride + g * hw + nd * nd] for g in range(groups)]
    return np.concatenate(parts, axis=1)


def _same(a, b, keys=KEYS, ckpt=None):
    """bit for bit on keys; ckpt = (t, S, mm): also on every defined word of the checkpoint"""
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    if ckpt is not None:
        wa, wb = _ckpt_words(ckpt[0], a["ckpt"], *ckpt[1:]), _ckpt_words(ckpt[0], b["ckpt"], *ckpt[1:])
        assert np.isfinite(wa).all() and np.array_equal(wa, wb), "checkpoint"


# ---- refresh schedules, operator level ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_refresh_schedules_vs_generic_kernels_and_oracle(t, n, mm):
    """the default (helper-wave) specialised kernels: the row of H^-1 in registers must be the group's at every substep of both
    launches; the generic kernels of the same library reload everything from LDS"""
    c = _case(n)
    spec, gen = _engine(t), _engine(t, DSIM_FORCE_GENERIC="1")
    assert spec.variant > 0 and gen.variant == 0
    a, b = _run(spec, c, S4, mm), _run(gen, c, S4, mm)
    for k in KEYS:
        e = relerr(a[k], b[k])
        print("S=4 mm=%d N=%d specialised vs generic %s %.2e" % (mm, n, k, e))
        assert e < 1e-5, (k, e)
    _assert_vs_oracle(t, c, a, _oracle_run(t, c, S4, mm, "rec"), "S=4 mm=%d N=%d oracle" % (mm, n))


@pytest.mark.parametrize("n", NS)
def test_recorded_step_vs_recording(t, n):
    """ant_step.npz (S = 16, one group): the reference's own outputs"""
    g = golden("ant_step")
    sl = slice(0, n)
    c = _case(n)
    r = _run(_engine(t), c, int(g["substeps"]), int(g["mm_freq"]))
    e = dict(q=relerr(r["q"], g["q_out"][sl]), qd=relerr(r["qd"], g["qd_out"][sl]),
             gq=relerr(project_tangent(t, c["q"], r["gq"]), project_tangent(t, c["q"], g["gq_in"][sl])),
             gqd=relerr(r["gqd"], g["gqd_in"][sl]), gact=relerr(r["gact"], g["gact_in"][sl]))
    print("recording N=%d: " % n + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3


# ---- kernel modes agree bit for bit at every schedule ---------------------------------------------------------------------------
@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_kernel_modes_agree_bit_for_bit(t, n, mm):
    """helper, single-wave, two-environments-per-wave (forward; it keeps the reload and the crossbar) and lean (its adjoint keeps
    the reload and takes the row broadcast) kernels: state, gradients, and the checkpoint words the joint-space phase writes"""
    from ckpt_fields import first_substep
    c = _case(n)
    ref = _run(_engine(t, **MODES["helper"]), c, S4, mm)
    single = _run(_engine(t, **MODES["single"]), c, S4, mm)
    _same(single, ref, ckpt=(t, S4, mm))   # (every row: q, qd, ..., f_tot, qdd; every group's inverse; tau is not saved)
    pair = _run(_engine(t, **MODES["pair"]), c, S4, mm)
    _same(pair, ref, ckpt=(t, S4, mm))
    fr, fp = first_substep(t, ref["ckpt"]), first_substep(t, pair["ckpt"])
    for k in ("ft_s", "qdd"):
        assert np.array_equal(fr[k], fp[k]), k
    for kw in (MODES["helper"], MODES["single"]):
        _same(_run(_engine(t, ckpt_mode="lean", **kw), c, S4, mm), ref)


# ---- launches that follow one another -------------------------------------------------------------------------------------------
TKE_ADD, LKE_SCALE = np.float32(3.0), np.float32(0.5)   # (Ant's joint_target_ke is 0, its joint_limit_ke 1000)


def _with_gains(t):
    t2 = copy.deepcopy(t)
    t2.joint_target_ke = (np.asarray(t.joint_target_ke, np.float32) + TKE_ADD).astype(np.float32)
    t2.joint_limit_ke = (np.asarray(t.joint_limit_ke, np.float32) * LKE_SCALE).astype(np.float32)
    return t2


@pytest.mark.parametrize("n", NS)
def test_launches_after_other_actions_and_other_gains(t, n):
    """one model: a step, a step with other actions, then Engine.set_params with other joint_target_ke / joint_limit_ke and a third
    step -- each equals, bit for bit, the same step on a fresh model built with those values"""
    c1 = _limits_case(t, n)      # (hinges outside their limits: both gains act)
    c2 = dict(c1, act=(-0.5 * c1["act"] + 0.25).astype(np.float32))
    eng = _engine(t, fresh=True)
    r1 = _run(eng, c1, S4, 2)
    r2 = _run(eng, c2, S4, 2)
    t3 = _with_gains(t)
    p = eng.step_parameters()
    p.joint_target_ke = _T(t3.joint_target_ke)
    p.joint_limit_ke = _T(t3.joint_limit_ke)
    eng.set_params(p)
    r3 = _run(eng, c2, S4, 2)
    _same(r1, _run(_engine(t, fresh=True), c1, S4, 2), ckpt=(t, S4, 2))
    _same(r2, _run(_engine(t, fresh=True), c2, S4, 2), ckpt=(t, S4, 2))
    f3 = _engine(t3, fresh=True)
    assert f3.variant > 0
    _same(r3, _run(f3, c2, S4, 2), ckpt=(t, S4, 2))
    assert not np.array_equal(r3["q"], r2["q"]) and not np.array_equal(r2["q"], r1["q"])


def _ant_env(n, mm):
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=n, device=DEV, render=False, seed=0, episode_length=1000, no_grad=False, stochastic_init=False,
                    MM_caching_frequency=mm, early_termination=False)
    assert e.fused
    return e


def _env_rollout(n, mm, actions, q0, qd0, generic=False, **kw):
    """H fused env steps from (q0, qd0) on a new AntEnv -> obs, rew per step, d(-sum rew)/d actions, end state.  The model is
    created at the first step: the switches hold for the whole rollout"""
    with _switches(**kw):
        e = _ant_env(n, mm)
        e.clear_grad()
        e.reset()
        e.reset_with_state(_T(q0), _T(qd0))
        e.initialize_trajectory()
        acts = torch.tensor(np.ascontiguousarray(actions), device=DEV, requires_grad=True)
        loss, obs_l, rew_l = 0.0, [], []
        for s in range(acts.shape[0]):
            obs, rew, done, info = e.step(acts[s])
            assert int(done.sum()) == 0
            obs_l.append(obs.detach().cpu().numpy().copy())
            rew_l.append(rew.detach().cpu().numpy().copy())
            loss = loss - rew.sum()
        loss.backward()
        torch.cuda.synchronize()
        assert (e.model.engine().variant == 0) == generic
    return dict(obs=np.stack(obs_l), rew=np.stack(rew_l), ga=acts.grad.cpu().numpy().copy(),
                q=e.state.joint_q.detach().cpu().numpy().copy(), qd=e.state.joint_qd.detach().cpu().numpy().copy())


def _env_inputs(n):
    g = golden("ant_rollout_mm1")
    rng = np.random.default_rng(23)
    acts = np.tanh(rng.normal(size=(2, n, g["actions"].shape[2]))).astype(np.float32)   # two steps, different actions
    return g["q0"][:n], g["qd0"][:n], acts


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_fused_env_steps_at_every_schedule(n, mm):
    """two consecutive AntEnv steps (16 substeps each: groups of mm, an uneven last group at mm = 3) with different actions: the
    kernel modes agree bit for bit; the generic kernels of the same library at 1e-4 (obs, rew, state) / 1e-3 (action gradients)"""
    q0, qd0, acts = _env_inputs(n)
    ref = _env_rollout(n, mm, acts, q0, qd0, **MODES["helper"])
    for name in ("single", "pair"):
        r = _env_rollout(n, mm, acts, q0, qd0, **MODES[name])
        for k in ref:
            assert np.array_equal(r[k], ref[k]), (name, k)
    gen = _env_rollout(n, mm, acts, q0, qd0, generic=True, DSIM_FORCE_GENERIC="1")
    e = {k: relerr(ref[k], gen[k]) for k in ref}
    print("AntEnv mm=%d N=%d specialised vs generic: " % (mm, n) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["obs"] < 1e-4 and e["rew"] < 1e-4 and e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["ga"] < 1e-3
    # the second step alone, from the first step's end state on a fresh environment: the same end state, bit for bit
    one = _env_rollout(n, mm, acts[:1], q0, qd0, **MODES["helper"])
    two = _env_rollout(n, mm, acts[1:], one["q"].reshape(n, -1), one["qd"].reshape(n, -1), **MODES["helper"])
    assert np.array_equal(two["q"], ref["q"]) and np.array_equal(two["qd"], ref["qd"])


def test_fused_env_replays_the_recorded_rollout_mm1():
    """ant_rollout_mm1.npz (a refresh in every substep: the row of H^-1 changes in every substep of both launches), its first three
    environments through the fused AntEnv against the recording's observations, rewards, action gradients and end state: 1e-3,
    cosine of the action gradients above 0.9999 (tests/test_gpu_envs.py)"""
    g = golden("ant_rollout_mm1")
    n, mm = 3, int(g["mm_freq"])
    assert mm == 1
    r = _env_rollout(n, mm, g["actions"][:, :n], g["q0"][:n], g["qd0"][:n])
    assert relerr(r["obs"], g["obs"][:, :n]) < 1e-3
    assert np.abs(r["rew"] - g["rew"][:, :n]).max() < 1e-3 * max(1.0, np.abs(g["rew"]).max())
    ga, gr = r["ga"].astype(np.float64), g["grad_actions"][:, :n].astype(np.float64)
    cos = (ga * gr).sum() / (np.linalg.norm(ga) * np.linalg.norm(gr))
    print("rollout_mm1 N=3: action gradients %.2e  cosine %.7f" % (relerr(ga, gr), cos))
    assert cos > 0.9999 and relerr(ga, gr) < 1e-3
    assert relerr(r["q"].reshape(n, -1), g["q_final"][:n]) < 1e-3


def test_graph_replay_after_set_params_equals_fresh_eager_model():
    """the same two steps captured as one graph on an environment whose model took other gains through Engine.set_params: every
    replay gives the eager result of an environment that was given those gains the same way and never ran under the old ones"""
    from diffrl_amd.graph import GraphedRollout
    n, mm = 3, 3
    q0, qd0, acts = _env_inputs(n)

    def with_gains(e):
        eng = e.model.engine()
        p = eng.step_parameters()
        p.joint_target_ke = _T((p.joint_target_ke.cpu().numpy() + TKE_ADD).astype(np.float32))
        p.joint_limit_ke = _T((p.joint_limit_ke.cpu().numpy() * LKE_SCALE).astype(np.float32))
        eng.set_params(p)

    def body_for(a):
        def body(env):
            env.initialize_trajectory()
            return -torch.stack([env.step(a_t)[1] for a_t in a.unbind(0)]).sum()
        return body

    def prepared(run_before):
        e = _ant_env(n, mm)
        e.clear_grad()
        e.reset()
        e.reset_with_state(_T(q0), _T(qd0))
        if run_before:   # steps under the template's gains first: nothing of them may survive into the later launches
            with torch.no_grad():
                e.step(torch.tensor(acts[0], device=DEV))
            e.reset()
            e.reset_with_state(_T(q0), _T(qd0))
        with_gains(e)
        return e

    e1 = prepared(False)
    a1 = torch.tensor(acts, device=DEV, requires_grad=True)
    loss1 = body_for(a1)(e1)
    loss1.backward()
    torch.cuda.synchronize()
    e2 = prepared(True)
    a2 = torch.tensor(acts, device=DEV, requires_grad=True)
    roll = GraphedRollout(e2, body_for(a2), leaves=[a2], carry_state=False)
    for _ in range(2):
        loss2 = roll.replay()
    torch.cuda.synchronize()
    assert float(loss2) == float(loss1.detach())
    assert torch.equal(a2.grad, a1.grad)


# ---- limit branches: the hoisted lower / upper / lke feed them ------------------------------------------------------------------
def _limits_case(t, n):
    """the recorded start states with one hinge below its lower limit and one above its upper limit in every environment"""
    c = _case(n)
    q = c["q"].copy()
    jt, qs = np.asarray(t.joint_type), np.asarray(t.joint_q_start)
    hinges = [int(qs[i]) for i in range(t.n_links) if int(jt[i]) in (0, 1)]
    lo, hi = np.asarray(t.joint_limit_lower, np.float32), np.asarray(t.joint_limit_upper, np.float32)
    for e in range(n):
        a, b = hinges[(2 * e) % len(hinges)], hinges[(2 * e + 3) % len(hinges)]
        q[e, a] = lo[a] - np.float32(0.2)
        q[e, b] = hi[b] + np.float32(0.2)
    return dict(c, q=q)


@pytest.mark.parametrize("n", NS)
def test_hinges_below_and_above_their_limits(t, n):
    c = _limits_case(t, n)
    jt, qs = np.asarray(t.joint_type), np.asarray(t.joint_q_start)
    hinges = [int(qs[i]) for i in range(t.n_links) if int(jt[i]) in (0, 1)]
    lo, hi = np.asarray(t.joint_limit_lower), np.asarray(t.joint_limit_upper)
    assert (c["q"][:, hinges] < lo[hinges]).any(axis=1).all() and (c["q"][:, hinges] > hi[hinges]).any(axis=1).all()
    ref = _run(_engine(t, **MODES["helper"]), c, S4, 2)
    _assert_vs_oracle(t, c, ref, _oracle_run(t, c, S4, 2, "limits"), "limits N=%d oracle" % n)
    gen = _run(_engine(t, DSIM_FORCE_GENERIC="1"), c, S4, 2)
    for k in KEYS:
        assert relerr(ref[k], gen[k]) < 1e-5, k
    for name in ("single", "pair"):
        _same(_run(_engine(t, **MODES[name]), c, S4, 2), ref)
    _same(_run(_engine(t, ckpt_mode="lean"), c, S4, 2), ref)
