"""-m gpu: per-environment step parameters (dsim_model_reserve_env_params / dsim_model_set_env_params, Engine.set_env_params,
EnvStepParameters through the integrator, DFlexEnv.randomize_step_parameters) on the real HIP kernels.

The reference of a per-environment launch is the SAME kernels in shared mode: environment e under row e must give the bits of an
N = 1 launch on a second Engine under set_params(row e) -- the only difference is the address the constants are fetched from -- so
every comparison with it is torch.equal.  Shapes: N = 3 environments (odd: a pair has an empty half), 3 substeps with the mass
matrix refreshed every 2 (a group ends inside the step), the same start state, actuation and cotangents in every environment, so
that only the parameters differ; row e holds the template's values times a distinct factor per field and row, the contact mu and
kf ordered differently from ke so that the rows do not all take the same friction branch."""
import gc
import importlib.util
import os

import numpy as np
import pytest
import torch

import par_lib as P
from oracle_lib import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, S, MM = 3, 3, 2
FACTORS = dict(joint_target_ke=(0.6, 1.0, 1.7), joint_target_kd=(1.7, 0.6, 1.0), joint_limit_ke=(1.0, 1.7, 0.6),
               joint_limit_kd=(0.6, 1.7, 1.0), joint_target=(1.7, 1.0, 0.6))
CONTACT_FACTORS = ((0.6, 1.0, 1.7), (1.0, 1.7, 0.6), (1.7, 0.6, 1.0), (1.0, 1.7, 0.6))   # ke, kd, kf, mu
# the row of tests/golden/<env>_par.npz that is the one environment: on the ground, contacts in both friction branches
FIXTURE_ROW = dict(ant=7, humanoid=9, snu=4, cartpole=0)


def _engine(t, monkeypatch, generic=False, lean=False, **kw):
    from diffrl_amd.engine import Engine
    if generic:
        monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    return Engine(t, torch.device(DEV), ckpt_mode="lean" if lean else "full", **kw)


def _T(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV).reshape(-1) if a is not None else None


def _tile(x, n):
    return x.view(1, -1).repeat(n, 1).reshape(-1).contiguous() if x is not None else None


def _rows(eng):
    """the template's values times the factors above: an EnvStepParameters of N rows"""
    p = eng.env_step_parameters(N)
    for k, f in FACTORS.items():
        getattr(p, k).mul_(torch.tensor(f, device=DEV).view(N, 1))
    for j, f in enumerate(CONTACT_FACTORS):
        p.contact_material[:, :, j] *= torch.tensor(f, device=DEV).view(N, 1)
    return p


def _row(p, e):
    from diffrl_amd.engine import StepParameters
    return StepParameters(**{k: getattr(p, k)[e].clone().contiguous() for k in p.FIELDS})


def _case(name):
    """(template, ONE environment's q, qd, act, muscle_act | None, gq_out, gqd_out as flat device tensors, dt)"""
    if name == "user_tree":
        from diffrl_amd.template import ArticulationTemplate
        from test_edge_cases_cpu import _tree_states
        t = ArticulationTemplate.load(os.path.join(ROOT, "tests", "golden", "user_tree.npz"))
        rng = np.random.default_rng(11)
        q, qd, act = _tree_states(t, rng, 1)
        q[:, 1] -= 0.2   # (towards the ground: some of its contacts penetrate)
        gq, gqd = rng.normal(0, 1, q.shape).astype(np.float32), rng.normal(0, 1, qd.shape).astype(np.float32)
        return t, _T(q), _T(qd), _T(act), None, _T(gq), _T(gqd), S / 960.0
    t, g, (act, mact) = P.case(name)
    r = slice(FIXTURE_ROW[name], FIXTURE_ROW[name] + 1)
    return (t, _T(g["q_in"][r]), _T(g["qd_in"][r]), _T(act[r]), _T(mact[r]) if mact is not None else None, _T(g["gq_out"][r]),
            _T(g["gqd_out"][r]), float(g["dt"]))


def _forward(eng, n, q, qd, act, mact, step):
    """dsim_step_forward into a ZEROED checkpoint: the words between the padded arrays of a row are never written, so that two
    checkpoints can be compared whole"""
    import ctypes as C
    p = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    qo, qdo = torch.empty_like(q), torch.empty_like(qd)
    ck = torch.zeros(n, int(eng._lib.dsim_ckpt_floats_mm(eng._h, step[1], step[2])), device=DEV)
    eng._call(eng._lib.dsim_step_forward, eng._h, n, p(q), p(qd), p(act), p(mact if eng.n_muscles else None), C.c_float(step[0]),
              step[1], step[2], p(qo), p(qdo), p(ck))
    return qo, qdo, ck


def _everything(eng, t, n, one, extras):
    """every launch kind the parameters reach, for n copies of the one environment of _case -> {name: [n, .] tensor}"""
    _, q, qd, act, mact, gq, gqd, dt = one
    q, qd, act, mact, gq, gqd = (_tile(x, n) for x in (q, qd, act, mact, gq, gqd))
    step = (dt, S, MM)
    out = {}
    out["q_out"], out["qd_out"], ck = _forward(eng, n, q, qd, act, mact, step)
    out["ckpt"] = ck
    b = eng.backward(ck, act, mact, *step, gq, gqd)
    out.update({"bwd_" + k: v for k, v in zip(("gq", "gqd", "gact", "gmact"), b) if v is not None})
    bp = eng.backward_params(ck, act, mact, *step, gq, gqd)
    out.update({"par_" + k: v for k, v in zip(("gq", "gqd", "gact", "gmact", "g_dof", "g_contact"), bp) if v is not None})
    if extras:
        J = eng.step_jacobian(ck, act, mact, *step)
        out.update({"jac_" + k: v for k, v in zip(("state", "act"), J[:2])})
        lit = eng.backward(ck, act, mact, *step, gq, gqd, literal=True)
        out.update({"lit_" + k: v for k, v in zip(("gq", "gqd", "gact"), lit[:3])})
    # the read-outs, forward and backward (seeded cotangents, the same in every environment)
    gen = torch.Generator().manual_seed(5)
    jd = eng.joint_dynamics_forward(q, qd, act, mact)
    out.update({"jd_" + k: v for k, v in zip(("tau", "qdd", "f_s"), jd)})
    cot = [_tile(torch.randn(v.numel() // n, generator=gen).to(DEV), n) for v in jd]
    gjd = eng.joint_dynamics_backward(q, qd, act, mact, *cot)
    out.update({"jd_g%d" % i: v for i, v in enumerate(gjd) if v is not None})
    gc_ = eng.ground_contacts_forward(q, qd)
    out.update({"gc_" + k: v for k, v in zip(("point", "vel", "force", "link_wrench"), gc_)})
    cot = [_tile(torch.randn(v.numel() // n, generator=gen).to(DEV), n) if v.numel() else None for v in gc_]
    ggc = eng.ground_contacts_backward(q, qd, *cot)
    out.update({"gc_g%d" % i: v for i, v in enumerate(ggc) if v is not None})
    torch.cuda.synchronize()
    eng.status()
    return {k: v.reshape(n, -1) for k, v in out.items()}


_refs = {}


def _reference(name, generic, lean, monkeypatch):
    """the three shared N = 1 runs on an Engine of their own, one per row of _rows: computed once per model and kernel set,
    moved to the host and left unchanged"""
    key = (name, generic, lean)
    if key not in _refs:
        one = _case(name)
        eng = _engine(one[0], monkeypatch, generic, lean, **({"specialise": True} if name == "user_tree" else {}))
        p = _rows(eng)
        rows = []
        for e in range(N):
            eng.set_params(_row(p, e))
            rows.append({k: v.cpu() for k, v in _everything(eng, one[0], 1, one, extras=name == "ant").items()})
        _refs[key] = rows
    return _refs[key]


def _assert_rows_equal(got, rows, label, n=N):
    for e in range(n):
        assert sorted(got) == sorted(rows[e]), label
        for k in got:
            assert torch.equal(got[k][e].cpu(), rows[e][k][0]), "%s: %s of environment %d differs from the shared run under its row" % (label, k, e)


CONFIGS = [("ant", False, False), ("ant", False, True), ("humanoid", False, False), ("snu", False, False), ("snu", False, True),
           ("cartpole", False, False), ("ant", True, False), ("user_tree", False, False)]


@pytest.mark.parametrize("name,generic,lean", CONFIGS, ids=["%s-%s-%s" % (n, "generic" if g else "own", "lean" if l else "full")
                                                            for n, g, l in CONFIGS])
def test_rows_equal_shared_runs_bit_for_bit(name, generic, lean, monkeypatch):
    rows = _reference(name, generic, lean, monkeypatch)
    one = _case(name)
    t = one[0]
    eng = _engine(t, monkeypatch, generic, lean, **({"specialise": True} if name == "user_tree" else {}))
    assert eng.env_params() == 0
    eng.set_env_params(_rows(eng))
    assert eng.env_params() == N
    got = _everything(eng, t, N, one, extras=name == "ant")
    _assert_rows_equal(got, rows, "%s %s %s" % (name, "generic" if generic else "own kernels", "lean" if lean else "full"))
    # not vacuous: the parameters matter, and the rows are not each other's
    assert not torch.equal(got["q_out"][0], got["q_out"][1]) and not torch.equal(got["q_out"][1], got["q_out"][2])
    if t.n_contacts:   # contacts penetrate, and over the rows both friction branches occur (kf in one, mu in the other)
        gcon = got["par_g_contact"].view(N, t.n_contacts, 4)
        assert all(float(gcon[:, :, j].abs().max()) > 0 for j in range(4)), name
    print("%s variant %d waves %d: %d tensors x %d rows equal the shared runs" % (name, eng.variant, eng.waves, len(got), N))


def _env(name, n):
    from diffrl_amd import envs
    cls = dict(ant=envs.AntEnv, humanoid=envs.HumanoidEnv, snu=envs.SNUHumanoidEnv)[name]
    return cls(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=MM)


def _fused(eng, spec, n, one, n_act):
    """env_forward with episode bookkeeping, then env_backward, for n copies of the one environment -> {name: [n, .] tensor}"""
    from diffrl_amd.engine import EpisodeIO
    _, q, qd, _, _, gq, gqd, dt = one
    gen = torch.Generator().manual_seed(9)
    actions = _tile((2.0 * torch.rand(n_act, generator=gen) - 1.0).to(DEV), n)
    gobs, grew = _tile(torch.randn(spec.n_obs, generator=gen).to(DEV), n), _tile(torch.randn(1, generator=gen).to(DEV), n)
    q, qd, gq, gqd = (_tile(x, n) for x in (q, qd, gq, gqd))
    ep = EpisodeIO(torch.zeros(n, dtype=torch.int64, device=DEV), q.view(1, n, -1).clone(), qd.view(1, n, -1).clone(),
                   torch.zeros(n, dtype=torch.int32, device=DEV), 1000, False, False, want_obs_before=True)
    qo, qdo, obs, rew, ck, obs_before, done = eng.env_forward(spec, q, qd, actions, dt, S, MM, True, ep)
    g = eng.env_backward(spec, ck, actions, dt, S, MM, gq, gqd, gobs, grew)
    torch.cuda.synchronize()
    eng.status()
    out = dict(q_out=qo, qd_out=qdo, obs=obs, rew=rew, obs_before=obs_before, done=done.float(), gq=g[0], gqd=g[1], gactions=g[2])
    return {k: v.reshape(n, -1) for k, v in out.items()}


@pytest.mark.parametrize("name", ["ant", "humanoid", "snu"])
def test_fused_env_kernels_rows_equal_shared_launches(name, monkeypatch):
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    env = _env(name, N)   # (its spec -- action mapping, observation, reward -- does not depend on the number of environments)
    spec, eng, n_act = env._spec(), env.model.engine(), env.num_actions
    one = _case(name)
    p = _rows(eng)
    eng.set_env_params(p)
    got = _fused(eng, spec, N, one, n_act)
    eng2 = _engine(env.model.template(), monkeypatch)
    rows = []
    for e in range(N):
        eng2.set_params(_row(p, e))
        rows.append({k: v.cpu() for k, v in _fused(eng2, spec, 1, one, n_act).items()})
    _assert_rows_equal(got, rows, name + " fused env step")
    assert not torch.equal(got["obs"][0], got["obs"][1])
    eng.reset_params()


def test_randomized_environments_started_alike_observe_differently(monkeypatch):
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    from diffrl_amd.engine import EnvStepParameters
    env, one = _ant_on_the_ground(N)
    gen = torch.Generator(device=DEV).manual_seed(3)
    p = env.randomize_step_parameters({"contact_material": {"mu": (0.3, 1.7), "kf": (0.3, 1.7), 0: (0.5, 1.5)},
                                       "joint_target_ke": (0.5, 1.5), "joint_limit_kd": (0.5, 1.5)}, generator=gen)
    assert isinstance(p, EnvStepParameters) and env.model.engine().env_params() == N
    t0 = env.model.engine().step_parameters()
    f = p.contact_material[:, :, 3] / t0.contact_material[None, :, 3]
    assert float((f - f[:, :1]).abs().max()) < 1e-6 and float(f.min()) >= 0.3 - 1e-6 and float(f.max()) <= 1.7 + 1e-6   # one factor per environment
    assert len(set(f[:, 0].tolist())) == N
    assert torch.equal(p.joint_target_kd, t0.joint_target_kd[None].repeat(N, 1))        # a field not named keeps the template's values
    assert torch.equal(p.contact_material[:, :, 1], t0.contact_material[None, :, 1].repeat(N, 1))
    with torch.no_grad():   # the same state in every environment (the fixture's: on the ground), the same action
        env.state.joint_q, env.state.joint_qd = _tile(one[1], N), _tile(one[2], N)
        obs, rew, done, _ = env.step(torch.zeros((N, env.num_actions), device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all()) and not torch.equal(obs[0], obs[1]) and not torch.equal(obs[1], obs[2])
    env.model.engine().reset_params()
    with torch.no_grad():
        env.state.joint_q, env.state.joint_qd = _tile(one[1], N), _tile(one[2], N)
        obs, _, _, _ = env.step(torch.zeros((N, env.num_actions), device=DEV))
    assert torch.equal(obs[0], obs[1]) and torch.equal(obs[1], obs[2])   # back to one block: alike again


def test_pair_kernels_are_not_used_in_per_environment_mode(monkeypatch):
    """DSIM_HELPER=0 DSIM_PAIR=1: every shared-mode forward launch of Ant runs two environments per wavefront, which share one
    copy of the constants; per-environment mode must fall back to the plain kernels"""
    rows = _reference("ant", False, False, monkeypatch)
    monkeypatch.setenv("DSIM_HELPER", "0")
    monkeypatch.setenv("DSIM_PAIR", "1")
    one = _case("ant")
    t, q, qd, act, _, _, _, dt = one
    eng = _engine(t, monkeypatch)
    p = _rows(eng)
    eng.set_env_params(p)
    qo, qdo, ck = _forward(eng, N, _tile(q, N), _tile(qd, N), _tile(act, N), None, (dt, S, MM))
    torch.cuda.synchronize()
    for e in range(N):
        assert torch.equal(qo.view(N, -1)[e].cpu(), rows[e]["q_out"][0]) and torch.equal(qdo.view(N, -1)[e].cpu(), rows[e]["qd_out"][0])
        assert torch.equal(ck[e].cpu(), rows[e]["ckpt"][0])
    # shared mode on the same Engine (the pair kernels): every environment equals the shared run under those values
    eng.reset_params()
    eng.set_params(_row(p, 2))
    qo, qdo, ck = _forward(eng, N, _tile(q, N), _tile(qd, N), _tile(act, N), None, (dt, S, MM))
    torch.cuda.synchronize()
    for e in range(N):
        assert torch.equal(qo.view(N, -1)[e].cpu(), rows[2]["q_out"][0]) and torch.equal(qdo.view(N, -1)[e].cpu(), rows[2]["qd_out"][0])
    eng.status()


def test_mode_changes(monkeypatch):
    import ctypes as C
    from diffrl_amd import capi
    rows = _reference("ant", False, False, monkeypatch)
    one = _case("ant")
    t, q, qd, act, _, _, _, dt = one
    step = (dt, S, MM)
    eng = _engine(t, monkeypatch)
    run = lambda n: _forward(eng, n, _tile(q, n), _tile(qd, n), _tile(act, n), None, step)  # noqa: E731
    base = [x.cpu() for x in run(1)]
    x = torch.ones(N, t.n_links, device=DEV)
    with pytest.raises(capi.DsimError, match="reserve"):   # shared mode: no rows to write
        eng._call(eng._lib.dsim_model_set_env_params, eng._h, capi.PARAM_TARGET_KE, N, C.c_void_p(x.data_ptr()))
    p = _rows(eng)
    eng.set_env_params(p)
    with pytest.raises(capi.DsimError, match="null pointer"):
        eng._call(eng._lib.dsim_model_set_env_params, eng._h, capi.PARAM_TARGET_KE, N, None)
    with pytest.raises(capi.DsimError, match="unknown parameter field"):
        eng._call(eng._lib.dsim_model_set_env_params, eng._h, 6, N, C.c_void_p(x.data_ptr()))
    with pytest.raises(capi.DsimError, match="4.*3"):
        eng._call(eng._lib.dsim_model_set_env_params, eng._h, capi.PARAM_TARGET_KE, N + 1, C.c_void_p(x.data_ptr()))
    # more environments than rows: refused, naming both; fewer: the first rows
    with pytest.raises(capi.DsimError, match=r"n_envs = 4\b.*\b3 environments"):
        run(N + 1)
    qo, qdo, ck = run(2)
    torch.cuda.synchronize()
    for e in range(2):
        assert torch.equal(qo.view(2, -1)[e].cpu(), rows[e]["q_out"][0]) and torch.equal(ck[e].cpu(), rows[e]["ckpt"][0])
    # a shared set_params in per-environment mode is for ALL rows
    eng.set_params(_row(p, 1))
    assert eng.env_params() == N
    qo, qdo, ck = run(N)
    torch.cuda.synchronize()
    for e in range(N):
        assert torch.equal(qo.view(N, -1)[e].cpu(), rows[1]["q_out"][0]) and torch.equal(qdo.view(N, -1)[e].cpu(), rows[1]["qd_out"][0])
        assert torch.equal(ck[e].cpu(), rows[1]["ckpt"][0])
    # ... and the values all share are what a later reservation starts from
    eng.reserve_env_params(2)
    assert eng.env_params() == 2
    qo, _, _ = run(2)
    assert torch.equal(qo.view(2, -1)[1].cpu(), rows[1]["q_out"][0])
    # reset_params: one block again, the template's bits
    eng.reset_params()
    assert eng.env_params() == 0
    again = [x.cpu() for x in run(1)]
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    big = [x.cpu() for x in run(N + 1)]   # (no row limit in shared mode)
    assert torch.equal(big[0].view(N + 1, -1)[N], base[0].view(-1))
    eng.status()


def _ant_on_the_ground(n):
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=MM, early_termination=False)
    e.reset()
    one = _case("ant")
    with torch.no_grad():
        e.state.joint_q, e.state.joint_qd = _tile(one[1], n), _tile(one[2], n)
    return e, one


def test_autograd_returns_per_environment_gradients(monkeypatch):
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    from diffrl_amd.engine import EnvStepParameters
    e, one = _ant_on_the_ground(N)
    model, integ, eng = e.model, e.integrator, e.model.engine()
    _, q1, qd1, act1, _, gq1, gqd1, dt = one
    q, qd, act, cq, cqd = (_tile(x, N) for x in (q1, qd1, act1, gq1, gqd1))
    step = (dt, S, MM)

    def leaves(p):
        for k in p.FIELDS:
            setattr(p, k, getattr(p, k).clone().requires_grad_(True))
        return p

    def run(p):
        s = model.state()
        s.joint_q, s.joint_qd, s.joint_act = q.clone().requires_grad_(True), qd.clone(), act
        s1 = integ.forward(model, s, *step, params=p)
        ((s1.joint_q * cq).sum() + (s1.joint_qd * cqd).sum()).backward()
        return s, s1

    p = leaves(_rows(eng))
    assert isinstance(model.step_parameters(per_env=True), EnvStepParameters)
    s, s1 = run(p)
    # the raw launches under the same values, folded without the sum over the environments
    eng.set_env_params([x.detach() for x in p.tensors()])
    a = eng.forward(q, qd, act, None, *step, True)
    b = eng.backward_params(a[2], act, None, *step, cq, cqd)
    f = eng.fold_param_grads(b[4], b[5], per_env=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], s1.joint_q.detach()) and torch.equal(s.joint_q.grad, b[0])
    for k, x in zip(p.FIELDS, f):
        got = getattr(p, k).grad
        assert got is not None and got.shape == getattr(p, k).shape and got.shape[0] == N, k
        assert torch.equal(got, x.view(got.shape)), k
    assert float(p.contact_material.grad.abs().max()) > 0 and not torch.equal(p.contact_material.grad[0], p.contact_material.grad[1])
    # all rows equal: the sum over the rows is the gradient of the shared tensor (SimStepParams), up to the fp32 re-association of
    # at most 3 N terms per entry -- 1e-5 relative in each tensor's max-norm
    pe = leaves(model.step_parameters(per_env=True))
    run(pe)
    eng.reset_params()
    ps = model.step_parameters()
    for k in ps.FIELDS:
        setattr(ps, k, getattr(ps, k).requires_grad_(True))
    run(ps)
    torch.cuda.synchronize()
    for k in ps.FIELDS:
        want, got = getattr(ps, k).grad, getattr(pe, k).grad.sum(0)
        if float(want.abs().max()) == 0:
            assert float(got.abs().max()) == 0, k
            continue
        err = relerr(got.cpu().numpy(), want.cpu().numpy())
        print("%s: sum of the per-environment gradients against the shared gradient %.2e" % (k, err))
        assert err < 1e-5, (k, err)
    eng.reset_params()
    eng.status()


def test_graphed_rollout_with_per_environment_leaves(monkeypatch):
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    from diffrl_amd import capi
    from diffrl_amd.engine import EnvStepParameters
    from diffrl_amd.graph import GraphedRollout
    e, one = _ant_on_the_ground(N)
    model, integ, eng = e.model, e.integrator, e.model.engine()
    base = _rows(eng)
    eng.set_env_params(base)   # reserved before anything is captured
    nd, H = model.dofs_per_articulation, 2
    acts = torch.zeros((H, N, nd), device=DEV)
    acts[:, :, 6:] = 100.0
    q0, qd0 = e.state.joint_q.detach().clone(), e.state.joint_qd.detach().clone()
    stat = torch.zeros(1, device=DEV)

    def make_body(cm, tke):
        def body(env):
            p = EnvStepParameters(**{k: getattr(base, k) for k in base.FIELDS})
            p.contact_material, p.joint_target_ke = cm, tke
            st = env.state
            for h in range(H):
                st.joint_act = acts[h].reshape(-1)
                st = integ.forward(model, st, env.sim_dt, S, MM, params=p)
            env.state = st
            loss = (st.joint_q.view(N, -1)[:, 0] ** 2).sum() + (st.joint_qd ** 2).sum()
            stat.copy_(loss.detach().view(1))
            return loss
        return body

    def eager(cm_values, tke_values):
        cm, tke = cm_values.clone().requires_grad_(True), tke_values.clone().requires_grad_(True)
        st = model.state()
        st.joint_q, st.joint_qd = q0.clone(), qd0.clone()
        e.state = st
        make_body(cm, tke)(e).backward()
        torch.cuda.synchronize()
        return float(stat), cm.grad.clone(), tke.grad.clone()

    v0 = (base.contact_material.clone(), base.joint_target_ke.clone())
    v1 = (v0[0] * torch.tensor([1.0, 1.0, 0.5, 0.5], device=DEV), v0[1] * 1.5 + 0.25)
    ref0, ref1 = eager(*v0), eager(*v1)
    assert ref0[0] != ref1[0] and np.isfinite(ref0[0]) and float(ref0[1].abs().max()) > 0
    # (no autograd graph of the eager runs may be alive at the capture: graph.py)
    st = model.state()
    st.joint_q, st.joint_qd = q0.clone(), qd0.clone()
    e.state = st
    gc.collect()
    cm, tke = v0[0].clone().requires_grad_(True), v0[1].clone().requires_grad_(True)
    roll = GraphedRollout(e, make_body(cm, tke), leaves=[cm, tke], carry_state=False)
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) == ref0[0] and torch.equal(cm.grad, ref0[1]) and torch.equal(tke.grad, ref0[2])
    assert cm.grad.shape == (N, model.template().n_contacts, 4) and tke.grad.shape == (N, model.template().n_links)
    with torch.no_grad():   # in place: the next replay runs under the new values
        cm.copy_(v1[0])
        tke.copy_(v1[1])
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) == ref1[0] and torch.equal(cm.grad, ref1[1]) and torch.equal(tke.grad, ref1[2])
    # the reservation itself is refused on a capturing stream, and changes nothing
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        with pytest.raises(capi.DsimError, match="capture"):
            eng._call(eng._lib.dsim_model_reserve_env_params, eng._h, N + 2)
        stat.add_(0.0)
    torch.cuda.synchronize()
    assert eng.env_params() == N
    eng.reset_params()
    eng.status()


def test_the_example_runs_in_both_modes(capsys):
    """examples/domain_rand_lite.py, two iterations, eager and captured: finite losses"""
    spec = importlib.util.spec_from_file_location("domain_rand_lite", os.path.join(ROOT, "examples", "domain_rand_lite.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for flags in ([], ["--graph"]):
        hist = ex.main(["--envs", "16", "--horizon", "4", "--iters", "2"] + flags)
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("loss:")]
        assert len(line) == 1 and ("graph" if flags else "eager") in line[0], line
        assert len(hist) == 2 and all(np.isfinite(v) for row in hist for v in row)
