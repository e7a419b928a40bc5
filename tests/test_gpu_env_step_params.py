"""-m gpu: parameter gradients through the fused env.step on the real HIP kernels -- dsim_env_step_backward_params,
Engine.env_backward_params, EnvStepParams, DFlexEnv.set_step_parameters, GraphedRollout with parameter leaves.

Shapes: N = 3 environments, substeps = 4, the mass matrix refreshed every 2nd substep (tests/env_par_lib.py), the start states of
the recordings tests/golden/<env>_envpar.npz (on the ground; one past two joint limits).  References:
  * the recordings of the reference's own env class, per parameter tensor within max(1e-4, 10 x its recorded noise);
  * the device's own dsim_env_step_backward (state gradients) and dsim_step_backward_params on the fused forward's checkpoint
    (parameter outputs under zero gobs / grew / gobs_before), bit for bit;
  * in per-environment mode, an N = 1 shared launch under row e, bit for bit.
"""
import gc
import os

import numpy as np
import pytest
import torch

import env_par_lib as E
from oracle_lib import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, S, MM = 3, E.SUBSTEPS, E.MM
# (model, generic kernels, lean checkpoints)
CONFIGS = [("ant", False, False), ("ant", False, True), ("ant", True, False), ("humanoid", False, False), ("snu", False, False),
           ("cartpole", False, False), ("user_tree", False, False)]
IDS = ["%s-%s-%s" % (n, "generic" if g else "own", "lean" if l else "full") for n, g, l in CONFIGS]
FACTORS = (0.7, 1.0, 1.5)   # per-environment rows: the template's values times these


def _T(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV) if a is not None else None


def _engine(t, monkeypatch, generic=False, lean=False, **kw):
    from diffrl_amd.engine import Engine
    if generic:
        monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    return Engine(t, torch.device(DEV), ckpt_mode="lean" if lean else "full", **kw)


_keep = []


def _case(name):
    """(template, spec with a DEVICE act_scale, host act_scale, dt, dict of N-environment inputs as host arrays)"""
    from diffrl_amd import capi
    rs = np.random.RandomState(3)
    if name == "user_tree":
        from diffrl_amd.template import ArticulationTemplate
        from test_edge_cases_cpu import _tree_states
        t = ArticulationTemplate.load(os.path.join(ROOT, "tests", "golden", "user_tree.npz"))
        na = t.n_qd - 6
        scale = np.full(na, 30.0, np.float32)
        q, qd, _ = _tree_states(t, np.random.default_rng(11), N)
        q[:, 1] -= 0.2   # (towards the ground: some of its contacts penetrate)
        a = rs.uniform(-0.9, 0.9, (N, na)).astype(np.float32)
        dt = S / 960.0
        mk = lambda p: capi.make_env_spec(capi.ENV_LOCOMOTION, capi.REW_ANT, na, 13 + (t.n_q - 7) + (t.n_qd - 6) + na, p, act_offset=6,  # noqa: E731
                                          obs_actions=True, inv_start_rot=(0.0, 0.0, 0.0, 1.0), target_xz=(100.0, 0.0),
                                          termination_height=0.0)
    else:
        t, g, host_spec, scale = E.case(name)
        q, qd, a, dt = g["q0"][-N:], g["qd0"][-N:], g["actions"][0][-N:].copy(), float(g["dt"])
        mk = None
    dscale = _T(scale)
    _keep.append(dscale)
    if mk is not None:
        spec = mk(dscale.data_ptr())
    else:
        spec = type(host_spec).from_buffer_copy(host_spec)
        spec.act_scale = dscale.data_ptr()
    c = dict(q=q, qd=qd, a=a, gq=rs.normal(size=(N, t.n_q)).astype(np.float32), gqd=rs.normal(size=(N, t.n_qd)).astype(np.float32),
             gobs=rs.normal(size=(N, spec.n_obs)).astype(np.float32), grew=rs.normal(size=N).astype(np.float32),
             gobs_b=rs.normal(size=(N, spec.n_obs)).astype(np.float32))
    return t, spec, scale, dt, c


def _nanlike(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _raw_backward_params(eng, spec, ck, a, dt, cots, want=(True, True)):
    """dsim_env_step_backward_params into NaN-filled buffers: what comes back was written"""
    import ctypes as C
    n, t = ck.shape[0], eng.template
    p = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    gq, gqd, ga = _nanlike(n, t.n_q), _nanlike(n, t.n_qd), _nanlike(n, spec.n_act)
    g_dof = _nanlike(n, 5, t.n_qd) if want[0] else None
    g_con = _nanlike(n, t.n_contacts, 4) if want[1] else None
    eng._call(eng._lib.dsim_env_step_backward_params, eng._h, C.byref(spec), n, p(ck), p(a), C.c_float(dt), S, MM, *[p(x) for x in cots],
              p(gq), p(gqd), p(ga), p(g_dof), p(g_con))
    return dict(gq=gq, gqd=gqd, ga=ga, g_dof=g_dof, g_contact=g_con)


def _launches(eng, t, spec, scale, dt, c, n=N, rows=slice(None)):
    """fused forward (no episode), the parameter adjoint under full cotangents and under the state cotangents alone, the plain fused
    adjoint and the step parameter adjoint on the same checkpoint -> dict of [n, .] tensors"""
    q, qd, a = (_T(c[k][rows]).reshape(-1) for k in ("q", "qd", "a"))
    cots = [_T(c[k][rows]).reshape(-1) for k in ("gq", "gqd", "gobs", "grew", "gobs_b")]
    qo, qdo, obs, rew, ck = eng.env_forward(spec, q, qd, a, dt, S, MM, True)
    par = _raw_backward_params(eng, spec, ck, a, dt, cots)
    plain = eng.env_backward(spec, ck, a, dt, S, MM, *cots)
    zero = _raw_backward_params(eng, spec, ck, a, dt, cots[:2] + [None, None, None])
    act, mact = E.joint_actuation(t, spec, scale, c["a"][rows])
    step = eng.backward_params(ck, _T(act).reshape(-1), _T(mact).reshape(-1) if mact is not None else None, dt, S, MM, *cots[:2])
    torch.cuda.synchronize()
    eng.status()
    out = dict(q_out=qo, obs=obs, rew=rew, plain_gq=plain[0], plain_gqd=plain[1], plain_ga=plain[2], step_g_dof=step[4],
               step_g_contact=step[5])
    out.update({"par_" + k: v for k, v in par.items()})
    out.update({"zero_" + k: v for k, v in zero.items()})
    return {k: v.reshape(n, -1) for k, v in out.items()}


def _user(name):
    return {"specialise": True} if name == "user_tree" else {}


@pytest.mark.parametrize("name,generic,lean", CONFIGS, ids=IDS)
def test_equals_the_devices_own_adjoints_bit_for_bit(name, generic, lean, monkeypatch):
    """(a) gq_in / gqd_in / gactions are dsim_env_step_backward's; (b) with zero gobs / grew / gobs_before the parameter outputs are
    dsim_step_backward_params' on the fused forward's checkpoint.  Every word of every output is written."""
    t, spec, scale, dt, c = _case(name)
    eng = _engine(t, monkeypatch, generic, lean, **_user(name))
    r = _launches(eng, t, spec, scale, dt, c)
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
    for k in ("gq", "gqd", "ga"):
        assert torch.equal(r["par_" + k], r["plain_" + k]), k
    assert torch.equal(r["zero_g_dof"], r["step_g_dof"]) and float(r["zero_g_dof"].abs().max()) > 0
    assert torch.equal(r["zero_g_contact"], r["step_g_contact"])
    if t.n_contacts:
        assert float(r["zero_g_contact"].abs().max()) > 0
    assert not torch.equal(r["par_g_dof"], r["zero_g_dof"])   # the reward / observation cotangents reach the parameters
    print("%s variant %d waves %d" % (name, eng.variant, eng.waves))


@pytest.mark.parametrize("name,generic,lean", CONFIGS, ids=IDS)
def test_rows_equal_shared_launches_bit_for_bit(name, generic, lean, monkeypatch):
    """per-environment mode: environment e under row e equals an N = 1 shared launch under those values"""
    from diffrl_amd.engine import StepParameters
    t, spec, scale, dt, c = _case(name)
    eng = _engine(t, monkeypatch, generic, lean, **_user(name))
    p = eng.env_step_parameters(N)
    f = torch.tensor(FACTORS, device=DEV)
    for k in p.FIELDS:
        x = getattr(p, k)
        x.mul_(f.view(N, *([1] * (x.dim() - 1))))
    p.contact_material[:, :, 3] *= f.flip(0).view(N, 1) ** 2   # (mu ordered differently from ke: not one friction branch for all)
    eng.set_env_params(p)
    got = _launches(eng, t, spec, scale, dt, c)
    eng2 = _engine(t, monkeypatch, generic, lean, **_user(name))
    for e in range(N):
        eng2.set_params(StepParameters(**{k: getattr(p, k)[e].clone().contiguous() for k in p.FIELDS}))
        one = _launches(eng2, t, spec, scale, dt, c, n=1, rows=slice(e, e + 1))
        for k in got:
            assert torch.equal(got[k][e], one[k][0]), "%s of environment %d differs from the shared launch under its row" % (k, e)
    assert not torch.equal(got["par_g_dof"][0], got["par_g_dof"][1])
    # more environments than rows: refused
    from diffrl_amd import capi
    ck = torch.zeros(N + 1, int(eng._lib.dsim_ckpt_floats_mm(eng._h, S, MM)), device=DEV)
    with pytest.raises(capi.DsimError, match=r"n_envs = 4\b.*\b3 environments"):
        _raw_backward_params(eng, spec, ck, torch.zeros((N + 1) * spec.n_act, device=DEV), dt, [None] * 5)
    eng.reset_params()


def test_sanitize_scrubs_the_parameter_outputs(monkeypatch):
    """the exploded states of humanoid_exploded.npz without an episode block (nothing flags them invalid): non-finite parameter
    words with sanitize_grads = 0, none with 1, and every word that was finite is returned unchanged"""
    t, spec, scale, dt, _ = _case("humanoid")
    x = E.golden("humanoid_exploded")
    n = x["q0"].shape[0]
    eng = _engine(t, monkeypatch)
    a = _T(x["actions"][0]).reshape(-1)
    ck = eng.env_forward(spec, _T(x["q0"]).reshape(-1), _T(x["qd0"]).reshape(-1), a, dt, S, MM, True)[4]
    rs = np.random.RandomState(9)
    cots = [_T(rs.normal(size=s).astype(np.float32)).reshape(-1) for s in ((n, t.n_q), (n, t.n_qd), (n, spec.n_obs), (n,))] + [None]
    out = {}
    for on in (0, 1):
        spec.sanitize_grads = on
        out[on] = _raw_backward_params(eng, spec, ck, a, dt, cots)
    torch.cuda.synchronize()
    spec.sanitize_grads = 0
    raw, clean = out[0], out[1]
    for k in ("g_dof", "g_contact", "gq", "gqd"):
        bad = ~torch.isfinite(raw[k])
        assert bool(torch.isfinite(clean[k]).all()), k
        assert torch.equal(clean[k][~bad], raw[k][~bad]) and not bool(clean[k][bad].any()), k
    assert bool(torch.isfinite(clean["ga"]).all())
    assert bool((~torch.isfinite(raw["g_dof"])).any()) and bool((~torch.isfinite(raw["g_contact"])).any())
    assert bool(torch.isfinite(raw["g_dof"][[0, 2]]).all()) and float(clean["g_dof"][[0, 2]].abs().max()) > 0
    try:
        eng.status()   # (an exploded state may have left the unit sphere: the mark belongs to this test's inputs)
    except Exception:
        pass


FIXTURES = [c for c in CONFIGS if c[0] != "user_tree"]


@pytest.mark.parametrize("name,generic,lean", FIXTURES, ids=IDS[:len(FIXTURES)])
def test_recorded_rollout_matches_the_reference(name, generic, lean, monkeypatch):
    from diffrl_amd.engine import EpisodeIO
    t, spec, scale, dt, _ = _case(name)
    g = E.golden(name + "_envpar")
    eng = _engine(t, monkeypatch, generic, lean)
    host = lambda x: x.detach().cpu().numpy()  # noqa: E731

    def forward(q, qd, a, ep):
        n = q.shape[0]
        prog, cnt = _T(ep.progress, torch.int64), _T(ep.reset_count, torch.int32)
        io = EpisodeIO(prog, _T(ep.reset_q), _T(ep.reset_qd), cnt, ep.episode_length, ep.height_terminate, ep.check_invalid,
                       want_obs_before=True)
        qo, qdo, obs, rew, ck, ob, done = eng.env_forward(spec, _T(q).reshape(-1), _T(qd).reshape(-1), _T(a).reshape(-1), dt, S, MM,
                                                          True, io)
        torch.cuda.synchronize()
        ep.progress[:], ep.reset_count[:], ep.done[:], ep.obs_before[:] = host(prog), host(cnt), host(done), host(ob)
        return host(qo).reshape(n, -1), host(qdo).reshape(n, -1), host(obs), host(rew), ck

    def backward(ck, a, *cots):
        n = ck.shape[0]
        r = _raw_backward_params(eng, spec, ck, _T(a).reshape(-1), dt, [_T(x).reshape(-1) if x is not None else None for x in cots])
        torch.cuda.synchronize()
        return {k: host(v).reshape(n, *v.shape[1:]) for k, v in r.items()}

    rec, ga, g_dof, g_con = E.rollout(name, t, g, spec, forward, backward)
    eng.status()
    E.check_recording(name, t, g, rec, ga, g_dof, g_con)


def _ant(n, early_termination=False):
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=MM,
                    early_termination=early_termination)
    e.sim_substeps, e.sim_dt = S, float(E.golden("ant_envpar")["dt"])   # (the step of the recordings: four of its own substeps)
    e.reset()
    g = E.golden("ant_envpar")
    with torch.no_grad():
        e.state.joint_q, e.state.joint_qd = _T(g["q0"][-n:]).reshape(-1), _T(g["qd0"][-n:]).reshape(-1)
    return e, _T(g["actions"][:2, -n:])


def _leaves(p):
    for k in p.FIELDS:
        setattr(p, k, getattr(p, k).clone().requires_grad_(True))
    return p


def _two_steps(e, acts, w):
    loss = 0.0
    for h in range(2):
        obs, rew, done, info = e.step(acts[h])
        loss = loss - rew.sum() + (w * info["obs_before_reset"]).sum()
    return loss + (w * obs).sum()


@pytest.mark.parametrize("per_env", [False, True], ids=["shared", "per-env"])
def test_env_step_twice_then_backward_equals_the_folded_raw_launches(per_env, monkeypatch):
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    e, acts = _ant(N)
    eng, spec = e.model.engine(), e._spec()
    p = _leaves(eng.env_step_parameters(N) if per_env else eng.step_parameters())
    assert e.set_step_parameters(p) is p and e.step_params is p and eng.env_params() == (N if per_env else 0)
    w = 0.01 * torch.randn(N, e.num_obs, generator=torch.Generator().manual_seed(2)).to(DEV)
    q0, qd0 = e.state.joint_q.clone(), e.state.joint_qd.clone()
    a = acts.clone().requires_grad_(True)
    _two_steps(e, a, w).backward()
    torch.cuda.synchronize()
    # the raw launches: two fused forwards with the environment's episode block, then the reverse chain
    from diffrl_amd.engine import EpisodeIO
    dt = float(e.sim_dt)
    io = lambda: EpisodeIO(prog, e._pool[0], e._pool[1], cnt, e.episode_length, e.height_terminate, e.check_invalid, True)  # noqa: E731
    prog, cnt = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    f0 = eng.env_forward(spec, q0, qd0, acts[0].reshape(-1).contiguous(), dt, S, MM, True, io())
    f1 = eng.env_forward(spec, f0[0], f0[1], acts[1].reshape(-1).contiguous(), dt, S, MM, True, io())
    grew = -torch.ones(N, device=DEV)
    b1 = eng.env_backward_params(spec, f1[4], acts[1].reshape(-1).contiguous(), dt, S, MM, None, None, w.contiguous(), grew, w.contiguous())
    b0 = eng.env_backward_params(spec, f0[4], acts[0].reshape(-1).contiguous(), dt, S, MM, b1[0], b1[1], None, grew, w.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a.grad[0], b0[2]) and torch.equal(a.grad[1], b1[2])
    folds = [eng.fold_param_grads(b[3], b[4], per_env=per_env) for b in (b1, b0)]   # (autograd's order: the last step first)
    for k, x1, x0 in zip(p.FIELDS, *folds):
        got = getattr(p, k).grad
        assert got is not None and got.shape == getattr(p, k).shape, k
        assert torch.equal(got, (x1.view(got.shape) + x0.view(got.shape))), k
    assert float(p.contact_material.grad.abs().max()) > 0 and float(p.joint_target_kd.grad.abs().max()) > 0
    e.set_step_parameters(None)
    assert e.step_params is None and eng.env_params() == 0
    eng.status()


def test_equal_rows_sum_to_the_shared_gradient(monkeypatch):
    """all rows equal: the per-environment gradient summed over the rows is the gradient of the shared tensor, up to the fp32
    re-association of N terms per entry and step -- 1e-5 relative in each tensor's max-norm"""
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    grads = {}
    for per_env in (True, False):
        e, acts = _ant(N)
        eng = e.model.engine()
        p = _leaves(eng.env_step_parameters(N) if per_env else eng.step_parameters())
        e.set_step_parameters(p)
        w = 0.01 * torch.randn(N, e.num_obs, generator=torch.Generator().manual_seed(2)).to(DEV)
        _two_steps(e, acts, w).backward()
        torch.cuda.synchronize()
        grads[per_env] = {k: getattr(p, k).grad.clone() for k in p.FIELDS}
        e.set_step_parameters(None)
    for k, want in grads[False].items():
        got = grads[True][k].sum(0)
        if float(want.abs().max()) == 0:
            assert float(got.abs().max()) == 0, k
            continue
        err = relerr(got.cpu().numpy(), want.cpu().numpy())
        print("%s: sum of the per-environment gradients against the shared gradient %.2e" % (k, err))
        assert err < 1e-5, (k, err)


def test_plain_path_without_a_leaf_and_the_epoch_guard(monkeypatch):
    """no tensor requiring grad: exactly the EnvStep path (no parameter launch); parameters set again between a step and its
    backward: DsimError"""
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    from diffrl_amd import capi
    e, acts = _ant(N)
    eng = e.model.engine()
    seen = []
    keep = eng.env_backward_params
    eng.env_backward_params = lambda *a, **k: (seen.append(1), keep(*a, **k))[1]
    p = eng.step_parameters()
    e.set_step_parameters(p)
    a = acts.clone().requires_grad_(True)
    obs, rew, _, _ = e.step(a[0])
    rew.sum().backward()
    assert not seen and float(a.grad.abs().max()) > 0
    p = _leaves(p)
    e.set_step_parameters(p)
    e.clear_grad()
    obs, rew, _, _ = e.step(a[1])
    e.set_step_parameters(p)   # (an optimiser step would do this): the checkpoint is now stale
    with pytest.raises(capi.DsimError, match="parameter epoch"):
        rew.sum().backward()
    assert not seen
    e.clear_grad()
    obs, rew, _, _ = e.step(a[1])
    rew.sum().backward()
    torch.cuda.synchronize()
    assert seen == [1] and float(p.joint_target_ke.grad.abs().max()) > 0
    e.set_step_parameters(None)
    eng.status()


def test_graphed_rollout_with_parameter_leaves(monkeypatch):
    """a captured two-step rollout whose leaves are parameter tensors equals eager runs, before and after an in-place update"""
    monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    from diffrl_amd.graph import GraphedRollout
    e, acts = _ant(N)
    eng = e.model.engine()
    base = eng.env_step_parameters(N)
    eng.set_env_params(base)   # the first call with a new N allocates: before anything is captured
    w = 0.01 * torch.randn(N, e.num_obs, generator=torch.Generator().manual_seed(2)).to(DEV)
    q0, qd0 = e.state.joint_q.detach().clone(), e.state.joint_qd.detach().clone()
    stat = torch.zeros(1, device=DEV)

    def make_body(p):
        def body(env):
            env.set_step_parameters(p)   # first: a replay sees in-place updates of the leaves
            loss = _two_steps(env, acts, w)
            stat.copy_(loss.detach().view(1))
            return loss
        return body

    def params(cm, tkd):
        from diffrl_amd.engine import EnvStepParameters
        p = EnvStepParameters(**{k: getattr(base, k) for k in base.FIELDS})
        p.contact_material, p.joint_target_kd = cm, tkd
        return p

    def eager(cm_values, tkd_values):
        cm, tkd = cm_values.clone().requires_grad_(True), tkd_values.clone().requires_grad_(True)
        st = e.model.state()
        st.joint_q, st.joint_qd = q0.clone(), qd0.clone()
        e.state = st
        e.progress_buf = torch.zeros_like(e.progress_buf)
        make_body(params(cm, tkd))(e).backward()
        torch.cuda.synchronize()
        return float(stat), cm.grad.clone(), tkd.grad.clone()

    v0 = (base.contact_material.clone(), base.joint_target_kd.clone())
    v1 = (v0[0] * torch.tensor([1.0, 1.0, 0.5, 0.5], device=DEV), v0[1] * 1.5 + 0.25)
    ref0, ref1 = eager(*v0), eager(*v1)
    assert ref0[0] != ref1[0] and np.isfinite(ref0[0]) and float(ref0[1].abs().max()) > 0 and float(ref0[2].abs().max()) > 0
    st = e.model.state()
    st.joint_q, st.joint_qd = q0.clone(), qd0.clone()
    e.state = st
    e.progress_buf = torch.zeros_like(e.progress_buf)
    gc.collect()
    cm, tkd = v0[0].clone().requires_grad_(True), v0[1].clone().requires_grad_(True)
    roll = GraphedRollout(e, make_body(params(cm, tkd)), leaves=[cm, tkd], carry_state=False)
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) == ref0[0] and torch.equal(cm.grad, ref0[1]) and torch.equal(tkd.grad, ref0[2])
    with torch.no_grad():
        cm.copy_(v1[0])
        tkd.copy_(v1[1])
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) == ref1[0] and torch.equal(cm.grad, ref1[1]) and torch.equal(tkd.grad, ref1[2])
    e.set_step_parameters(None)
    eng.status()


def test_the_example_runs_in_both_modes(capsys):
    """examples/sysid_env_lite.py, a few iterations, eager and captured: finite losses that go down, scales that move towards
    the true ones"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sysid_env_lite", os.path.join(ROOT, "examples", "sysid_env_lite.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for flags in ([], ["--graph"]):
        hist = ex.main(["--envs", "16", "--horizon", "4", "--iters", "6"] + flags)
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("loss:")]
        assert len(line) == 1 and ("graph" if flags else "eager") in line[0], line
        assert len(hist) == 6 and all(np.isfinite(v) for row in hist for v in row)
        assert hist[-1][0] < hist[0][0] and hist[-1][1] > 1.0 and hist[-1][2] > 1.0, hist
