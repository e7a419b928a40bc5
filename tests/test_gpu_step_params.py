"""-m gpu: model-parameter gradients of the step on the real HIP kernels -- dsim_model_set_params / dsim_step_backward_params
through the C ABI, SemiImplicitIntegrator.forward(..., params=p) under torch.autograd, inside a captured rollout, and
examples/sysid_lite.py.

References and bounds are those of tests/test_step_params_cpu.py (its docstring has the reasoning): tests/golden/<env>_par.npz, the
reference's own tape replay of three substeps with requires_grad on its model tensors; q_out / qd_out 1e-4, state gradients 1e-3,
every parameter gradient tensor (and every column of shape_materials) in its own max-norm at 10 x its recorded noise, floor 1e-4,
ceiling 1e-3, nothing excluded.  Sizes: the fixtures' own batches, and N = 1."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import par_lib as P
from oracle_lib import project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAN = float("nan")


def _engine(env, generic, monkeypatch, lean=False, template=None):
    from diffrl_amd.engine import Engine
    if generic:
        monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    t = template if template is not None else template_from_golden(env)
    eng = Engine(t, torch.device(DEV), ckpt_mode="lean" if lean else "full")
    assert (eng.variant == 0) == generic
    return t, eng


def _T(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV).reshape(-1) if a is not None else None


def _p(x):
    return x.data_ptr() if x is not None else None


def _inputs(name, rows=slice(None)):
    t, g, (act, mact) = P.case(name)
    return g, _T(g["q_in"][rows]), _T(g["qd_in"][rows]), _T(act[rows]), _T(mact[rows]) if mact is not None else None


def _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out, want=(True, True), want_act=True):
    """dsim_step_backward_params into NaN-filled buffers (what comes back was written); an output not wanted is passed as NULL"""
    import ctypes as C
    n, nd, M, Cn = ck.shape[0], t.n_qd, t.n_muscles, t.n_contacts
    full = lambda *s: torch.full(s, NAN, device=DEV)  # noqa: E731
    gq, gqd = full(n * t.n_q), full(n * nd)
    ga = full(n * nd) if want_act else None
    gm = full(n * M) if (want_act and M) else None
    g_dof = full(n, 5, nd) if want[0] else None
    g_con = full(n, Cn, 4) if want[1] else None
    eng._call(eng._lib.dsim_step_backward_params, eng._h, n, _p(ck), _p(act), _p(mact), C.c_float(step[0]), step[1], step[2],
              _p(gq_out), _p(gqd_out), _p(gq), _p(gqd), _p(ga), _p(gm), _p(g_dof), _p(g_con))
    torch.cuda.synchronize()
    return dict(gq=gq, gqd=gqd, gact=ga, gmact=gm, g_dof=g_dof, g_contact=g_con)


def _np(x, n):
    return x.cpu().numpy().reshape(n, -1)


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", P.ENVS)
def test_against_the_fixture(env, generic, lean, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch, lean)
    g, q, qd, act, mact = _inputs(env)
    B = g["q_in"].shape[0]
    step = (float(g["dt"]), int(g["substeps"]), int(g["mm_freq"]))
    qo, qdo, ck = eng.forward(q, qd, act, mact, *step, True)
    gq_out, gqd_out = _T(g["gq_out"]), _T(g["gqd_out"])
    r = _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out)
    eng.status()
    tang = lambda x: project_tangent(t, g["q_in"], x)  # noqa: E731
    ga_ref, ga = (g["gmuscle_act"], r["gmact"]) if t.n_muscles else (g["gact"], r["gact"])
    e = dict(q=relerr(_np(qo, B), g["q_out"]), qd=relerr(_np(qdo, B), g["qd_out"]), gq=relerr(tang(_np(r["gq"], B)), tang(g["gq_in"])),
             gqd=relerr(_np(r["gqd"], B), g["gqd_in"]), gact=relerr(_np(ga, B), ga_ref))
    label = "%s %s %s" % (env, "generic" if generic else "specialised", "lean" if lean else "full")
    print(label + " " + " ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < P.STATE_BOUND and e["qd"] < P.STATE_BOUND, e
    assert e["gq"] < P.GRAD_BOUND and e["gqd"] < P.GRAD_BOUND and e["gact"] < P.GRAD_BOUND, e
    g_dof, g_con = r["g_dof"].cpu().numpy(), r["g_contact"].cpu().numpy()
    assert np.isfinite(g_dof).all() and np.isfinite(g_con).all()   # written, not accumulated
    f = P.fold(t, env, g_dof, g_con)
    for k in P.PARAM_TENSORS:
        if "noise_" + k in g:
            err, bound = relerr(f[k], g[k]), P.param_bound(g["noise_" + k])
            print("%s %s err %.2e  reference noise %.1e  bound %.1e" % (label, k, err, float(g["noise_" + k]), bound))
            assert err <= bound, (k, err, bound)
        elif k in f:
            assert not np.asarray(g[k]).any() and not f[k].any(), k
    if t.n_contacts:
        for j, col in enumerate(("ke", "kd", "kf", "mu")):
            ej, bj = relerr(f["g_shape_materials"][..., j], g["g_shape_materials"][..., j]), P.param_bound(g["noise_g_shape_materials_cols"][j])
            print("%s shape_materials.%s err %.2e  bound %.1e" % (label, col, ej, bj))
            assert ej <= bj, (col, ej, bj)
    # the state gradients are dsim_step_backward's, bit for bit
    plain = eng.backward(ck, act, mact, *step, gq_out, gqd_out)
    torch.cuda.synchronize()
    assert torch.equal(plain[0], r["gq"]) and torch.equal(plain[1], r["gqd"]) and torch.equal(plain[2], r["gact"])
    assert plain[3] is None or torch.equal(plain[3], r["gmact"])
    # two launches: identical bits
    again = _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out)
    assert all(torch.equal(r[k], again[k]) for k in r if r[k] is not None)
    # NULL patterns: g_dof only, g_contact only, gact / gmuscle_act NULL
    a = _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out, want=(True, False))
    assert torch.equal(a["g_dof"], r["g_dof"]) and torch.equal(a["gq"], r["gq"])
    if t.n_contacts:
        b = _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out, want=(False, True), want_act=False)
        assert torch.equal(b["g_contact"], r["g_contact"]) and torch.equal(b["gqd"], r["gqd"])
    # N = 1: a row of the batch
    g1, q1, qd1, act1, mact1 = _inputs(env, slice(1, 2))
    _, _, ck1 = eng.forward(q1, qd1, act1, mact1, *step, True)
    r1 = _raw_params(eng, t, ck1, act1, mact1, step, _T(g["gq_out"][1:2]), _T(g["gqd_out"][1:2]))
    assert torch.equal(r1["g_dof"][0], r["g_dof"][1]) and torch.equal(r1["g_contact"][0], r["g_contact"][1])
    assert torch.equal(r1["gq"], r["gq"].view(B, -1)[1])
    eng.status()


def test_error_returns(monkeypatch):
    import ctypes as C
    from diffrl_amd import capi
    t, eng = _engine("ant", False, monkeypatch)
    g, q, qd, act, mact = _inputs("ant")
    step = (float(g["dt"]), int(g["substeps"]), int(g["mm_freq"]))
    _, _, ck = eng.forward(q, qd, act, mact, *step, True)
    gq_out, gqd_out = _T(g["gq_out"]), _T(g["gqd_out"])
    with pytest.raises(capi.DsimError, match="both null"):
        _raw_params(eng, t, ck, act, mact, step, gq_out, gqd_out, want=(False, False))
    with pytest.raises(capi.DsimError, match="null pointer"):
        _raw_params(eng, t, ck, act, mact, step, None, gqd_out)
    x = torch.zeros(t.n_links, device=DEV)
    with pytest.raises(capi.DsimError, match="unknown parameter field"):
        eng._call(eng._lib.dsim_model_set_params, eng._h, 6, _p(x))
    with pytest.raises(capi.DsimError, match="null pointer"):
        eng._call(eng._lib.dsim_model_set_params, eng._h, capi.PARAM_TARGET_KE, None)
    with pytest.raises(capi.DsimError, match="elements"):
        eng.set_params([x[:3].contiguous()] + [None] * 5)
    # a model without contacts: setting the contact materials succeeds and does nothing
    _, cart = _engine("cartpole", False, monkeypatch)
    cart._call(cart._lib.dsim_model_set_params, cart._h, capi.PARAM_CONTACT_MATERIAL, _p(x))
    torch.cuda.synchronize()
    eng.status()


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", ("ant", "snu", "cheetah"))
def test_set_params_equals_a_model_created_with_the_values(env, generic, monkeypatch):
    from diffrl_amd.engine import StepParameters
    t, eng = _engine(env, generic, monkeypatch)
    g, q, qd, act, mact = _inputs(env)
    step = (float(g["dt"]), int(g["substeps"]), int(g["mm_freq"]))
    base = eng.forward(q, qd, act, mact, *step, True)
    vals = P.perturbed_params(t)
    p = StepParameters(joint_target_ke=_T(vals["target_ke"]), joint_target_kd=_T(vals["target_kd"]), joint_limit_ke=_T(vals["limit_ke"]),
                       joint_limit_kd=_T(vals["limit_kd"]), joint_target=_T(vals["target"]),
                       contact_material=_T(vals["contact_material"]).view(-1, 4))
    eng.set_params(p)
    a = eng.forward(q, qd, act, mact, *step, True)
    ga = eng.backward_params(a[2], act, mact, *step, _T(g["gq_out"]), _T(g["gqd_out"]))
    _, eng2 = _engine(env, generic, monkeypatch, template=P.with_params(t, vals))
    b = eng2.forward(q, qd, act, mact, *step, True)
    gb = eng2.backward_params(b[2], act, mact, *step, _T(g["gq_out"]), _T(g["gqd_out"]))
    torch.cuda.synchronize()
    # (q_out, qd_out: the checkpoint buffers are uninitialised memory between their rows' padded arrays)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], base[1])   # the values matter
    assert all(torch.equal(x, y) for x, y in zip(ga, gb) if x is not None)
    # the read-outs run under the set values too
    assert all(torch.equal(x, y) for x, y in zip(eng.joint_dynamics_forward(q, qd, act, mact), eng2.joint_dynamics_forward(q, qd, act, mact)))
    eng.reset_params()
    c = eng.forward(q, qd, act, mact, *step, True)
    torch.cuda.synchronize()
    assert torch.equal(c[0], base[0]) and torch.equal(c[1], base[1])
    eng.status()


def _ant(n):
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16, early_termination=False)
    e.reset()
    with torch.no_grad():   # onto the ground: the contact parameters need contacts
        for _ in range(12):
            e.step(torch.zeros((n, e.num_actions), device=DEV))
    return e


def _leaf_params(model, scale=1.0):
    p = model.step_parameters()
    for k in p.FIELDS:
        setattr(p, k, (getattr(p, k) * scale).requires_grad_(True))
    return p


def test_autograd_two_chained_steps_is_the_sum_of_the_single_steps():
    e = _ant(4)
    model, integ, eng = e.model, e.integrator, e.model.engine()
    t = model.template()
    assert np.array_equal(model.contact_shape.cpu().numpy(), np.asarray(P.golden("ant_model")["contact_material"]))
    p = _leaf_params(model, 1.1)
    n, nd = 4, t.n_qd
    q0, qd0 = e.state.joint_q.detach().clone(), e.state.joint_qd.detach().clone()
    gen = torch.Generator().manual_seed(3)
    act = torch.zeros(n, nd)
    act[:, 6:] = (2.0 * torch.rand((n, nd - 6), generator=gen) - 1.0) * 200.0
    act = act.to(DEV).reshape(-1)
    cq, cqd = torch.randn(n * t.n_q, generator=gen).to(DEV), torch.randn(n * nd, generator=gen).to(DEV)
    step = (e.sim_dt, e.sim_substeps, 16)
    s = model.state()
    s.joint_q, s.joint_qd = q0.clone().requires_grad_(True), qd0.clone()
    s.joint_act = act
    s1 = integ.forward(model, s, *step, params=p)
    s1.joint_act = act
    s2 = integ.forward(model, s1, *step, params=p)
    ((s2.joint_q * cq).sum() + (s2.joint_qd * cqd).sum()).backward()
    # by hand: two forward launches that keep their checkpoints, two parameter sweeps, folded and added
    eng.set_params(p)
    a1 = eng.forward(q0, qd0, act, None, *step, True)
    a2 = eng.forward(a1[0], a1[1], act, None, *step, True)
    assert torch.equal(a2[0], s2.joint_q.detach())
    b2 = eng.backward_params(a2[2], act, None, *step, cq, cqd)
    b1 = eng.backward_params(a1[2], act, None, *step, b2[0], b2[1])
    f1, f2 = eng.fold_param_grads(b1[4], b1[5]), eng.fold_param_grads(b2[4], b2[5])
    torch.cuda.synchronize()
    for k, x1, x2 in zip(p.FIELDS, f1, f2):
        got = getattr(p, k).grad
        assert got is not None and got.shape == getattr(p, k).shape and bool(torch.isfinite(got).all()), k
        assert torch.equal(got.reshape(-1), (x1 + x2).reshape(-1)) or torch.equal(got.reshape(-1), (x2 + x1).reshape(-1)), k
    assert torch.equal(s.joint_q.grad, b1[0])
    assert float(p.contact_material.grad[:, 3].abs().max()) > 0 and float(p.joint_limit_kd.grad.abs().max()) > 0
    eng.reset_params()
    eng.status()


def test_graphed_rollout_with_a_parameter_leaf_sees_in_place_updates():
    from diffrl_amd.graph import GraphedRollout
    e = _ant(4)
    model, integ = e.model, e.integrator
    base = model.step_parameters()
    n, nd, H = 4, model.dofs_per_articulation, 2
    acts = torch.zeros((H, n, nd), device=DEV)
    acts[:, :, 6:] = 100.0
    mu = base.contact_material[:, 3].clone().requires_grad_(True)
    stat = torch.zeros(1, device=DEV)

    def body(env):
        p = type(base)(**{k: getattr(base, k) for k in base.FIELDS})
        p.contact_material = torch.cat([base.contact_material[:, :3], mu.view(-1, 1)], dim=1)
        st = env.state
        for h in range(H):
            st.joint_act = acts[h].reshape(-1)
            st = integ.forward(model, st, env.sim_dt, env.sim_substeps, 16, params=p)
        env.state = st
        loss = (st.joint_q.view(n, -1)[:, 0] ** 2).sum() + (st.joint_qd ** 2).sum()
        stat.copy_(loss.detach().view(1))
        return loss

    roll = GraphedRollout(e, body, leaves=[mu], carry_state=False)
    roll.replay()
    torch.cuda.synchronize()
    l0, g0 = float(stat), mu.grad.clone()
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) == l0 and torch.equal(mu.grad, g0)   # the same start state: the same bits
    assert np.isfinite(l0) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    with torch.no_grad():
        mu.mul_(0.5)
    roll.replay()
    torch.cuda.synchronize()
    assert float(stat) != l0 and not torch.equal(mu.grad, g0)
    model.engine().reset_params()


def test_the_example_lowers_its_loss(capsys):
    """examples/sysid_lite.py, a few iterations, eager and captured: finite values, and the final loss below the initial one"""
    spec = importlib.util.spec_from_file_location("sysid_lite", os.path.join(ROOT, "examples", "sysid_lite.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for flags in ([], ["--graph"]):
        hist = ex.main(["--envs", "16", "--horizon", "4", "--iters", "6"] + flags)
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("loss:")]
        assert len(line) == 1 and ("graph" if flags else "eager") in line[0], line
        assert all(np.isfinite(v) for row in hist for v in row)
        assert hist[-1][0] < hist[0][0], (hist[0], hist[-1])
