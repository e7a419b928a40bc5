"""-m gpu: the differentiable joint dynamics on the real HIP kernels -- dsim_joint_dynamics / dsim_joint_dynamics_backward
through the C ABI, Engine.joint_dynamics under torch.autograd, behind a whole env-step, and inside a captured rollout.

References and bounds are those of tests/test_joint_dynamics_cpu.py and tests/dyn_lib.py (their docstrings have the reasoning):
the reference simulator's recordings (tests/golden/<env>_step.npz, <env>_dyn.npz); forward 1e-4; every cotangent set in its own max-norm, adjoint 10 x the reference's
recorded +-1 ulp noise of that set (floor 1e-5, ceiling 1e-3; pairs noisier than 3e-4 excluded, at most three, all SNUHumanoid gq, and still
finite); joint_q gradients compared after project_tangent, own radial part <= 1e-6 of max |gq|.  The composite case goes through
a whole contact-rich env-step: 10 x its recorded noise with the step's bounds as floors (state 1e-4, gradients 1e-3)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dyn_lib as D
from kin_lib import radial_part
from oracle_lib import golden, project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "tests", "inject", "libdsim_user.so")
DEV = "cuda:0"


def _engine(env, generic, monkeypatch):
    from diffrl_amd.engine import Engine
    if generic:
        monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    t = template_from_golden(env)
    eng = Engine(t, torch.device(DEV))
    assert (eng.variant == 0) == generic
    return t, eng


def _T(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV).reshape(-1) if a is not None else None


def _N(a, n):
    return a.detach().cpu().numpy().reshape(n, -1) if a is not None else None


def _raw_backward(eng, q, qd, act, mact, c):
    n = q.shape[0]
    out = eng.joint_dynamics_backward(_T(q), _T(qd), _T(act), _T(mact), _T(c[0]), _T(c[1]), _T(c[2]))
    torch.cuda.synchronize()
    return tuple(_N(x, n) for x in out)


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", D.ENVS)
def test_forward_vs_the_reference_recordings(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    g = golden(env + "_step")
    q, qd, act, mact, muscles = D.inputs(g)
    B, L = q.shape[0], t.n_links
    tau, qdd, fs = eng.joint_dynamics_forward(_T(q), _T(qd), _T(act), _T(mact))
    assert tau.shape == (B * t.n_qd,) and qdd.shape == (B * t.n_qd,) and fs.shape == (B * L, 6)
    torch.cuda.synchronize()
    eng.status()
    errs = dict(tau=relerr(_N(tau, B), g["sub_tau"]), qdd=relerr(_N(qdd, B), g["sub_qdd"]),
                f_s=relerr(_N(fs, B), g["sub_f_s"].reshape(B, -1)))
    print(env, "generic" if generic else "specialised", "forward", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(e < D.FWD_BOUND for e in errs.values()), errs


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", D.ENVS)
def test_adjoint_vs_the_reference_recordings(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    g, dyn = golden(env + "_step"), golden(env + "_dyn")
    q, qd, act, mact, muscles = D.inputs(g)
    plan, excluded = D.adjoint_plan(env, dyn, muscles)
    label = "generic" if generic else "specialised"
    print(env, label, "excluded ((state, tensor), (sets, largest recorded noise)):", excluded)
    atag = "gmact" if muscles else "gact"
    for tag in D.COTANGENTS:
        gq, gqd, gact, gmact = _raw_backward(eng, q, qd, act, mact, D.cotangents(dyn, tag))
        assert all(np.isfinite(v).all() for v in (gq, gqd, gact)) and (gmact is None or np.isfinite(gmact).all())
        got = dict(gq=project_tangent(t, q, gq), gqd=gqd)
        got[atag] = gmact if muscles else gact
        ref = dict(gq=project_tangent(t, q, dyn["gq_" + tag]), gqd=dyn["gqd_" + tag])
        ref[atag] = dyn[atag + "_" + tag]
        rad = radial_part(t, q, gq)
        for k in got:
            rows, bound, noise = plan[(tag, k)]
            e = D.rows_err(got[k], ref[k], rows)
            print("%s %s cotangent %-3s %-5s err %.2e  reference noise %.2e  bound %.1e" % (env, label, tag, k, e, noise, bound))
            assert e < bound, (tag, k, e, bound)
        assert rad <= D.RADIAL, (tag, rad)
    eng.status()


def test_determinism_and_argument_contract(monkeypatch):
    from diffrl_amd import capi
    t, eng = _engine("humanoid", False, monkeypatch)
    g, dyn = golden("humanoid_step"), golden("humanoid_dyn")
    q, qd, act, _, _ = D.inputs(g)
    B = q.shape[0]
    zeros = (np.zeros_like(dyn["c_tau"]), np.zeros_like(dyn["c_qdd"]), np.zeros_like(dyn["c_fs"]))
    for tag in D.COTANGENTS:
        c = D.cotangents(dyn, tag)
        a = _raw_backward(eng, q, qd, act, None, c)
        b = _raw_backward(eng, q, qd, act, None, tuple(x if x is not None else z for x, z in zip(c, zeros)))
        a2 = _raw_backward(eng, q, qd, act, None, c)
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a[:3], b[:3], a2[:3]))   # NULL == zeros; two launches
    # NULL act is zeros, forward and backward
    f0 = eng.joint_dynamics_forward(_T(q), _T(qd), None, None)
    f1 = eng.joint_dynamics_forward(_T(q), _T(qd), _T(np.zeros_like(act)), None)
    f2 = eng.joint_dynamics_forward(_T(q), _T(qd), _T(act), None)
    assert all(torch.equal(x, y) for x, y in zip(f0, f1)) and not torch.equal(f0[0], f2[0])
    c = D.cotangents(dyn, "all")
    b0 = _raw_backward(eng, q, qd, None, None, c)
    b1 = _raw_backward(eng, q, qd, np.zeros_like(act), None, c)
    assert all(np.array_equal(x, y) for x, y in zip(b0[:3], b1[:3]))
    # NULL outputs are skipped: the others are what the full call writes, and a skipped buffer is not touched
    n, nd, L = B, t.n_qd, t.n_links
    lib, h, P = eng._lib, eng._h, lambda x: x.data_ptr() if x is not None else None   # noqa: E731
    tq, tqd, ta = _T(q), _T(qd), _T(act)
    for skip in range(3):
        outs = [torch.full((n * nd,), 7.0, device=DEV), torch.full((n * nd,), 7.0, device=DEV), torch.full((n * L * 6,), 7.0, device=DEV)]
        ptrs = [P(o) if k != skip else None for k, o in enumerate(outs)]
        eng._ck(lib.dsim_joint_dynamics(h, n, P(tq), P(tqd), P(ta), None, ptrs[0], ptrs[1], ptrs[2], None))
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert torch.equal(o, f2[k].reshape(-1)) if k != skip else bool((o == 7.0).all())
    gq = torch.empty(n * t.n_q, device=DEV)
    gqd = torch.empty(n * nd, device=DEV)
    tc = _T(dyn["c_qdd"])
    eng._ck(lib.dsim_joint_dynamics_backward(h, n, P(tq), P(tqd), P(ta), None, None, P(tc), None, P(gq), P(gqd), None, None, None))
    torch.cuda.synchronize()
    ref = _raw_backward(eng, q, qd, act, None, D.cotangents(dyn, "qdd"))
    assert np.array_equal(_N(gq, n), ref[0]) and np.array_equal(_N(gqd, n), ref[1])        # gact / gmuscle_act NULL: skipped
    with pytest.raises(capi.DsimError):
        eng._ck(lib.dsim_joint_dynamics(h, n, P(tq), P(tqd), P(ta), None, None, None, None, None))   # all three outputs NULL
    eng.status()


def test_non_unit_quaternion_is_reported_by_the_next_call(monkeypatch):
    from diffrl_amd import capi
    t, eng = _engine("ant", False, monkeypatch)
    g, dyn = golden("ant_step"), golden("ant_dyn")
    q, qd, act, _, _ = D.inputs(g)
    bad = q.copy()
    bad[5, 3:7] *= np.float32(1.001)
    eng.joint_dynamics_forward(_T(bad), _T(qd), _T(act), None)       # launches; the kernel marks the model
    torch.cuda.synchronize()
    with pytest.raises(capi.DsimError, match="environment 5"):
        eng.joint_dynamics_forward(_T(q), _T(qd), _T(act), None)     # ... and the next call on the model refuses, once
    tau, _, _ = eng.joint_dynamics_forward(_T(q), _T(qd), _T(act), None)
    torch.cuda.synchronize()
    eng.status()
    assert relerr(_N(tau, q.shape[0]), g["sub_tau"]) < D.FWD_BOUND
    # the adjoint launch does not check again (the forward launch of the same state did)
    eng.joint_dynamics_backward(_T(bad), _T(qd), _T(act), None, None, _T(dyn["c_qdd"]), None)
    torch.cuda.synchronize()
    eng.status()


_USER_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import dyn_lib as D
from kin_lib import radial_part
from diffrl_amd.engine import Engine
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import relerr, project_tangent
from test_edge_cases_cpu import _tree_states
dev = torch.device("cuda:0")
T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev).reshape(-1)
N = lambda a, n: a.cpu().numpy().reshape(n, -1)
h = D.CHECK_H
for tag, path in D.USER_MODELS:
    t = ArticulationTemplate.load(path)
    n = 6
    q, qd, act = _tree_states(t, np.random.default_rng(17), n)
    g = np.random.default_rng(5).normal(size=qd.shape).astype(np.float32)
    for generic in (True, False):
        if generic: os.environ["DSIM_FORCE_GENERIC"] = "1"
        else: os.environ.pop("DSIM_FORCE_GENERIC", None)
        eng = Engine(t, dev)
        assert (eng.variant == 0) == generic, (eng.variant, generic)
        mact = torch.zeros(0, device=dev)
        gq, gqd, gact, _ = eng.joint_dynamics_backward(T(q), T(qd), T(act), None, None, T(g), None)
        qo, qdo, ck = eng.forward(T(q), T(qd), T(act), mact, h, 1, 1, True)
        sq, sqd, sact, _ = eng.backward(ck, T(act), mact, h, 1, 1, torch.zeros_like(T(q)), T(g))
        torch.cuda.synchronize()
        eng.status()
        gq = N(gq, n)
        errs = [relerr(project_tangent(t, q, gq), project_tangent(t, q, N(sq, n) / h)), relerr(N(gact, n), N(sact, n) / h)]
        print("RESULT %%s %%s worst=%%.3e radial=%%.3e  (gq gact: %%s)" %% (
            tag, "generic" if generic else "specialised", max(errs), radial_part(t, q, gq), " ".join("%%.2e" %% e for e in errs)))
'''


def test_user_models_qdd_adjoint_equals_the_step_adjoint_of_one_substep():
    """tests/inject/libdsim_user.so (generic kernels + the sets of the two user models): with one substep of length h, a fresh
    mass matrix, gq_out = 0 and gqd_out = g, dsim_step_backward returns h (d qdd / d q)^T g and h (d qdd / d act)^T g"""
    if not os.path.exists(USER_LIB):
        pytest.fail("tests/inject/libdsim_user.so is missing: __graft_entry__.build() makes it with python -m diffrl_amd.specialise")
    e = dict(os.environ, DSIM_LIB=USER_LIB)
    e.pop("DSIM_FORCE_GENERIC", None)
    r = subprocess.run([sys.executable, "-c", _USER_SCRIPT % dict(root=ROOT)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    res = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    print("\n".join(res))
    assert len(res) == 4, r.stdout
    for l in res:
        assert float(l.split("worst=")[1].split()[0]) < D.CHECK_BOUND and float(l.split("radial=")[1].split()[0]) <= D.RADIAL, l


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", D.ENVS)
def test_shipped_models_qdd_adjoint_equals_the_step_adjoint_of_one_substep(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    g = golden(env + "_step")
    q, qd, act, mact, muscles = D.inputs(g)
    n, h = q.shape[0], D.CHECK_H
    gg = np.random.default_rng(5).normal(size=qd.shape).astype(np.float32)
    m = _T(mact) if muscles else torch.zeros(0, device=DEV)
    gq, gqd, gact, gmact = eng.joint_dynamics_backward(_T(q), _T(qd), _T(act), _T(mact), None, _T(gg), None)
    qo, qdo, ck = eng.forward(_T(q), _T(qd), _T(act), m, h, 1, 1, True)
    sq, sqd, sact, smact = eng.backward(ck, _T(act), m, h, 1, 1, torch.zeros_like(_T(q)), _T(gg))
    torch.cuda.synchronize()
    eng.status()
    errs = dict(gq=relerr(project_tangent(t, q, _N(gq, n)), project_tangent(t, q, _N(sq, n) / h)))
    if muscles:
        errs["gmact"] = relerr(_N(gmact, n), _N(smact, n) / h)
    else:
        errs["gact"] = relerr(_N(gact, n), _N(sact, n) / h)
    print(env, "generic" if generic else "specialised", "vs step adjoint / h:", " ".join("%s %.2e" % kv for kv in errs.items()), "bound %.1e" % D.CHECK_BOUND)
    assert all(e < D.CHECK_BOUND for e in errs.values()), errs


def test_autograd_returns_the_raw_gradients_and_unused_outputs_get_no_cotangent(monkeypatch):
    t, eng = _engine("humanoid", False, monkeypatch)
    g, dyn = golden("humanoid_step"), golden("humanoid_dyn")
    q0, qd0, act0, _, _ = D.inputs(g)
    B = q0.shape[0]
    c = [_T(dyn["c_tau"]), _T(dyn["c_qdd"]), _T(dyn["c_fs"]).view(-1, 6)]
    seen = []
    raw = eng.joint_dynamics_backward
    monkeypatch.setattr(eng, "joint_dynamics_backward", lambda *a: (seen.append([x is not None for x in a[4:]]), raw(*a))[1])
    leaves = lambda: (_T(q0).requires_grad_(True), _T(qd0).requires_grad_(True), _T(act0).requires_grad_(True))   # noqa: E731
    q, qd, act = leaves()
    tau, qdd, fs = eng.joint_dynamics(q, qd, act)
    assert tau.grad_fn is not None and qdd.grad_fn is not None and fs.grad_fn is not None
    assert tau.shape == (B * t.n_qd,) and qdd.shape == (B * t.n_qd,) and fs.shape == (B * t.n_links, 6)
    ((tau * c[0]).sum() + (qdd * c[1]).sum() + (fs * c[2]).sum()).backward()
    gq, gqd, gact, _ = raw(_T(q0), _T(qd0), _T(act0), None, *c)
    assert torch.equal(q.grad, gq) and torch.equal(qd.grad, gqd) and torch.equal(act.grad, gact) and seen[-1] == [True, True, True]
    # one output: the other two arrive as None (no zero-filled buffers are materialised)
    for k, want in ((1, [False, True, False]), (2, [False, False, True]), (0, [True, False, False])):
        q, qd, act = leaves()
        (eng.joint_dynamics(q, qd, act)[k] * c[k]).sum().backward()
        cc = [x if j == k else None for j, x in enumerate(c)]
        gq, gqd, gact, _ = raw(_T(q0), _T(qd0), _T(act0), None, *cc)
        assert seen[-1] == want and torch.equal(q.grad, gq) and torch.equal(qd.grad, gqd) and torch.equal(act.grad, gact)
    # no actuation given: zeros, and no gradient for it; shapes of the caller's tensors are kept
    q2, qd2 = _T(q0).view(B, -1).requires_grad_(True), _T(qd0).view(B, -1).requires_grad_(True)
    eng.joint_dynamics(q2, qd2)[1].pow(2).sum().backward()
    assert q2.grad.shape == q2.shape and qd2.grad.shape == qd2.shape
    a2 = _T(act0).view(B, -1).requires_grad_(True)
    eng.joint_dynamics(_T(q0), _T(qd0), a2)[0].sum().backward()
    assert a2.grad.shape == a2.shape
    torch.cuda.synchronize()


def test_model_surface_after_an_env_step_gives_an_action_gradient():
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=4, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16)
    e.reset()
    a = torch.zeros((4, 8), device=DEV, requires_grad=True)
    act = torch.tanh(a + 0.1)
    e.step(act)
    joint_act = torch.cat([torch.zeros((4, 6), device=DEV), act * e.action_strength], dim=1).reshape(-1)
    tau, qdd, fs = e.model.joint_dynamics(e.state, joint_act=joint_act)
    L, nd = e.model.links_per_articulation, e.model.joint_dof_count // 4
    assert tau.shape == (4 * nd,) and qdd.shape == (4 * nd,) and fs.shape == (4 * L, 6)
    (1e-4 * qdd.pow(2).sum() + 1e-4 * tau.pow(2).sum() + 1e-4 * fs.pow(2).sum()).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(a.grad).all() and a.grad.abs().sum() > 0


@pytest.mark.parametrize("env", D.ENVS)
def test_composite_env_step_then_dynamics_vs_the_reference(env, monkeypatch):
    """SimStep -> Engine.joint_dynamics(q_out, qd_out, act, mact) -> loss on the three tensors -> backward, against the
    reference's recording of the same composite (tools/gen_dynamics_golden.py): the case users run"""
    from diffrl_amd.engine import SimStep
    t, eng = _engine(env, False, monkeypatch)
    g, dyn = golden(env + "_step"), golden(env + "_dyn")
    B = g["q_in"].shape[0]
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    q, qd = _T(g["q_in"]).requires_grad_(True), _T(g["qd_in"]).requires_grad_(True)
    muscles = "muscle_act_in" in g
    if muscles:
        act, mact = _T(np.zeros_like(g["qd_in"])), _T(g["muscle_act_in"]).requires_grad_(True)
    else:
        act, mact = _T(g["act_in"]).requires_grad_(True), None
    qo, qdo = SimStep.apply(eng, dt, S, mm, q, qd, act, mact)
    tau, qdd, fs = eng.joint_dynamics(qo, qdo, act, mact)
    ((tau * _T(dyn["c_tau"])).sum() + (qdd * _T(dyn["c_qdd"])).sum() + (fs * _T(dyn["c_fs"]).view(-1, 6)).sum()).backward()
    torch.cuda.synchronize()
    eng.status()
    atag = "gmact" if muscles else "gact"
    fwd = dict(tau=(relerr(_N(tau, B), dyn["comp_tau"]), D.composite_bound(dyn, "tau", 1e-4)),
               qdd=(relerr(_N(qdd, B), dyn["comp_qdd"]), D.composite_bound(dyn, "qdd", 1e-4)),
               f_s=(relerr(_N(fs, B), dyn["comp_f_s"].reshape(B, -1)), D.composite_bound(dyn, "f_s", 1e-4)))
    grad = dict(gq=(relerr(project_tangent(t, g["q_in"], _N(q.grad, B)), project_tangent(t, g["q_in"], dyn["comp_gq_in"])),
                    D.composite_bound(dyn, "gq", 1e-3)),
                gqd=(relerr(_N(qd.grad, B), dyn["comp_gqd_in"]), D.composite_bound(dyn, "gqd", 1e-3)))
    if muscles:
        grad[atag] = (relerr(_N(mact.grad, B), dyn["comp_gmuscle_act"]), D.composite_bound(dyn, atag, 1e-3))
    else:
        grad[atag] = (relerr(_N(act.grad, B), dyn["comp_gact"]), D.composite_bound(dyn, atag, 1e-3))
    print(env, "composite", " ".join("%s %.2e (bound %.1e)" % ((k,) + v) for k, v in list(fwd.items()) + list(grad.items())))
    assert all(e < b for e, b in fwd.values()), fwd
    assert all(e < b for e, b in grad.values()), grad


def test_graph_replay_of_a_rollout_with_an_acceleration_and_foot_force_loss_is_bit_identical_to_eager():
    """open-loop Ant rollout whose loss adds qdd^2 and a foot link's f_s after every env.step: the captured rollout (forward +
    backward, one submission) replays to the eager loss and action gradient bit for bit"""
    from diffrl_amd import envs
    from diffrl_amd.graph import GraphedRollout
    dev, n, H, foot = torch.device(DEV), 64, 4, 2      # link 2: the lower link of the first leg
    gen = torch.Generator().manual_seed(0)
    actions = torch.tanh(2.0 * torch.rand((H, n, 8), generator=gen) - 1.0).to(dev)
    root = torch.zeros((n, 6), device=dev)

    def make():
        e = envs.AntEnv(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16, early_termination=True,
                        episode_length=1000)
        e.reset()
        return e

    def body_for(a):
        def body(env):
            env.initialize_trajectory()
            L = env.model.links_per_articulation
            total = 0.0
            for a_t in a.unbind(0):
                env.step(a_t)
                ja = torch.cat([root, a_t.clamp(-1.0, 1.0) * env.action_strength], dim=1).reshape(-1)
                _, qdd, fs = env.model.joint_dynamics(env.state, joint_act=ja)
                total = total + 1e-4 * qdd.pow(2).sum() + 1e-4 * fs.view(n, L, 6)[:, foot].pow(2).sum()
            return total / n
        return body

    e1 = make()
    a1 = actions.clone().requires_grad_(True)
    loss1 = body_for(a1)(e1)
    loss1.backward()
    e2 = make()
    a2 = actions.clone().requires_grad_(True)
    roll = GraphedRollout(e2, body_for(a2), leaves=[a2], carry_state=False)
    for _ in range(2):
        loss2 = roll.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(a1.grad).all() and a1.grad.abs().sum() > 0
    assert float(loss2) == float(loss1.detach())
    assert torch.equal(a2.grad, a1.grad)
