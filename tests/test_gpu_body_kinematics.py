"""-m gpu: the differentiable body kinematics on the real HIP kernels -- dsim_body_kinematics / dsim_body_kinematics_backward
through the C ABI, Engine.body_kinematics under torch.autograd, behind a whole env-step, and inside a captured rollout.

References and bounds are those of tests/test_body_kinematics_cpu.py (its docstring has the reasoning): the reference
simulator's recordings (tests/golden/<env>_step.npz, <env>_kin.npz), max-norm relative error < 1e-5 for the kinematics and its
adjoint, joint_q gradients compared after project_tangent, own radial part <= 1e-6 of max |gq|.  The composite case goes through
a whole contact-rich env-step and gets that step's bounds (tests/test_gpu_parity.py: state 1e-4, gradients 1e-3)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kin_lib as K
from oracle_lib import golden, project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "tests", "inject", "libdsim_user.so")
BOUND, RADIAL = 1e-5, 1e-6
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


def _T2(a, cols):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV).reshape(-1, cols) if a is not None else None


def _raw_backward(eng, t, q, qd, c):
    n = q.shape[0]
    gq, gqd = eng.body_kinematics_backward(_T(q), _T(qd), _T2(c[0], 7), _T2(c[1], 7), _T2(c[2], 6))
    torch.cuda.synchronize()
    return gq.cpu().numpy().reshape(n, -1), gqd.cpu().numpy().reshape(n, -1) if gqd is not None else None


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", K.ENVS)
def test_forward_and_adjoint_vs_the_reference_recordings(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    g, kin = golden(env + "_step"), golden(env + "_kin")
    q, qd = g["q_in"], g["qd_in"]
    B, L = q.shape[0], t.n_links
    xsc, xsm, vs = eng.body_kinematics_forward(_T(q), _T(qd))
    assert xsc.shape == (B * L, 7) and xsm.shape == (B * L, 7) and vs.shape == (B * L, 6)
    cx, cm, cv = eng.body_kinematics_forward(_T(g["q_out"]), _T(g["qd_out"]))
    px, pm, pv = eng.body_kinematics_forward(_T(q), None)
    torch.cuda.synchronize()
    eng.status()
    N = lambda a, c: a.cpu().numpy().reshape(B, L, c)   # noqa: E731
    errs = dict(X_sc=relerr(N(xsc, 7), g["sub_X_sc"].reshape(B, L, 7)), X_sm=relerr(N(xsm, 7), g["sub_X_sm"].reshape(B, L, 7)),
                v_s=relerr(N(vs, 6), g["sub_v_s"].reshape(B, L, 6)), comp_X_sc=relerr(N(cx, 7), kin["comp_X_sc"]),
                comp_X_sm=relerr(N(cm, 7), kin["comp_X_sm"]), comp_v_s=relerr(N(cv, 6), kin["comp_v_s"]))
    print(env, "generic" if generic else "specialised", "forward", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(e < BOUND for e in errs.values()), errs
    assert pv is None and torch.equal(px, xsc) and torch.equal(pm, xsm)           # no qd: the same poses, no twists
    cot = dict(Xsc=(kin["c_Xsc"], None, None), Xsm=(None, kin["c_Xsm"], None), vs=(None, None, kin["c_vs"]),
               all=(kin["c_Xsc"], kin["c_Xsm"], kin["c_vs"]))
    z7, z6 = np.zeros_like(kin["c_Xsc"]), np.zeros_like(kin["c_vs"])
    for tag, c in cot.items():
        gq, gqd = _raw_backward(eng, t, q, qd, c)
        assert np.isfinite(gq).all() and np.isfinite(gqd).all()
        e_q = relerr(project_tangent(t, q, gq), project_tangent(t, q, kin["gq_" + tag]))
        rad = K.radial_part(t, q, gq)
        if tag in ("Xsc", "Xsm"):
            assert not kin["gqd_" + tag].any() and not gqd.any()      # the poses do not depend on qd: exactly 0 on both sides
            e_qd = 0.0
        else:
            e_qd = relerr(gqd, kin["gqd_" + tag])
        print("%s %s cotangent %-3s: gq %.2e (reference's own +-1 ulp noise %.2e)  gqd %.2e (%.2e)  own radial part %.1e"
              % (env, "generic" if generic else "specialised", tag, e_q, float(kin["sens_gq"]), e_qd, float(kin["sens_gqd"]), rad))
        assert e_q < BOUND and e_qd < BOUND, (tag, e_q, e_qd)
        assert rad <= RADIAL, (tag, rad)
        # a NULL cotangent is a zero cotangent; the launch is deterministic
        full = tuple(x if x is not None else z for x, z in zip(c, (z7, z7, z6)))
        gq2, gqd2 = _raw_backward(eng, t, q, qd, full)
        assert np.array_equal(gq, gq2) and np.array_equal(gqd, gqd2)
    gq, gqd = _raw_backward(eng, t, q, None, (kin["c_Xsc"], kin["c_Xsm"], None))
    ref = _raw_backward(eng, t, q, qd, (kin["c_Xsc"], kin["c_Xsm"], None))
    assert gqd is None and np.array_equal(gq, ref[0])                                # no qd: the pose part


_USER_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import kin_lib as K
from diffrl_amd.engine import Engine
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import relerr
from test_edge_cases_cpu import _tree_states
dev = torch.device("cuda:0")
T = lambda a, c=None: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev).reshape(-1) if c is None else torch.tensor(np.ascontiguousarray(a, np.float32), device=dev).reshape(-1, c)
for tag, path in K.USER_MODELS:
    t = ArticulationTemplate.load(path)
    rng = np.random.default_rng(17)
    n, L = 6, t.n_links
    q, qd, _ = _tree_states(t, rng, n)
    c = [rng.normal(size=(n, L, 7)).astype(np.float32), rng.normal(size=(n, L, 7)).astype(np.float32), rng.normal(size=(n, L, 6)).astype(np.float32)]
    r = K.fk_batch(t, q, qd)
    rq, rqd = K.fk_adjoint_batch(t, q, qd, *c)
    for generic in (True, False):
        if generic: os.environ["DSIM_FORCE_GENERIC"] = "1"
        else: os.environ.pop("DSIM_FORCE_GENERIC", None)
        eng = Engine(t, dev)
        assert (eng.variant == 0) == generic, (eng.variant, generic)
        xsc, xsm, vs = eng.body_kinematics_forward(T(q), T(qd))
        gq, gqd = eng.body_kinematics_backward(T(q), T(qd), T(c[0], 7), T(c[1], 7), T(c[2], 6))
        torch.cuda.synchronize()
        eng.status()
        gq = gq.cpu().numpy().reshape(n, -1)
        errs = [relerr(xsc.cpu().numpy().reshape(n, L, 7), r[0]), relerr(xsm.cpu().numpy().reshape(n, L, 7), r[1]),
                relerr(vs.cpu().numpy().reshape(n, L, 6), r[2]), relerr(gq, rq), relerr(gqd.cpu().numpy().reshape(n, -1), rqd)]
        print("RESULT %%s %%s worst=%%.3e radial=%%.3e  (X_sc X_sm v_s gq gqd: %%s)" %% (
            tag, "generic" if generic else "specialised", max(errs), K.radial_part(t, q, gq), " ".join("%%.2e" %% e for e in errs)))
'''


def test_user_models_generic_and_specialised_match_the_float64_statement():
    """tests/inject/libdsim_user.so (generic kernels + the sets of the two user models): free, hinge, prismatic and ball joints,
    CSR-list subtrees (user_tree) and a 17-link row tree (user_rowtree), against the float64 statement of tests/kin_lib.py"""
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
        assert float(l.split("worst=")[1].split()[0]) < BOUND and float(l.split("radial=")[1].split()[0]) <= RADIAL, l


def test_autograd_returns_the_raw_gradients_and_unused_outputs_get_no_cotangent(monkeypatch):
    t, eng = _engine("humanoid", False, monkeypatch)
    g, kin = golden("humanoid_step"), golden("humanoid_kin")
    q0, qd0 = g["q_in"], g["qd_in"]
    B, L = q0.shape[0], t.n_links
    c = [_T2(kin[k], cols) for k, cols in (("c_Xsc", 7), ("c_Xsm", 7), ("c_vs", 6))]
    seen = []
    raw = eng.body_kinematics_backward
    monkeypatch.setattr(eng, "body_kinematics_backward", lambda *a: (seen.append([x is not None for x in a[2:]]), raw(*a))[1])
    # all three outputs
    q, qd = _T(q0).requires_grad_(True), _T(qd0).requires_grad_(True)
    xsc, xsm, vs = eng.body_kinematics(q, qd)
    assert xsc.grad_fn is not None and xsm.grad_fn is not None and vs.grad_fn is not None
    ((xsc * c[0]).sum() + (xsm * c[1]).sum() + (vs * c[2]).sum()).backward()
    gq, gqd = raw(_T(q0), _T(qd0), *c)
    assert torch.equal(q.grad, gq) and torch.equal(qd.grad, gqd) and seen[-1] == [True, True, True]
    # one output: the other two arrive as None (no zero-filled buffers are materialised)
    q, qd = _T(q0).requires_grad_(True), _T(qd0).requires_grad_(True)
    xsc, xsm, vs = eng.body_kinematics(q, qd)
    (xsc * c[0]).sum().backward()
    gq, gqd = raw(_T(q0), _T(qd0), c[0], None, None)
    assert seen[-1] == [True, False, False] and torch.equal(q.grad, gq) and torch.equal(qd.grad, gqd)
    q, qd = _T(q0).requires_grad_(True), _T(qd0).requires_grad_(True)
    (eng.body_kinematics(q, qd)[2] * c[2]).sum().backward()
    gq, gqd = raw(_T(q0), _T(qd0), None, None, c[2])
    assert seen[-1] == [False, False, True] and torch.equal(q.grad, gq) and torch.equal(qd.grad, gqd)
    # poses only
    q = _T(q0).requires_grad_(True)
    xsc, xsm, vs = eng.body_kinematics(q)
    assert vs is None
    (xsm * c[1]).sum().backward()
    assert seen[-1] == [False, True, False] and torch.equal(q.grad, raw(_T(q0), None, None, c[1], None)[0])
    # the detached read-back keeps its behaviour; shapes of the caller's tensors are kept
    assert eng.body_transforms(_T(q0))[0].grad_fn is None
    q2 = _T(q0).view(B, -1).requires_grad_(True)
    eng.body_kinematics(q2)[0].sum().backward()
    assert q2.grad.shape == q2.shape
    torch.cuda.synchronize()


def test_model_surface_and_state_tensors_keep_their_contract():
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=4, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16)
    e.reset()
    a = torch.zeros((4, 8), device=DEV, requires_grad=True)
    e.step(torch.tanh(a + 0.1))
    xsc, xsm, vs = e.model.body_kinematics(e.state)
    L = e.model.links_per_articulation
    assert xsc.shape == (4 * L, 7) and xsm.shape == (4 * L, 7) and vs.shape == (4 * L, 6)
    assert e.state.body_X_sc.grad_fn is None and e.state.body_X_sm.grad_fn is None      # unchanged: the read-back
    (xsc[:, :3].pow(2).sum() + vs.pow(2).sum()).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(a.grad).all() and a.grad.abs().sum() > 0


@pytest.mark.parametrize("env", K.ENVS)
def test_composite_env_step_then_kinematics_vs_the_reference(env, monkeypatch):
    """SimStep -> Engine.body_kinematics(q_out, qd_out) -> loss on the three tensors -> backward, against the reference's
    recording of the same composite (tools/gen_kinematics_golden.py): the case users care about"""
    from diffrl_amd.engine import SimStep
    t, eng = _engine(env, False, monkeypatch)
    g, kin = golden(env + "_step"), golden(env + "_kin")
    B, L = g["q_in"].shape[0], t.n_links
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    q, qd = _T(g["q_in"]).requires_grad_(True), _T(g["qd_in"]).requires_grad_(True)
    muscles = "muscle_act_in" in g
    if muscles:
        act, mact = _T(np.zeros_like(g["qd_in"])), _T(g["muscle_act_in"]).requires_grad_(True)
    else:
        act, mact = _T(g["act_in"]).requires_grad_(True), None
    qo, qdo = SimStep.apply(eng, dt, S, mm, q, qd, act, mact)
    xsc, xsm, vs = eng.body_kinematics(qo, qdo)
    ((xsc * _T2(kin["c_Xsc"], 7)).sum() + (xsm * _T2(kin["c_Xsm"], 7)).sum() + (vs * _T2(kin["c_vs"], 6)).sum()).backward()
    torch.cuda.synchronize()
    N = lambda a: a.detach().cpu().numpy().reshape(B, -1)   # noqa: E731
    fwd = dict(X_sc=relerr(N(xsc), kin["comp_X_sc"].reshape(B, -1)), X_sm=relerr(N(xsm), kin["comp_X_sm"].reshape(B, -1)),
               v_s=relerr(N(vs), kin["comp_v_s"].reshape(B, -1)))
    grad = dict(gq_in=relerr(project_tangent(t, g["q_in"], N(q.grad)), project_tangent(t, g["q_in"], kin["comp_gq_in"])),
                gqd_in=relerr(N(qd.grad), kin["comp_gqd_in"]))
    if muscles:
        grad["gmuscle_act"] = relerr(N(mact.grad), kin["comp_gmuscle_act"])
    else:
        grad["gact"] = relerr(N(act.grad), kin["comp_gact"])
    print(env, "composite", " ".join("%s %.2e" % kv for kv in list(fwd.items()) + list(grad.items())))
    assert all(e < 1e-4 for e in fwd.values()), fwd
    assert all(e < 1e-3 for e in grad.values()), grad


def _ant(n, **kw):
    from diffrl_amd import envs
    args = dict(num_envs=n, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16, early_termination=True,
                episode_length=1000)
    args.update(kw)
    return envs.AntEnv(**args)


def test_graph_replay_of_a_rollout_with_a_link_frame_loss_is_bit_identical_to_eager():
    """open-loop Ant rollout whose loss reads a foot's position and point velocity from body_kinematics after every env.step:
    the captured rollout (forward + backward, one submission) replays to the eager loss and action gradient bit for bit"""
    from diffrl_amd.graph import GraphedRollout
    dev, n, H, foot = torch.device(DEV), 64, 8, 2      # link 2: the lower link of the first leg
    gen = torch.Generator().manual_seed(0)
    actions = torch.tanh(2.0 * torch.rand((H, n, 8), generator=gen) - 1.0).to(dev)
    target = torch.tensor([0.5, 0.3, 0.4], device=dev)

    def body_for(a):
        def body(env):
            env.initialize_trajectory()
            L = env.model.links_per_articulation
            total = 0.0
            for a_t in a.unbind(0):
                env.step(a_t)
                xsc, _, vs = env.model.body_kinematics(env.state)
                p = xsc.view(n, L, 7)[:, foot, :3]
                tw = vs.view(n, L, 6)[:, foot]
                vp = tw[:, 3:] + torch.linalg.cross(tw[:, :3], p)      # velocity of the link frame's origin
                total = total + (p - target).pow(2).sum() + 1e-2 * vp.pow(2).sum()
            return total / n
        return body

    e1 = _ant(n)
    e1.reset()
    a1 = actions.clone().requires_grad_(True)
    loss1 = body_for(a1)(e1)
    loss1.backward()
    e2 = _ant(n)
    e2.reset()
    a2 = actions.clone().requires_grad_(True)
    roll = GraphedRollout(e2, body_for(a2), leaves=[a2], carry_state=False)
    for _ in range(2):
        loss2 = roll.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(a1.grad).all() and a1.grad.abs().sum() > 0
    assert float(loss2) == float(loss1.detach())
    assert torch.equal(a2.grad, a1.grad)


def test_non_unit_quaternion_is_reported_by_the_next_call(monkeypatch):
    from diffrl_amd import capi
    t, eng = _engine("ant", False, monkeypatch)
    g = golden("ant_step")
    bad = g["q_in"].copy()
    bad[5, 3:7] *= np.float32(1.001)
    eng.body_kinematics_forward(_T(bad), _T(g["qd_in"]))       # launches; the kernel marks the model
    torch.cuda.synchronize()
    with pytest.raises(capi.DsimError, match="environment 5"):
        eng.body_kinematics_forward(_T(g["q_in"]), _T(g["qd_in"]))   # ... and the next call on the model refuses, once
    xsc, _, _ = eng.body_kinematics_forward(_T(g["q_in"]), _T(g["qd_in"]))
    torch.cuda.synchronize()
    eng.status()
    assert relerr(xsc.cpu().numpy().reshape(g["sub_X_sc"].shape), g["sub_X_sc"]) < BOUND
    # the adjoint launch does not check again (the forward launch of the same state did)
    eng.body_kinematics_backward(_T(bad), _T(g["qd_in"]), _T2(golden("ant_kin")["c_Xsc"], 7), None, None)
    torch.cuda.synchronize()
    eng.status()
    # argument contract: v_s / gqd if and only if qd
    with pytest.raises(capi.DsimError):
        eng._ck(eng._lib.dsim_body_kinematics(eng._h, 1, None, None, None, None, None, None))


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", K.ENVS)
def test_body_transforms_is_the_kinematic_read_out_without_qd(env, generic, monkeypatch):
    """dsim_body_transforms launches the kernel of dsim_body_kinematics (no qd, no v_s, no status words): the same bits as the
    kinematic read-out, with or without qd.  Three environments: an odd count, one wave each (SNUHumanoid: four)."""
    t, eng = _engine(env, generic, monkeypatch)
    g = golden(env + "_step")
    q, qd = _T(g["q_in"][:3]), _T(g["qd_in"][:3])
    xf = eng.body_transforms(q)
    poses = eng.body_kinematics_forward(q, None)
    full = eng.body_kinematics_forward(q, qd)
    torch.cuda.synchronize()
    eng.status()
    assert xf[0].shape == (3 * t.n_links, 7) and torch.isfinite(xf[0]).all() and torch.isfinite(xf[1]).all()
    assert torch.equal(xf[0], poses[0]) and torch.equal(xf[1], poses[1])
    assert torch.equal(xf[0], full[0]) and torch.equal(xf[1], full[1])


def test_body_transforms_has_no_precondition_and_the_kinematic_read_out_keeps_its_own(monkeypatch):
    """a read-back of whatever the caller holds: a non-unit root quaternion is not reported by dsim_body_transforms, and is
    reported, with its environment, by dsim_body_kinematics on the same kernel"""
    from diffrl_amd import capi
    t, eng = _engine("ant", False, monkeypatch)
    bad = golden("ant_step")["q_in"][:2].copy()
    bad[1, 3:7] *= np.float32(1.01)
    eng.body_transforms(_T(bad))
    torch.cuda.synchronize()
    eng.status()
    eng.body_kinematics_forward(_T(bad), None)
    torch.cuda.synchronize()
    with pytest.raises(capi.DsimError, match="environment 1"):
        eng.status()
