"""-m gpu: the differentiable mass matrix read-out on the real HIP kernels -- dsim_mass_matrix / dsim_mass_matrix_backward through
the C ABI, Engine.mass_matrix under torch.autograd, behind a step, and inside a captured graph.

References and bounds are those of tests/test_mass_matrix_cpu.py (its docstring has the reasoning): sub_H + diag(armature) and
sub_S_s of the step fixtures at 1e-5, |H - H^T| <= 1e-6 max |H|; the inverse by its residual against 10 x the residual of the
float32 restatement of tests/mass_lib.py, floor 1e-6; the gradients of tests/golden/<env>_mass.npz, every cotangent set in its own
max-norm after project_tangent, 10 x the reference's recorded noise of the set, floor 1e-4, ceiling 1e-3, nothing excluded.
Sizes: the fixtures' own batches, and N = 1 and N = 3."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dyn_lib
import mass_lib as M
from kin_lib import radial_part
from oracle_lib import golden, project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "tests", "inject", "libdsim_user.so")
DEV = "cuda:0"
NAN = float("nan")


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


def _p(x):
    return x.data_ptr() if x is not None else None


def _raw_forward(eng, t, q, want=(True, True, True), fill=NAN):
    """dsim_mass_matrix into prefilled buffers (NaN: what comes back was written); an output not wanted is passed as NULL and its
    buffer returned as it was"""
    n, nd = q.shape[0], t.n_qd
    outs = [torch.full((n * nd * nd,), fill, device=DEV), torch.full((n * nd * nd,), fill, device=DEV), torch.full((n * nd * 6,), fill, device=DEV)]
    tq = _T(q)
    eng._call(eng._lib.dsim_mass_matrix, eng._h, n, tq.data_ptr(), *[_p(o) if w else None for o, w in zip(outs, want)])
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy().reshape(s) for o, s in zip(outs, ((n, nd, nd), (n, nd, nd), (n, nd, 6))))


def _raw_backward(eng, t, q, c):
    n = q.shape[0]
    gq = torch.full((n * t.n_q,), NAN, device=DEV)
    cs, tq = [_T(x) for x in c], _T(q)
    eng._call(eng._lib.dsim_mass_matrix_backward, eng._h, n, tq.data_ptr(), *[_p(x) for x in cs], gq.data_ptr())
    torch.cuda.synchronize()
    return gq.cpu().numpy().reshape(n, -1)


def _label(generic):
    return "generic" if generic else "specialised"


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", M.ENVS)
def test_forward_vs_the_reference(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    step = golden(env + "_step")
    q = step["q_in"]
    H, Hinv, S = out = _raw_forward(eng, t, q)
    eng.status()
    assert all(np.isfinite(o).all() for o in out)   # written, not accumulated
    eS, eH = relerr(S, M.reference_S(t, step)), relerr(H, M.reference_H(t, step))
    sym = float(np.abs(H - H.transpose(0, 2, 1)).max() / np.abs(H).max())
    bound, yard = M.residual_bound(M.reference_H(t, step))
    r = M.residual(Hinv, H)
    print("%s %s forward S %.2e H %.2e (bound %.0e)  |H - H^T| %.2e  residual %.2e restatement %.2e bound %.1e"
          % (env, _label(generic), eS, eH, M.FWD_BOUND, sym, r, yard, bound))
    assert eS < M.FWD_BOUND and eH < M.FWD_BOUND, (eS, eH)
    assert sym <= M.SYM_BOUND, sym
    assert r <= bound, (r, bound)
    again = _raw_forward(eng, t, q)
    assert all(np.array_equal(a, b) for a, b in zip(out, again))   # two launches: bit-identical
    for rows in (slice(1, 2), slice(2, 5)):   # N = 1 and N = 3: the rows of the batch
        assert all(np.array_equal(a, b[rows]) for a, b in zip(_raw_forward(eng, t, q[rows]), out))
    eng.status()


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", M.ENVS)
def test_consistent_with_the_shipped_readouts(env, generic, monkeypatch):
    """qdd of the dynamic read-out is Hinv tau, v_s of the kinematic read-out is the masked sum of S_d qd_d"""
    t, eng = _engine(env, generic, monkeypatch)
    step = golden(env + "_step")
    q, qd, act, mact, _ = dyn_lib.inputs(step)
    B = q.shape[0]
    _, Hinv, S = _raw_forward(eng, t, q)
    tau, qdd, _ = eng.joint_dynamics_forward(_T(q), _T(qd), _T(act), _T(mact))
    vs = eng.body_kinematics_forward(_T(q), _T(qd))[2]
    torch.cuda.synchronize()
    eng.status()
    tau, qdd, vs = tau.cpu().numpy().reshape(B, -1), qdd.cpu().numpy().reshape(B, -1), vs.cpu().numpy().reshape(B, -1, 6)
    ref = np.einsum("bij,bj->bi", Hinv.astype(np.float64), tau.astype(np.float64))
    assert (np.abs(qdd - ref) <= M.dot_bound(Hinv, tau)).all(), float(np.abs(qdd - ref).max())
    ref = np.einsum("id,bdk,bd->bik", M.link_dof_mask(t).astype(np.float64), S.astype(np.float64), qd.astype(np.float64))
    e = float(np.abs(vs - ref).max() / np.abs(vs).max())
    print("%s %s v_s against mask S qd %.2e" % (env, _label(generic), e))
    assert e < 1e-5, e


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", M.ENVS)
def test_adjoint_vs_the_fixture(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    step, m = golden(env + "_step"), golden(env + "_mass")
    q = step["q_in"]
    zeros = M.cotangents(dict(c_H=np.zeros_like(m["c_H"]), c_Hinv=np.zeros_like(m["c_Hinv"]), c_S=np.zeros_like(m["c_S"])), "all")
    for tag in M.SETS:
        c = M.cotangents(m, tag)
        gq = _raw_backward(eng, t, q, c)
        assert np.isfinite(gq).all()   # written, not accumulated
        noise = m["noise_gq_" + tag]
        e, bound = relerr(project_tangent(t, q, gq), project_tangent(t, q, m["gq_" + tag])), M.grad_bound(noise)
        print("%s %s cotangent %-4s err %.2e  reference noise %.2e  bound %.1e" % (env, _label(generic), tag, e, noise.max(), bound))
        assert e < bound, (tag, e, bound)
        assert radial_part(t, q, gq) <= M.RADIAL, tag
        # a NULL cotangent is a zero cotangent; two launches are bit-identical
        a = _raw_backward(eng, t, q, tuple(x if x is not None else z for x, z in zip(c, zeros)))
        assert np.array_equal(gq, a) and np.array_equal(gq, _raw_backward(eng, t, q, c)), tag
    for rows in (slice(1, 2), slice(2, 5)):   # N = 1 and N = 3: the rows of the batch (gq: of the set `all`)
        assert np.array_equal(_raw_backward(eng, t, q[rows], M.cotangents(m, "all", rows)), gq[rows])
    assert not _raw_backward(eng, t, q, (None, None, None)).any()   # all cotangents NULL: zeros are written
    eng.status()


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", ("cartpole", "hopper"))
def test_adjoint_equals_central_differences_on_the_hinges(env, generic, monkeypatch):
    """of the kernels' own float32 forward, step 1e-2, the loss summed in float64: to 1e-3 of the largest hinge gradient"""
    t, eng = _engine(env, generic, monkeypatch)
    step, m = golden(env + "_step"), golden(env + "_mass")
    q, cs = step["q_in"], M.cotangents(m, "all")
    coords = [int(t.joint_q_start[i]) for i in range(t.n_links) if int(t.joint_type[i]) in (0, 1)]
    loss = lambda qv: sum((o.astype(np.float64) * c).reshape(len(qv), -1).sum(axis=1) for o, c in zip(_raw_forward(eng, t, qv), cs))  # noqa: E731
    gq = _raw_backward(eng, t, q, cs).astype(np.float64)
    fd = np.zeros((len(q), len(coords)))
    for n, k in enumerate(coords):
        qp, qm = q.copy(), q.copy()
        qp[:, k] += np.float32(M.FD_STEP)
        qm[:, k] -= np.float32(M.FD_STEP)
        fd[:, n] = (loss(qp) - loss(qm)) / (qp[:, k].astype(np.float64) - qm[:, k])
    e = float(np.abs(fd - gq[:, coords]).max() / np.abs(gq[:, coords]).max())
    print("%s %s central differences against the adjoint %.2e (bound %.0e)" % (env, _label(generic), e, M.FD_BOUND))
    assert e < M.FD_BOUND, e


def test_argument_contract(monkeypatch):
    from diffrl_amd import capi
    t, eng = _engine("humanoid", False, monkeypatch)
    q = golden("humanoid_step")["q_in"]
    n, nd = q.shape[0], t.n_qd
    full = _raw_forward(eng, t, q)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, True, False), (True, False, False), (False, False, True)):
        out = _raw_forward(eng, t, q, want)   # a NULL output is not touched; the others -- Hinv alone included -- are the full call's
        for w, a, b in zip(want, out, full):
            assert np.array_equal(a, b) if w else bool(np.isnan(a).all()), want
    tq = _T(q)
    buf = torch.empty(n * nd * nd, device=DEV)
    with pytest.raises(capi.DsimError):
        eng._call(eng._lib.dsim_mass_matrix, eng._h, n, tq.data_ptr(), None, None, None)
    with pytest.raises(capi.DsimError):
        eng._call(eng._lib.dsim_mass_matrix, eng._h, n, None, buf.data_ptr(), None, None)
    with pytest.raises(capi.DsimError):
        eng._call(eng._lib.dsim_mass_matrix_backward, eng._h, n, tq.data_ptr(), buf.data_ptr(), None, None, None)
    with pytest.raises(capi.DsimError):
        eng._call(eng._lib.dsim_mass_matrix_backward, eng._h, n, None, buf.data_ptr(), None, None, torch.empty(n * t.n_q, device=DEV).data_ptr())
    torch.cuda.synchronize()
    eng.status()


def test_non_unit_quaternion_is_reported_by_the_next_call(monkeypatch):
    from diffrl_amd import capi
    t, eng = _engine("ant", False, monkeypatch)
    step, m = golden("ant_step"), golden("ant_mass")
    q = step["q_in"]
    bad = q.copy()
    bad[5, 3:7] *= np.float32(1.001)
    eng.mass_matrix_forward(_T(bad))       # launches; the kernel marks the model
    torch.cuda.synchronize()
    with pytest.raises(capi.DsimError, match="environment 5"):
        eng.mass_matrix_forward(_T(q))     # ... and the next call on the model refuses, once
    H = eng.mass_matrix_forward(_T(q))[0]
    torch.cuda.synchronize()
    eng.status()
    assert relerr(H.cpu().numpy(), M.reference_H(t, step)) < M.FWD_BOUND
    # the adjoint launch does not check again (the forward launch of the same state did)
    eng.mass_matrix_backward(_T(bad), _T(m["c_H"]), None, None)
    torch.cuda.synchronize()
    eng.status()


_USER_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import mass_lib as M
from kin_lib import radial_part, USER_MODELS
from diffrl_amd.engine import Engine
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import project_tangent, relerr
from test_edge_cases_cpu import _tree_states
dev = torch.device("cuda:0")
T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev).reshape(-1)
for tag, path in USER_MODELS:
    t = ArticulationTemplate.load(path)
    n, nd = 6, t.n_qd
    q, qd, _ = _tree_states(t, np.random.default_rng(17), n)
    q, qd = q.astype(np.float32), qd.astype(np.float32)
    rs = np.random.RandomState(11)
    cs = tuple(rs.normal(size=s).astype(np.float32) for s in ((n, nd, nd), (n, nd, nd), (n, nd, 6)))
    # the host harness's generic kernels (held to the reference on the six recorded models) are the reference here
    ref = M.emu_mass_forward(t, q, False, 1, user=True)
    rgq = project_tangent(t, q, M.emu_mass_backward(t, q, *cs, static=False, waves=1, user=True))
    for generic in (True, False):
        if generic: os.environ["DSIM_FORCE_GENERIC"] = "1"
        else: os.environ.pop("DSIM_FORCE_GENERIC", None)
        eng = Engine(t, dev)
        assert (eng.variant == 0) == generic, (eng.variant, generic)
        H, Hinv, S = eng.mass_matrix_forward(T(q))
        gq = eng.mass_matrix_backward(T(q), *[T(c) for c in cs])
        vs = eng.body_kinematics_forward(T(q), T(qd))[2]
        torch.cuda.synchronize()
        eng.status()
        H, Hinv, S = H.cpu().numpy(), Hinv.cpu().numpy(), S.cpu().numpy().reshape(n, nd, 6)
        gq = gq.cpu().numpy().reshape(n, -1)
        bound, yard = M.residual_bound(H)
        vref = np.einsum("id,bdk,bd->bik", M.link_dof_mask(t).astype(np.float64), S.astype(np.float64), qd.astype(np.float64))
        vs = vs.cpu().numpy().reshape(n, -1, 6)
        print("RESULT %%s %%s fwd=%%.3e sym=%%.3e res=%%.3e res_bound=%%.3e vs=%%.3e gq=%%.3e radial=%%.3e" %% (
            tag, "generic" if generic else "specialised", max(relerr(H, ref[0]), relerr(S, ref[2])),
            np.abs(H - H.transpose(0, 2, 1)).max() / np.abs(H).max(), M.residual(Hinv, H), bound,
            np.abs(vs - vref).max() / np.abs(vs).max(), relerr(project_tangent(t, q, gq), rgq), radial_part(t, q, gq)))
'''


def test_user_models_vs_the_host_harness():
    """tests/inject/libdsim_user.so (generic kernels + the sets of the two user models, compiled from the same sources with no
    further work): forward against the host harness at the forward bound, the inverse by its residual, the kinematic read-out,
    and the adjoint of all three cotangents against the host harness's at the floor of the gradient bounds, 1e-4"""
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
        v = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in l.split()[3:]}
        assert v["fwd"] < M.FWD_BOUND and v["sym"] <= M.SYM_BOUND and v["res"] <= v["res_bound"] and v["vs"] < 1e-5, l
        assert v["gq"] < 1e-4 and v["radial"] <= M.RADIAL, l


def test_autograd_returns_the_raw_gradients_and_unused_outputs_get_no_cotangent(monkeypatch):
    t, eng = _engine("humanoid", False, monkeypatch)
    q0, m = golden("humanoid_step")["q_in"], golden("humanoid_mass")
    B, nd = q0.shape[0], t.n_qd
    c = [_T(m["c_H"]).view(B, nd, nd), _T(m["c_Hinv"]).view(B, nd, nd), _T(m["c_S"]).view(-1, 6)]
    seen = []
    raw = eng.mass_matrix_backward
    monkeypatch.setattr(eng, "mass_matrix_backward", lambda *a: (seen.append([x is not None for x in a[1:]]), raw(*a))[1])
    q = _T(q0).requires_grad_(True)
    out = eng.mass_matrix(q)
    assert all(o.grad_fn is not None for o in out)
    assert [tuple(o.shape) for o in out] == [(B, nd, nd), (B, nd, nd), (B * nd, 6)]
    sum((o * x).sum() for o, x in zip(out, c)).backward()
    assert torch.equal(q.grad, raw(_T(q0), *c)) and seen[-1] == [True] * 3
    for k in range(3):   # one output: the others arrive as None (no zero-filled buffers are materialised)
        q = _T(q0).view(B, -1).requires_grad_(True)
        (eng.mass_matrix(q)[k] * c[k]).sum().backward()
        gq = raw(_T(q0), *[x if j == k else None for j, x in enumerate(c)])
        assert seen[-1] == [j == k for j in range(3)] and torch.equal(q.grad.reshape(-1), gq) and q.grad.shape == q.shape
    torch.cuda.synchronize()


@pytest.mark.parametrize("env", ("ant", "snu"))
def test_step_then_mass_matrix_under_one_backward_is_the_two_raw_calls_chained(env, monkeypatch):
    from diffrl_amd.engine import SimStep
    t, eng = _engine(env, False, monkeypatch)
    step, m = golden(env + "_step"), golden(env + "_mass")
    B, nd = step["q_in"].shape[0], t.n_qd
    S, mm, dt = int(step["substeps"]), int(step["mm_freq"]), float(step["dt"])
    q0, qd0, act0, mact0, muscles = dyn_lib.inputs(step)
    if muscles:
        act0 = np.zeros_like(qd0)
    q, qd, act = _T(q0).requires_grad_(True), _T(qd0).requires_grad_(True), _T(act0).requires_grad_(True)
    mact = _T(mact0).requires_grad_(True) if muscles else None
    c = [_T(m["c_H"]).view(B, nd, nd), _T(m["c_Hinv"]).view(B, nd, nd), _T(m["c_S"]).view(-1, 6)]
    qo, qdo = SimStep.apply(eng, dt, S, mm, q, qd, act, mact)
    sum((o * x).sum() for o, x in zip(eng.mass_matrix(qo), c)).backward()
    # the same by hand: the read-out's adjoint at the step's output, then the step's adjoint with that cotangent on q_out
    qo2, qdo2, ck = eng.forward(_T(q0), _T(qd0), _T(act0), _T(mact0) if muscles else None, dt, S, mm, True)
    assert torch.equal(qo2, qo.detach())
    gqo = eng.mass_matrix_backward(qo2, *c)
    g = eng.backward(ck, _T(act0), _T(mact0) if muscles else None, dt, S, mm, gqo, torch.zeros_like(qdo2))
    torch.cuda.synchronize()
    eng.status()
    assert torch.equal(q.grad, g[0]) and torch.equal(qd.grad, g[1]) and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0
    assert torch.equal(mact.grad if muscles else act.grad, g[3] if muscles else g[2])


def test_graph_replay_of_forward_plus_backward_is_bit_identical_to_eager(monkeypatch):
    t, eng = _engine("humanoid", False, monkeypatch)
    q0, m = golden("humanoid_step")["q_in"], golden("humanoid_mass")
    B, nd = q0.shape[0], t.n_qd
    q = _T(q0)
    c = [_T(m["c_H"]), _T(m["c_Hinv"]), _T(m["c_S"])]
    res = [torch.zeros((B, nd, nd), device=DEV), torch.zeros((B, nd, nd), device=DEV), torch.zeros((B * nd, 6), device=DEV),
           torch.zeros(B * t.n_q, device=DEV)]

    def run():   # a linear graph: forward, backward, four copies
        out = eng.mass_matrix_forward(q)
        gq = eng.mass_matrix_backward(q, *c)
        for dst, src in zip(res, out + (gq,)):
            dst.copy_(src)

    run()
    torch.cuda.synchronize()
    eager = [r.clone() for r in res]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        run()
    for _ in range(2):
        for r in res:
            r.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(r, e) for r, e in zip(res, eager))
    eng.status()


def test_model_surface_and_the_link_jacobian():
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=4, device=DEV, no_grad=False, stochastic_init=False, MM_caching_frequency=16)
    e.reset()
    t = e.model.template()
    L, nd = e.model.links_per_articulation, t.n_qd
    mask = e.model.link_dof_mask
    assert mask.shape == (L, nd) and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), M.link_dof_mask(t))
    a = torch.zeros((4, 8), device=DEV, requires_grad=True)
    e.step(torch.tanh(a + 0.1))
    H, Hinv, S = e.model.mass_matrix(e.state)
    assert H.shape == (4, nd, nd) and Hinv.shape == (4, nd, nd) and S.shape == (4 * nd, 6)
    assert all(x.grad_fn is not None for x in (H, Hinv, S))
    # the twist of the last link is its Jacobian times qd
    qd = e.state.joint_qd.view(4, nd)
    J = (mask[L - 1].view(1, nd, 1) * S.view(4, nd, 6)).transpose(1, 2)
    v = e.model.engine().body_kinematics_forward(e.state.joint_q.detach(), e.state.joint_qd.detach())[2].view(4, L, 6)[:, L - 1]
    assert float((torch.einsum("bkd,bd->bk", J, qd) - v).abs().max()) <= 1e-5 * float(v.abs().max())
    (0.5 * torch.einsum("bi,bij,bj->", qd, H, qd) + torch.einsum("bki,bij,bkj->", J, Hinv, J)).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(a.grad).all() and a.grad.abs().sum() > 0


def test_the_example_prints_the_same_loss_eager_and_graphed(capsys):
    """examples/inertia_lite.py: the first iteration's loss (the same actor, the same start state) of the eager run and of the
    run that captures the whole rollout, as printed"""
    spec = importlib.util.spec_from_file_location("inertia_lite", os.path.join(ROOT, "examples", "inertia_lite.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    printed = []
    for flags in ([], ["--graph"]):
        hist = ex.main(["--envs", "16", "--horizon", "3", "--iters", "2", "--settle", "12"] + flags)
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("loss:")]
        assert len(line) == 1 and ("graph" if flags else "eager") in line[0], line
        assert all(np.isfinite(v) for row in hist for v in row) and hist[0][1] > 0 and hist[0][2] > 0
        printed.append(line[0].split(";")[0].split(",")[0])   # "loss: first iteration <value>"
    print(printed)
    assert printed[0] == printed[1], printed
