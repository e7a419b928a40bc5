"""-m gpu: the step Jacobian on the real HIP kernels -- dsim_step_backward_multi / dsim_step_jacobian through the C ABI,
Engine.backward_multi / Engine.step_jacobian, SemiImplicitIntegrator.linearize, a captured replay and the example.

The new launch runs the unchanged step adjoint once per (environment, cotangent) workgroup, so its first property is BIT
equality with sequential dsim_step_backward calls; the comparison with the reference's recording (tests/golden/<env>_lin.npz)
uses the bounds of tests/test_step_jacobian_cpu.py (tests/jac_lib.py has the reasoning): every block in its own max-norm, q_in
columns after project_tangent, 1e-3; at most one block per model excluded where the reference's own +-1 ulp noise exceeds 1e-4.
N = 3 environments unless stated."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jac_lib as J
from oracle_lib import golden, template_from_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_LIB = os.path.join(ROOT, "tests", "inject", "libdsim_user.so")
DEV = "cuda:0"
N = 3


def _engine(env, generic, monkeypatch, lean=False):
    from diffrl_amd.engine import Engine
    if generic:
        monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("DSIM_FORCE_GENERIC", raising=False)
    t = template_from_golden(env)
    eng = Engine(t, torch.device(DEV), ckpt_mode="lean" if lean else "full")
    assert (eng.variant == 0) == generic
    return t, eng


def _T(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV).reshape(-1) if a is not None else None


def _step_inputs(env, n=N, mm=None):
    """the first n states of the step fixture (tiled if it has fewer) -> (q, qd, act, mact | None, dt, S, mm) on the device"""
    g = golden(env + "_step")
    rows = np.arange(n) % g["q_in"].shape[0]
    mact = _T(g["muscle_act_in"][rows]) if "muscle_act_in" in g else None
    return (_T(g["q_in"][rows]), _T(g["qd_in"][rows]), _T(g["act_in"][rows]), mact, float(g["dt"]), int(g["substeps"]),
            int(g["mm_freq"]) if mm is None else mm)


def _sequential(eng, ck, act, mact, dt, S, mm, gq, gqd):
    """K calls to dsim_step_backward, stacked: gq [n, K, n_q], gqd [n, K, n_qd] -> the four outputs as [n, K, .]"""
    n, K = gq.shape[0], gq.shape[1]
    outs = [eng.backward(ck, act, mact, dt, S, mm, gq[:, k].contiguous(), gqd[:, k].contiguous()) for k in range(K)]
    return tuple(torch.stack([o[j].view(n, -1) for o in outs], dim=1) if outs[0][j] is not None else None for j in range(4))


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _bit_equality(eng, inputs, seed=7):
    q, qd, act, mact, dt, S, mm = inputs
    n, nq, nd = q.numel() // eng.n_q, eng.n_q, eng.n_qd
    Kf = nq + nd
    _, _, ck = eng.forward(q, qd, act, mact, dt, S, mm, True)
    gen = torch.Generator().manual_seed(seed)
    gq, gqd = torch.randn((n, Kf, nq), generator=gen).to(DEV), torch.randn((n, Kf, nd), generator=gen).to(DEV)
    own = _sequential(eng, ck, act, mact, dt, S, mm, gq, gqd)
    shared = _sequential(eng, ck, act, mact, dt, S, mm, gq[:1].expand(n, Kf, nq), gqd[:1].expand(n, Kf, nd))
    for K in (1, 2, Kf):
        cut = lambda r: tuple(x[:, :K] if x is not None else None for x in r)   # noqa: E731
        got = eng.backward_multi(ck, act, mact, dt, S, mm, gq[:, :K].contiguous(), gqd[:, :K].contiguous(), shared=False)
        assert got[0].shape == (n, K, nq) and got[1].shape == (n, K, nd) and got[2].shape == (n, K, nd)
        assert _same(got, cut(own)), ("per-environment cotangents", K)
        got = eng.backward_multi(ck, act, mact, dt, S, mm, gq[0, :K].contiguous(), gqd[0, :K].contiguous(), shared=True)
        assert _same(got, cut(shared)), ("shared cotangents", K)
    assert all(x is None or bool(torch.isfinite(x).all()) for x in own)
    assert (own[3] is not None) == (eng.n_muscles > 0)
    torch.cuda.synchronize()
    eng.status()


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", J.ENVS)
def test_multi_equals_sequential_backward_bit_for_bit(env, generic, lean, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch, lean)
    _bit_equality(eng, _step_inputs(env))


def test_multi_equals_sequential_backward_with_a_mass_matrix_every_substep(monkeypatch):
    t, eng = _engine("ant", False, monkeypatch)
    _bit_equality(eng, _step_inputs("ant", mm=1))


_USER_SCRIPT = r'''
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import test_gpu_step_jacobian as G
from kin_lib import USER_MODELS
from diffrl_amd.engine import Engine
from diffrl_amd.template import ArticulationTemplate
from test_edge_cases_cpu import _tree_states
dev = torch.device("cuda:0")
for tag, path in USER_MODELS:
    t = ArticulationTemplate.load(path)
    q, qd, act = _tree_states(t, np.random.default_rng(17), G.N)
    for generic in (True, False):
        if generic: os.environ["DSIM_FORCE_GENERIC"] = "1"
        else: os.environ.pop("DSIM_FORCE_GENERIC", None)
        for mode in ("full", "lean"):
            eng = Engine(t, dev, ckpt_mode=mode)
            assert (eng.variant == 0) == generic, (eng.variant, generic)
            G._bit_equality(eng, (G._T(q), G._T(qd), G._T(act), None, 1.0 / 60.0, 4, 2))
            print("RESULT %%s %%s %%s ok" %% (tag, "generic" if generic else "specialised", mode))
'''


def test_user_models_multi_equals_sequential_backward():
    """tests/inject/libdsim_user.so: the generic kernels + the sets of the two user models, through the template and specialise path"""
    if not os.path.exists(USER_LIB):
        pytest.fail("tests/inject/libdsim_user.so is missing: __graft_entry__.build() makes it with python -m diffrl_amd.specialise")
    e = dict(os.environ, DSIM_LIB=USER_LIB)
    e.pop("DSIM_FORCE_GENERIC", None)
    r = subprocess.run([sys.executable, "-c", _USER_SCRIPT % dict(root=ROOT)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    res = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    print("\n".join(res))
    assert len(res) == 8, r.stdout


def _lin_jacobian(env, generic, monkeypatch):
    t, eng = _engine(env, generic, monkeypatch)
    _, inp, lin = J.case(env)
    act, mact = _T(inp["act"]), _T(inp["mact"])
    _, _, ck = eng.forward(_T(inp["q"]), _T(inp["qd"]), act, mact, inp["dt"], inp["S"], inp["mm"], True)
    return t, eng, inp, lin, ck, act, mact


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("env", J.ENVS)
def test_jacobian_equals_multi_with_identity_seeds_and_matches_the_reference(env, generic, monkeypatch):
    t, eng, inp, lin, ck, act, mact = _lin_jacobian(env, generic, monkeypatch)
    a = (inp["dt"], inp["S"], inp["mm"])
    nq, K = t.n_q, t.n_q + t.n_qd
    Js, Ja, Jm = eng.step_jacobian(ck, act, mact, *a)
    B = ck.shape[0]
    assert Js.shape == (B, K, K) and Ja.shape == (B, K, t.n_qd) and (Jm is None) == (t.n_muscles == 0)
    eye = torch.eye(K, device=DEV)
    m = eng.backward_multi(ck, act, mact, *a, eye[:, :nq].contiguous(), eye[:, nq:].contiguous(), shared=True)
    assert torch.equal(torch.cat([m[0], m[1]], dim=2), Js) and torch.equal(m[2], Ja) and (Jm is None or torch.equal(m[3], Jm))
    torch.cuda.synchronize()
    eng.status()
    label = "generic" if generic else "specialised"
    Jn = Js.cpu().numpy()
    J.compare(env, label, t, inp["q"], lin, Jn, Ja.cpu().numpy(), Jm.cpu().numpy() if Jm is not None else None)
    # quaternion blocks of the q_in columns are tangent
    rad = J.radial(t, inp["q"], Jn[:, :, :nq])
    print(env, label, "|J[:, quaternion block] . quat_in| / max |J| = %.2e (bound %.0e)" % (rad, J.RADIAL))
    assert rad <= J.RADIAL


def test_contract_determinism_null_outputs_sentinels_and_error_codes(monkeypatch):
    from diffrl_amd import capi
    t, eng, inp, lin, ck, act, mact = _lin_jacobian("snu", False, monkeypatch)
    a = (inp["dt"], inp["S"], inp["mm"])
    B, nq, nd, M = ck.shape[0], t.n_q, t.n_qd, t.n_muscles
    K = nq + nd
    first = eng.step_jacobian(ck, act, mact, *a)
    again = eng.step_jacobian(ck, act, mact, *a)
    assert _same(first, again)                                     # two launches agree bit for bit
    lib, h = eng._lib, eng._h
    P = lambda x: x.data_ptr() if x is not None else None   # noqa: E731

    def buf(cols):   # one row too long: the extra row is a sentinel
        return torch.full((B * K + 1, cols), 7.0, device=DEV)

    def call(n, Js, Ja, Jm, ckpt=ck):
        return lib.dsim_step_jacobian(h, n, P(ckpt), P(act), P(mact), C.c_float(a[0]), a[1], a[2], P(Js), P(Ja), P(Jm), None)

    Js, Ja, Jm = buf(K), buf(nd), buf(M)
    assert call(B, Js, Ja, Jm) == capi.OK
    torch.cuda.synchronize()
    for o, ref in ((Js, first[0]), (Ja, first[1]), (Jm, first[2])):
        assert torch.equal(o[:-1].reshape(ref.shape), ref) and bool((o[-1] == 7.0).all())
    # NULL J_act / J_muscle are skipped: J_state is what the full call writes, the skipped buffers are not touched
    Js2 = buf(K)
    assert call(B, Js2, None, None) == capi.OK
    torch.cuda.synchronize()
    assert torch.equal(Js2, Js)
    # the multi call: sentinels behind every output, NULL gact / gmuscle_act skipped
    gen = torch.Generator().manual_seed(1)
    gq, gqd = torch.randn((2, nq), generator=gen).to(DEV), torch.randn((2, nd), generator=gen).to(DEV)
    ref = eng.backward_multi(ck, act, mact, *a, gq, gqd, shared=True)
    o = [torch.full((B * 2 + 1, c), 7.0, device=DEV) for c in (nq, nd, nd, M)]

    def multi(n, k, outs, gq_=gq):
        return lib.dsim_step_backward_multi(h, n, k, 1, P(ck), P(act), P(mact), C.c_float(a[0]), a[1], a[2], P(gq_), P(gqd),
                                            P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), None)

    assert multi(B, 2, o) == capi.OK
    torch.cuda.synchronize()
    for x, r in zip(o, ref):
        assert torch.equal(x[:-1].reshape(r.shape), r) and bool((x[-1] == 7.0).all())
    o2 = [torch.full((B * 2 + 1, c), 7.0, device=DEV) for c in (nq, nd)]
    assert multi(B, 2, o2 + [None, None]) == capi.OK
    torch.cuda.synchronize()
    assert torch.equal(o2[0], o[0]) and torch.equal(o2[1], o[1])
    # error codes, returned before anything is launched: the output buffers keep their fill
    fresh = [torch.full((B * 2 + 1, c), 7.0, device=DEV) for c in (nq, nd, nd, M)]
    assert multi(B, 0, fresh) == capi.ERR_INVALID and multi(B, -1, fresh) == capi.ERR_INVALID     # n_cot <= 0
    assert multi(B, 2, fresh, gq_=None) == capi.ERR_INVALID                                       # a required pointer
    assert multi(B, 2, [None] + fresh[1:]) == capi.ERR_INVALID
    assert call(B, None, Ja, Jm) == capi.ERR_INVALID and call(B, Js, Ja, Jm, ckpt=None) == capi.ERR_INVALID
    assert multi(1 << 23, 2, fresh) == capi.ERR_LIMIT                                             # 2^24 workgroups: over the grid limit
    assert call(1 << 20, Js, Ja, Jm) == capi.ERR_LIMIT                                            # 2^20 * 53
    assert b"grid limit" in lib.dsim_last_error()
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in fresh)
    # the Python layer refuses a checkpoint of another geometry and actuation of another batch
    with pytest.raises(capi.DsimError):
        eng.step_jacobian(ck[:, :-4].contiguous(), act, mact, *a)
    with pytest.raises(capi.DsimError):
        eng.step_jacobian(ck, act[:nd], mact, *a)
    with pytest.raises(capi.DsimError):
        eng.backward_multi(ck, act, mact, *a, gq, gqd[:1], shared=True)
    eng.status()


@pytest.mark.parametrize("env", ["ant", "cartpole"])
def test_engine_jacobian_rows_equal_autograd_through_simstep(env, monkeypatch):
    from diffrl_amd.engine import SimStep
    t, eng = _engine(env, False, monkeypatch)
    q, qd, act, mact, dt, S, mm = _step_inputs(env)
    nq, nd = t.n_q, t.n_qd
    K = nq + nd
    ql, qdl, al = q.clone().requires_grad_(True), qd.clone().requires_grad_(True), act.clone().requires_grad_(True)
    qo, qdo = SimStep.apply(eng, dt, S, mm, ql, qdl, al, None)
    out = torch.cat([qo.view(N, nq), qdo.view(N, nd)], dim=1)
    _, _, ck = eng.forward(q, qd, act, None, dt, S, mm, True)
    Js, Ja, _ = eng.step_jacobian(ck, act, None, dt, S, mm)
    for k in range(K):
        seed = torch.zeros_like(out)
        seed[:, k] = 1.0
        gq, gqd, ga = torch.autograd.grad(out, (ql, qdl, al), seed, retain_graph=True)
        assert torch.equal(Js[:, k, :nq], gq.view(N, nq)) and torch.equal(Js[:, k, nq:], gqd.view(N, nd)), k
        assert torch.equal(Ja[:, k], ga.view(N, nd)), k
    torch.cuda.synchronize()
    eng.status()


def test_linearize_returns_the_state_of_forward_and_the_engine_jacobian():
    from diffrl_amd import envs
    e = envs.AntEnv(num_envs=4, device=DEV, no_grad=True, stochastic_init=False, MM_caching_frequency=16)
    e.reset()
    st = e.model.state()
    st.joint_q, st.joint_qd = e.state.joint_q.detach().clone(), e.state.joint_qd.detach().clone()
    gen = torch.Generator().manual_seed(2)
    st.joint_act = torch.cat([torch.zeros((4, 6)), 100.0 * (2.0 * torch.rand((4, 8), generator=gen) - 1.0)], dim=1).reshape(-1).to(DEV)
    a = (e.sim_dt, e.sim_substeps, e.MM_caching_frequency)
    ref = e.integrator.forward(e.model, st, *a)
    out, A, B = e.integrator.linearize(e.model, st, *a)
    assert torch.equal(out.joint_q, ref.joint_q) and torch.equal(out.joint_qd, ref.joint_qd)
    nq, nd = e.model.coords_per_articulation, e.model.dofs_per_articulation
    assert A.shape == (4, nq + nd, nq + nd) and B.shape == (4, nq + nd, nd)
    assert not A.requires_grad and not B.requires_grad and not out.joint_q.requires_grad
    eng = e.model.engine()
    _, _, ck = eng.forward(st.joint_q, st.joint_qd, st.joint_act, None, float(a[0]), int(a[1]), int(a[2]), True)
    Js, Ja, _ = eng.step_jacobian(ck, st.joint_act, None, float(a[0]), int(a[1]), int(a[2]))
    assert torch.equal(A, Js) and torch.equal(B, Ja) and bool(torch.isfinite(A).all()) and float(B.abs().max()) > 0
    torch.cuda.synchronize()


def test_graph_replay_of_forward_plus_jacobian_is_bit_identical_to_eager(monkeypatch):
    t, eng = _engine("ant", False, monkeypatch)
    q, qd, act, _, dt, S, mm = _step_inputs("ant", n=4)
    K = t.n_q + t.n_qd
    res = [torch.zeros(4 * t.n_q, device=DEV), torch.zeros((4, K, K), device=DEV), torch.zeros((4, K, t.n_qd), device=DEV)]

    def run():   # a linear graph: forward, Jacobian, three copies
        qo, _, ck = eng.forward(q, qd, act, None, dt, S, mm, True)
        Js, Ja, _ = eng.step_jacobian(ck, act, None, dt, S, mm)
        for dst, src in zip(res, (qo, Js, Ja)):
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


@pytest.mark.parametrize("flags", [[], ["--graph"]], ids=["eager", "graph"])
def test_example_prints_finite_numbers(flags):
    e = dict(os.environ)
    e.pop("DSIM_FORCE_GENERIC", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "jacobian_lite.py")] + flags, cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-1500:])
    print(r.stdout)
    rows = [l.replace("/", " ").split() for l in r.stdout.splitlines() if l.strip() and l.split()[0].isdigit()]
    assert len(rows) == 16 and all(len(x) == 5 for x in rows), r.stdout
    assert all(np.isfinite(float(v)) for x in rows for v in x[1:])
