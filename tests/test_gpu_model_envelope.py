"""-m gpu: the generic (run-time layout) kernels on models at the edges of what dsim_model_create admits (include/dsim.h "Admitted
models"): 64 links and 64 dofs at once (A), contact items that no longer fit beside the link lanes of one wave (B), 64 dofs on 22
links (C), more than 64 contacts without muscles -- the four-wave kernels (D), the literal adjoint at its limit (E), muscles on a
tree of 40 links (F).  tests/big_models.py builds them and asserts what puts each on its path; tests/test_model_envelope_cpu.py
runs the same models through the host harness.  References: the scalar oracle, the float64 statements of the read-outs, float64
numpy for H.  Bounds: tests/test_gpu_edge_cases.py::test_generic_kernels_on_random_trees for the step (state 1e-4 / 1e-3,
gradients 1e-3; the probe of step_grad_tolerance has a budget of 0 here), the read-outs' own GPU tests for the read-outs.
Measured figures: profiles/model_envelope.txt."""

import numpy as np
import pytest
import torch

import big_models as bm
import con_lib
import dyn_lib
import kin_lib
import mass_lib
import par_lib
from diffrl_amd import capi
from oracle_lib import oracle_backward, oracle_forward, project_tangent, relerr, step_grad_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 5
_engines = {}


@pytest.fixture(scope="module")
def models():
    """name -> template, built once"""
    return {name: bm.model(name)[0] for name in bm.MODELS}


def T(a, cols=None):
    x = torch.tensor(np.ascontiguousarray(a, np.float32), device=torch.device(DEV))
    return x.reshape(-1) if cols is None else x.reshape(-1, cols)


def A(x, n=N):
    return x.cpu().numpy().reshape(n, -1)


def _engine(models, name, mode="full"):
    """the model's Engine with the wave count the library picks (no DSIM_WAVES), one per checkpoint mode"""
    from diffrl_amd.engine import Engine
    if (name, mode) not in _engines:
        eng = Engine(models[name], DEV, ckpt_mode=mode)
        assert eng.variant == 0, "these models have no kernel set of their own: the generic kernels"
        assert eng.waves == bm.expected_waves(bm.dims_of(models[name])[1])
        _engines[(name, mode)] = eng
    return _engines[(name, mode)]


def _step(eng, x, S, mm, literal=False):
    """-> (q_out, qd_out, gq, gqd, gact, gmact | None) as [n, .] arrays"""
    q, qd, act, mact, gq, gqd = x
    n, dt = q.shape[0], S / 960.0
    m = T(mact) if mact is not None else None
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), m, dt, S, mm, True)
    r = eng.backward(ck, T(act), m, dt, S, mm, T(gq), T(gqd), literal=literal)
    torch.cuda.synchronize()
    eng.status()
    return tuple(A(v, n) if v is not None else None for v in (qo, qdo) + tuple(r))


def _hold_oracle_bounds(t, x, out, o, S, mm, what):
    q, qd, act, mact, gq, gqd = x
    state, err = bm.step_errors(t, q, out, o)
    print(what, (S, mm), " ".join("%s %.2e" % kv for kv in list(state.items()) + list(err.items())))
    assert state["q"] < 1e-4 and state["qd"] < 1e-3, state
    tol = step_grad_tolerance(t, q, qd, act, mact, S / 960.0, S, mm, gq, gqd, err, ref=o, what=what)   # 1e-3; probed: budget 0
    assert all(err[k] < tol[k] for k in err), (err, tol)


@pytest.mark.parametrize("name", sorted(bm.MODELS))
def test_wave_count_and_kernel_set(models, name):
    eng = _engine(models, name)
    off, d = bm.check_property(name, models[name])
    assert eng.variant == 0 and eng.waves == {"A": 1, "B": 1, "C": 1, "D": 4, "E": 1, "E25": 1, "F": 4}[name]


@pytest.mark.parametrize("mode", ["full", "lean"])
@pytest.mark.parametrize("S,mm", bm.SCHEDULES)
@pytest.mark.parametrize("name", bm.BASE)
def test_step_against_the_oracle(models, name, S, mm, mode):
    """forward, backward and (F) the muscle gradient, five environments"""
    t = models[name]
    x, o = bm.oracle_case(name, N, S, mm)
    out = _step(_engine(models, name, mode), x, S, mm)
    _hold_oracle_bounds(t, x, out, o, S, mm, "%s %s" % (name, mode))
    if t.n_muscles:
        assert np.abs(o["gmact"]).max() > 0
    if mode == "lean":   # the adjoint recomputes the forward phases with the same code: nothing differs (include/dsim.h)
        full = _step(_engine(models, name, "full"), x, S, mm)
        assert all(np.array_equal(a, b) for a, b in zip(out, full) if a is not None)


@pytest.mark.parametrize("name,waves", [("A", 4), ("B", 4), ("C", 4), ("D", 1)])
def test_the_other_wave_count(models, name, waves, monkeypatch):
    """DSIM_WAVES at Engine creation puts the model on the kernels it would not get by itself.  Both directions hold the oracle
    bounds.  Against the library's own choice ALL tensors -- q_out, qd_out, gq, gqd, gact -- are expected bit-identical: a wave
    count changes which lane does an item of a per-item loop, never the order of a sum (the per-link, per-dof and per-contact
    sums run over the same lists in the same order; the host harness, which executes the same phase code with 64 and with 256
    lanes, gives identical bits on all six models: tests/test_model_envelope_cpu.py)."""
    from diffrl_amd.engine import Engine
    t = models[name]
    own_eng = _engine(models, name)   # (created, or taken from the cache, before the override is in the environment)
    monkeypatch.setenv("DSIM_WAVES", str(waves))
    eng = Engine(t, DEV)
    assert eng.variant == 0 and eng.waves == waves != own_eng.waves
    for S, mm in bm.SCHEDULES:
        x, o = bm.oracle_case(name, N, S, mm)
        out = _step(eng, x, S, mm)
        _hold_oracle_bounds(t, x, out, o, S, mm, "%s DSIM_WAVES=%d" % (name, waves))
        own = _step(own_eng, x, S, mm)
        diff = [relerr(a, b) for a, b in zip(out[:5], own[:5])]
        print(name, (S, mm), "against the library's own wave count (q qd gq gqd gact):", " ".join("%.2e" % e for e in diff))
        assert all(np.array_equal(a, b) for a, b in zip(out[:5], own[:5])), diff


def test_literal_adjoint_at_its_limit(models):
    """E: 24 links / 28 dofs, dsim_step_backward_literal against the oracle's literal gq, un-projected, 1e-3 (tests/test_gpu_parity.py::
    test_literal_backward_vs_oracle_batch, its step geometry too: the first mass-matrix group shorter than the step)"""
    t = models["E"]
    x = bm.states("E", N)
    q, qd, act, mact, gq, gqd = x
    S, mm = 6, 4
    o = oracle_backward(t, q, qd, act, mact, S / 960.0, S, mm, gq, gqd)
    out = _step(_engine(models, "E"), x, S, mm, literal=True)
    e = (relerr(out[2], o["gq"]), relerr(out[3], o["gqd"]))
    print("E literal gq %.2e gqd %.2e" % e)
    assert e[0] < 1e-3 and e[1] < 1e-3
    plain = _step(_engine(models, "E"), x, S, mm)
    assert relerr(plain[2], o["gq"]) > 1e-3, "the reference's radial component is in the comparison"


def test_one_link_beyond_the_literal_limit(models):
    """E25: dsim_step_backward_literal returns DSIM_ERR_LIMIT, every other call works"""
    t = models["E25"]
    eng = _engine(models, "E25")
    S, mm = 3, 3
    x, o = bm.oracle_case("E25", N, S, mm)
    q, qd, act, mact, gq, gqd = x
    out = _step(eng, x, S, mm)
    _hold_oracle_bounds(t, x, out, o, S, mm, "E25")
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), None, S / 960.0, S, mm, True)
    with pytest.raises(capi.DsimError, match="dsim error -3: dsim_step_backward_literal handles models of up to 24 links and 28 dofs"):
        eng.backward(ck, T(act), None, S / 960.0, S, mm, T(gq), T(gqd), literal=True)
    r = eng.backward_params(ck, T(act), None, S / 960.0, S, mm, T(gq), T(gqd))
    J = eng.step_jacobian(ck[:1], T(act[:1]), None, S / 960.0, S, mm)
    H = eng.mass_matrix_forward(T(q))
    torch.cuda.synchronize()
    assert np.array_equal(A(r[0]), out[2]) and torch.isfinite(J[0]).all() and torch.isfinite(H[1]).all()


@pytest.mark.parametrize("name", ["A", "C", "D", "F"])
def test_many_cotangents_equal_single_sweeps(models, name):
    """backward_multi with K = 3 shared cotangents equals three single sweeps bit for bit; A: the rows of step_jacobian equal
    identity-seeded sweeps at two environments"""
    t = models[name]
    eng = _engine(models, name)
    q, qd, act, mact, gq, gqd = bm.states(name, N)
    S, mm = 3, 3
    dt = S / 960.0
    m = T(mact) if mact is not None else None
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), m, dt, S, mm, True)
    rng = np.random.default_rng(3)
    cq, cqd = rng.normal(size=(3, t.n_q)).astype(np.float32), rng.normal(size=(3, t.n_qd)).astype(np.float32)
    multi = eng.backward_multi(ck, T(act), m, dt, S, mm, T(cq), T(cqd), shared=True)
    for k in range(3):
        r = eng.backward(ck, T(act), m, dt, S, mm, T(np.tile(cq[k], (N, 1))), T(np.tile(cqd[k], (N, 1))))
        for a, b in zip(multi, r):
            if a is not None:
                assert torch.equal(a[:, k].reshape(-1), b.reshape(-1)), (name, k)
    if name == "A":
        n, K = 2, t.n_q + t.n_qd
        J, Ja, Jm = eng.step_jacobian(ck[:n].contiguous(), T(act[:n]), None, dt, S, mm)
        assert torch.isfinite(J).all() and torch.isfinite(Ja).all()
        for k in (0, t.n_q - 1, t.n_q, K - 1):
            e = np.zeros((n, K), np.float32)
            e[:, k] = 1.0
            r = eng.backward(ck[:n].contiguous(), T(act[:n]), None, dt, S, mm, T(e[:, :t.n_q]), T(e[:, t.n_q:]))
            assert torch.equal(J[:, k, :t.n_q].reshape(-1), r[0]) and torch.equal(J[:, k, t.n_q:].reshape(-1), r[1])
            assert torch.equal(Ja[:, k].reshape(-1), r[2])
    torch.cuda.synchronize()
    eng.status()


@pytest.mark.parametrize("name", ["A", "D", "F"])
def test_parameter_gradients(models, name):
    """the state gradients of backward_params equal backward bit for bit; g_dof / g_contact are written, finite and equal the host
    harness's at par_lib.param_bound of a tensor without recorded reference noise (its floor, 1e-4)"""
    t = models[name]
    eng = _engine(models, name)
    x = bm.states(name, N)
    q, qd, act, mact, gq, gqd = x
    S, mm = 3, 2
    dt = S / 960.0
    m = T(mact) if mact is not None else None
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), m, dt, S, mm, True)
    plain = eng.backward(ck, T(act), m, dt, S, mm, T(gq), T(gqd))
    r = eng.backward_params(ck, T(act), m, dt, S, mm, T(gq), T(gqd))
    torch.cuda.synchronize()
    eng.status()
    for a, b in zip(r[:4], plain):
        if a is not None:
            assert torch.equal(a, b)
    g_dof, g_con = r[4].cpu().numpy(), r[5].cpu().numpy()
    assert g_dof.shape == (N, 5, t.n_qd) and g_con.shape == (N, t.n_contacts, 4) and np.isfinite(g_dof).all() and np.isfinite(g_con).all() and g_dof.any() and g_con.any()
    kw = dict(static=False, waves=eng.waves)
    hq, hqd, hck = par_lib.emu_par_forward(t, q, qd, act, mact, dt, S, mm, **kw)
    host = par_lib.emu_par_backward(t, hck, act, mact, dt, S, mm, gq, gqd, **kw)
    bound = par_lib.param_bound(0.0)
    for r_, k in enumerate(par_lib.DOF_ROWS):
        e = relerr(g_dof[:, r_], host["g_dof"][:, r_])
        print(name, "g_dof", k, "%.2e" % e)
        assert e < bound, (k, e)
    for j, k in enumerate(("ke", "kd", "kf", "mu")):
        e = relerr(g_con[..., j], host["g_contact"][..., j])
        print(name, "g_contact", k, "%.2e" % e)
        assert e < bound, (k, e)


@pytest.mark.parametrize("name", ["A", "D"])
def test_read_outs(models, name):
    """the four read-outs, forward and backward, with the references and bounds of their GPU tests on the user trees: kinematics
    against the float64 statement (1e-5), tau / qdd / f_s against the oracle's first substep (1e-4), the qdd adjoint against the
    step adjoint of one substep (dyn_lib.CHECK_BOUND), ground
    contacts against the float64 statement (1e-4; adjoint 10 x the statement's +-1 ulp noise, floor 1e-5), H and S against float64
    numpy J^T M J + diag(armature) (1e-5), Hinv by its residual, the mass-matrix adjoint against the host harness's (1e-4), which
    tests/test_model_envelope_cpu.py holds to central differences on the same models"""
    from test_ground_contacts_cpu import grad_bound, rows_err
    t = models[name]
    eng = _engine(models, name)
    q, qd, act = bm.states(name, N)[:3]
    L, nd, Cn = t.n_links, t.n_qd, t.n_contacts
    # kinematics
    rng = np.random.default_rng(17)
    c = [rng.normal(size=(N, L, 7)).astype(np.float32), rng.normal(size=(N, L, 7)).astype(np.float32), rng.normal(size=(N, L, 6)).astype(np.float32)]
    xsc, xsm, vs = eng.body_kinematics_forward(T(q), T(qd))
    gq, gqd = eng.body_kinematics_backward(T(q), T(qd), T(c[0], 7), T(c[1], 7), T(c[2], 6))
    r = kin_lib.fk_batch(t, q, qd)
    rq, rqd = kin_lib.fk_adjoint_batch(t, q, qd, *c)
    errs = dict(X_sc=relerr(xsc.cpu().numpy().reshape(N, L, 7), r[0]), X_sm=relerr(xsm.cpu().numpy().reshape(N, L, 7), r[1]),
                v_s=relerr(vs.cpu().numpy().reshape(N, L, 6), r[2]), gq=relerr(A(gq), rq), gqd=relerr(A(gqd), rqd))
    print(name, "kinematics", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(e < 1e-5 for e in errs.values()), errs
    assert kin_lib.radial_part(t, q, A(gq)) <= 1e-6
    # joint dynamics: the qdd adjoint against the step adjoint of one substep
    h = dyn_lib.CHECK_H
    g = np.random.default_rng(5).normal(size=qd.shape).astype(np.float32)
    dq, dqd, dact, _ = eng.joint_dynamics_backward(T(q), T(qd), T(act), None, None, T(g), None)
    tau, qdd, fs = eng.joint_dynamics_forward(T(q), T(qd), T(act), None)
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), None, h, 1, 1, True)
    sq, sqd, sact, _ = eng.backward(ck, T(act), None, h, 1, 1, torch.zeros_like(T(q)), T(g))
    ref = oracle_forward(t, q, qd, act, None, h, 1, 1, debug=True)[2]   # the scalar oracle's first substep
    errs = dict(gq=relerr(project_tangent(t, q, A(dq)), project_tangent(t, q, A(sq) / h)), gact=relerr(A(dact), A(sact) / h))
    fwd = dict(tau=relerr(A(tau), ref["tau"]), qdd=relerr(A(qdd), ref["qdd"]), f_s=relerr(A(fs), ref["f_s"].reshape(N, -1)))
    print(name, "joint dynamics", " ".join("%s %.2e" % kv for kv in list(fwd.items()) + list(errs.items())))
    assert all(e < dyn_lib.CHECK_BOUND for e in errs.values()) and all(e < dyn_lib.FWD_BOUND for e in fwd.values()), (errs, fwd)
    assert kin_lib.radial_part(t, q, A(dq)) <= dyn_lib.RADIAL
    # ground contacts
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    ref = con_lib.forward_batch(t, q64, qd64)
    edge = np.abs(ref[0][:, :, 1]) < con_lib.EDGE
    keep = ~edge.any(axis=1)
    assert keep.sum() >= 3
    rs = np.random.RandomState(11)
    cs = [rs.normal(size=s).astype(np.float32) for s in ((N, Cn, 3), (N, Cn, 3), (N, Cn, 3), (N, L, 6))]
    rq, rqd = con_lib.adjoint_batch(t, q64, qd64, *cs)
    runs = []
    for k in range(4):
        r2 = np.random.RandomState(100 + k)
        q1 = np.nextafter(q, q + r2.choice([-1.0, 1.0], size=q.shape).astype(np.float32)).astype(np.float64)
        qd1 = np.nextafter(qd, qd + r2.choice([-1.0, 1.0], size=qd.shape).astype(np.float32)).astype(np.float64)
        runs.append(con_lib.adjoint_batch(t, q1, qd1, *cs))
    nq_ = np.max([np.abs(project_tangent(t, q, x[0]) - rq).max(axis=1) for x in runs], axis=0) / np.abs(rq).max()
    nqd_ = np.max([np.abs(x[1] - rqd).max(axis=1) for x in runs], axis=0) / np.abs(rqd).max()
    out = eng.ground_contacts_forward(T(q), T(qd))
    gq, gqd = eng.ground_contacts_backward(T(q), T(qd), *[T(x) for x in cs])
    out = [o.cpu().numpy().reshape(r_.shape) for o, r_ in zip(out, ref)]
    fe = [np.abs(out[0] - ref[0]).max() / np.abs(ref[0]).max(), np.abs(out[1] - ref[1]).max() / np.abs(ref[1]).max(),
          np.abs(out[2] - ref[2])[~edge].max() / np.abs(ref[2]).max(), rows_err(out[3], ref[3], keep)]
    eq, eqd = rows_err(project_tangent(t, q, A(gq)), rq, keep), rows_err(A(gqd), rqd, keep)
    print(name, "contacts forward %.2e gq %.2e (bound %.1e) gqd %.2e (bound %.1e)" % (max(fe), eq, grad_bound(nq_[keep]), eqd, grad_bound(nqd_[keep])))
    assert max(fe) < 1e-4 and eq < grad_bound(nq_[keep]) and eqd < grad_bound(nqd_[keep])
    assert kin_lib.radial_part(t, q, A(gq)) <= 1e-6
    # mass matrix
    _, Href, Sref = bm.mass_reference(name, N)
    H, Hinv, S = eng.mass_matrix_forward(T(q))
    rs = np.random.RandomState(11)
    cm = tuple(rs.normal(size=s).astype(np.float32) for s in ((N, nd, nd), (N, nd, nd), (N, nd, 6)))
    gq = A(eng.mass_matrix_backward(T(q), *[T(x) for x in cm]))
    torch.cuda.synchronize()
    eng.status()
    H, Hinv, S = H.cpu().numpy(), Hinv.cpu().numpy(), S.cpu().numpy().reshape(N, nd, 6)
    bound, yard = mass_lib.residual_bound(Href)
    # (the product with the REFERENCE's H is reported, not bounded: it carries cond(H) x the rounding of H on top of the residual)
    res, res_ref = mass_lib.residual(Hinv, H), mass_lib.residual(Hinv, Href)
    hgq = mass_lib.emu_mass_backward(t, q, *cm, static=False, waves=eng.waves)
    eg = relerr(project_tangent(t, q, gq), project_tangent(t, q, hgq))
    print(name, "mass matrix H %.2e S %.2e residual %.2e (bound %.1e; with the reference's H %.2e) adjoint against the host harness %.2e"
          % (relerr(H, Href), relerr(S, Sref), res, bound, res_ref, eg))
    assert relerr(H, Href) < mass_lib.FWD_BOUND and relerr(S, Sref) < mass_lib.FWD_BOUND
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= mass_lib.SYM_BOUND * np.abs(H).max() and res <= bound
    assert eg < 1e-4 and kin_lib.radial_part(t, q, gq) <= mass_lib.RADIAL


def test_lds_limit(models):
    """the model one muscle below the 160 KiB limit is accepted and runs a step (against the oracle); one muscle more is refused
    with DSIM_ERR_LIMIT.  The parameter sweep adds its accumulators to the image: if they take the accepted model beyond the
    limit, dsim_step_backward_params returns DSIM_ERR_LIMIT and dsim_step_backward still works"""
    from diffrl_amd.engine import Engine
    below, above = bm.lds_limit_pair()
    off, d = bm.dims_of(below)
    assert off["total_words"] * 4 <= bm.LIMITS["lds_bytes"] < bm.dims_of(above)[0]["total_words"] * 4
    with pytest.raises(capi.DsimError, match="dsim error -3: model needs more than 160 KiB"):
        Engine(above, DEV)
    eng = Engine(below, DEV)
    assert eng.variant == 0 and eng.waves == 4
    from test_edge_cases_cpu import _tree_states
    n, S, mm = 2, 2, 2
    rng = np.random.default_rng(77)
    q, qd, act = _tree_states(below, rng, n)
    mact = rng.uniform(0.0, 10.0, (n, below.n_muscles)).astype(np.float32)
    gq, gqd = rng.normal(0, 1, q.shape).astype(np.float32), rng.normal(0, 1, qd.shape).astype(np.float32)
    x = (q, qd, act, mact, gq, gqd)
    o = oracle_backward(below, q, qd, act, mact, S / 960.0, S, mm, gq, gqd)
    out = _step(eng, x, S, mm)
    _hold_oracle_bounds(below, x, out, o, S, mm, "below the LDS limit (%d bytes)" % (off["total_words"] * 4))
    par_bytes = (off["total_words"] + 5 * d["nd"] + 4 * d["C"]) * 4
    qo, qdo, ck = eng.forward(T(q), T(qd), T(act), T(mact), S / 960.0, S, mm, True)
    if par_bytes > bm.LIMITS["lds_bytes"]:
        with pytest.raises(capi.DsimError, match="dsim error -3: .*with the parameter accumulators"):
            eng.backward_params(ck, T(act), T(mact), S / 960.0, S, mm, T(gq), T(gqd))
    else:
        r = eng.backward_params(ck, T(act), T(mact), S / 960.0, S, mm, T(gq), T(gqd))
        torch.cuda.synchronize()
        assert np.array_equal(A(r[0], n), out[2])
