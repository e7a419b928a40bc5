"""CPU: the differentiable mass matrix read-out (dsim_core.hpp: dsim_mass_forward / dsim_mass_backward) on the lane-serial host
build of the phase code (tests/emu/dsim_emu_mass.cpp, compiled by tests/mass_lib.py), generic and specialised layouts, one and
four wavefronts per environment, and the two user models.

References: sub_H + diag(joint_armature) and sub_S_s of tests/golden/<env>_step.npz (the reference simulator's model.H and
State.joint_S_s of q_in, which tools/gen_mass_golden.py asserts its own run reproduces bit for bit), and the gradients of
tests/golden/<env>_mass.npz, the reference's own tape replay from cotangents on those two tensors (a cotangent on Hinv carried to
model.H by the rule of the inverse in float64).

Bounds: S and H 1e-5 in the tensor's max-norm, |H - H^T| <= 1e-6 max |H|; the inverse by its residual max |Hinv H - I| (float64
product of the two fp32 tensors) against 10 x the residual of the float32 restatement of the elimination in tests/mass_lib.py on the
reference's matrix, floor 1e-6 (a direct comparison with an inverse of the reference's H would test the conditioning of H: 1e-6 of
H moves the float64 inverse of Humanoid's by 5e-3); every cotangent set in its own max-norm after project_tangent, 10 x the set's
recorded +-1 ulp noise of the reference, floor 1e-4, ceiling 1e-3, no state or set excluded; own radial part <= 1e-6 of max |gq|.
Measured on the host harness (profiles/mass_matrix_kernels.txt has the table): no (model, set) pair of the reference's noise
passes 3e-4 at K = 8.
"""
import itertools
import os
import re

import numpy as np
import pytest

import dyn_lib
import kin_lib
import mass_lib as M
from diffrl_amd import capi
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import golden, project_tangent, relerr, template_from_golden

VARIANTS = [(False, 1, "generic-1w"), (False, 4, "generic-4w"), (True, 1, "specialised-1w"), (True, 4, "specialised-4w")]
_cache, _fwd = {}, {}


def _case(name):
    if name not in _cache:
        _cache[name] = (template_from_golden(name), golden(name + "_step"), golden(name + "_mass"))
    return _cache[name]


def _forward(name, static, waves):
    """the fixture batch's read-out, computed once per kernel variant and left unchanged"""
    key = (name, static, waves)
    if key not in _fwd:
        t, step, _ = _case(name)
        _fwd[key] = M.emu_mass_forward(t, step["q_in"], static, waves)
        for o in _fwd[key]:
            o.setflags(write=False)
    return _fwd[key]


@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", M.ENVS)
def test_forward_matches_the_reference(name, static, waves, label):
    t, step, _ = _case(name)
    H, Hinv, S = _forward(name, static, waves)
    assert all(np.isfinite(o).all() for o in (H, Hinv, S))   # every word written (the buffers start as NaN)
    eS, eH = relerr(S, M.reference_S(t, step)), relerr(H, M.reference_H(t, step))
    sym = float(np.abs(H - H.transpose(0, 2, 1)).max() / np.abs(H).max())
    print("%s %s forward S %.2e H %.2e (bound %.0e)  |H - H^T| %.2e (bound %.0e)" % (name, label, eS, eH, M.FWD_BOUND, sym, M.SYM_BOUND))
    assert eS < M.FWD_BOUND and eH < M.FWD_BOUND, (eS, eH)
    assert sym <= M.SYM_BOUND, sym


@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", M.ENVS)
def test_inverse_by_its_residual(name, static, waves, label):
    t, step, _ = _case(name)
    H, Hinv, _ = _forward(name, static, waves)
    bound, yard = M.residual_bound(M.reference_H(t, step))
    r = M.residual(Hinv, H)
    print("%s %s residual max |Hinv H - I| %.2e  float32 restatement %.2e  bound %.1e" % (name, label, r, yard, bound))
    assert r <= bound, (r, bound)


@pytest.mark.parametrize("name", M.ENVS)
def test_consistent_with_the_shipped_readouts(name):
    """qdd of the dynamic read-out is Hinv tau, v_s of the kinematic read-out is the masked sum of S_d qd_d"""
    t, step, _ = _case(name)
    q, qd, act, mact, _ = dyn_lib.inputs(step)
    waves = kin_lib.waves_of(t)
    for static in (False, True):
        _, Hinv, S = _forward(name, static, waves)
        tau, qdd, _ = dyn_lib.emu_dyn_forward(t, q, qd, act, mact, static, waves)
        ref = np.einsum("bij,bj->bi", Hinv.astype(np.float64), tau.astype(np.float64))
        assert (np.abs(qdd - ref) <= M.dot_bound(Hinv, tau)).all(), float(np.abs(qdd - ref).max())
        vs = kin_lib.emu_kin_forward(t, q, qd, static, waves)[2]
        mask = M.link_dof_mask(t).astype(np.float64)
        ref = np.einsum("id,bdk,bd->bik", mask, S.astype(np.float64), qd.astype(np.float64))
        e = float(np.abs(vs - ref).max() / np.abs(vs).max())
        print("%s static=%s v_s against mask S qd %.2e" % (name, static, e))
        assert e < 1e-5, e


@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", M.ENVS)
def test_adjoint_matches_the_reference(name, static, waves, label):
    t, step, m = _case(name)
    q = step["q_in"]
    for tag in M.SETS:
        gq = M.emu_mass_backward(t, q, *M.cotangents(m, tag), static=static, waves=waves)
        assert np.isfinite(gq).all()
        noise = m["noise_gq_" + tag]
        e, bound = relerr(project_tangent(t, q, gq), project_tangent(t, q, m["gq_" + tag])), M.grad_bound(noise)
        print("%s %s cotangent %-4s err %.2e  reference noise %.2e  bound %.1e" % (name, label, tag, e, noise.max(), bound))
        assert e < bound, (tag, e, bound)
        rad = kin_lib.radial_part(t, q, gq)
        assert rad <= M.RADIAL, (tag, rad)


@pytest.mark.parametrize("name", M.ENVS)
def test_bit_for_bit_properties(name):
    """rows of N = 1 and N = 3 are the batch's rows; an output not asked for changes no other output (Hinv alone included); a
    NULL cotangent is a zero cotangent"""
    t, step, m = _case(name)
    q = step["q_in"]
    waves = kin_lib.waves_of(t)
    for static in (False, True):
        full = _forward(name, static, waves)
        gfull = M.emu_mass_backward(t, q, *M.cotangents(m, "all"), static=static, waves=waves)
        for rows in (slice(1, 2), slice(2, 5)):
            for a, b in zip(M.emu_mass_forward(t, q[rows], static, waves), full):
                assert np.array_equal(a, b[rows])
            assert np.array_equal(M.emu_mass_backward(t, q[rows], *M.cotangents(m, "all", rows), static=static, waves=waves), gfull[rows])
        q3, cs = q[:3], M.cotangents(m, "all", slice(0, 3))
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            out = M.emu_mass_forward(t, q3, static, waves, want=want)
            for w, a, b in zip(want, out, full):
                assert (a is None) if not w else np.array_equal(a, b[:3]), want
        for have in itertools.product((False, True), repeat=3):
            a = M.emu_mass_backward(t, q3, *[c if h else None for c, h in zip(cs, have)], static=static, waves=waves)
            b = M.emu_mass_backward(t, q3, *[c if h else np.zeros_like(c) for c, h in zip(cs, have)], static=static, waves=waves)
            assert np.array_equal(a, b), have
            if not any(have):
                assert not a.any()


def _hinge_coords(t):
    return [int(t.joint_q_start[i]) for i in range(t.n_links) if int(t.joint_type[i]) in (0, 1)]


def _fd_check(t, q, cs, coords, what, **kw):
    """central differences of the harness's own float32 forward (step 1e-2, the loss summed in float64) against the adjoint, on the
    given coordinates, relative to the largest of those gradient entries."""
    def loss(qv):
        out = M.emu_mass_forward(t, qv, **kw)
        return sum((o.astype(np.float64) * c).reshape(len(qv), -1).sum(axis=1) for o, c in zip(out, cs) if c is not None)
    gq = M.emu_mass_backward(t, q, *cs, **kw).astype(np.float64)
    fd = np.zeros((len(q), len(coords)))
    for n, k in enumerate(coords):
        qp, qm = q.copy(), q.copy()
        qp[:, k] += np.float32(M.FD_STEP)
        qm[:, k] -= np.float32(M.FD_STEP)
        fd[:, n] = (loss(qp) - loss(qm)) / (qp[:, k].astype(np.float64) - qm[:, k])
    e = float(np.abs(fd - gq[:, coords]).max() / np.abs(gq[:, coords]).max())
    print("%s central differences against the adjoint %.2e (bound %.0e)" % (what, e, M.FD_BOUND))
    assert e < M.FD_BOUND, e


@pytest.mark.parametrize("static", (False, True))
@pytest.mark.parametrize("name", ("cartpole", "hopper"))
def test_adjoint_equals_central_differences_on_the_hinges(name, static):
    t, step, m = _case(name)
    _fd_check(t, step["q_in"].copy(), M.cotangents(m, "all"), _hinge_coords(t), "%s static=%s" % (name, static), static=static, waves=1)


@pytest.mark.parametrize("tag,path", kin_lib.USER_MODELS)
def test_user_models(tag, path):
    """free, hinge, prismatic and ball joints, CSR-list subtrees (user_tree) and a 17-link row tree (user_rowtree): no recording,
    so the generic kernels (held to the reference on the six models above) are the reference of the specialised ones, H is
    symmetric, the inverse meets the residual bound of its own H, the read-outs agree, and the adjoint meets central differences"""
    from test_edge_cases_cpu import _tree_states
    t = ArticulationTemplate.load(path)
    q, qd, _ = _tree_states(t, np.random.default_rng(17), 6)
    q, qd = q.astype(np.float32), qd.astype(np.float32)
    gen = M.emu_mass_forward(t, q, False, 1, user=True)
    spe = M.emu_mass_forward(t, q, True, 1, user=True)
    for a, b, k in zip(spe[::2], gen[::2], ("H", "S")):
        e = relerr(a, b)
        print(tag, "specialised against generic", k, "%.2e" % e)
        assert e < M.FWD_BOUND, (k, e)
    rs = np.random.RandomState(11)
    B, nd = len(q), t.n_qd
    cs = tuple(rs.normal(size=s).astype(np.float32) for s in ((B, nd, nd), (B, nd, nd), (B, nd, 6)))
    mask = M.link_dof_mask(t).astype(np.float64)
    act = np.zeros_like(qd)
    mact = np.zeros((B, t.n_muscles), np.float32) if t.n_muscles else None
    for static, (H, Hinv, S) in ((False, gen), (True, spe)):
        assert np.abs(H - H.transpose(0, 2, 1)).max() <= M.SYM_BOUND * np.abs(H).max()
        bound, yard = M.residual_bound(H)
        r = M.residual(Hinv, H)
        print("%s static=%s residual %.2e restatement %.2e bound %.1e" % (tag, static, r, yard, bound))
        assert r <= bound, (r, bound)
        tau, qdd, _ = dyn_lib.emu_dyn_forward(t, q, qd, act, mact, static, 1, user=True)
        ref = np.einsum("bij,bj->bi", Hinv.astype(np.float64), tau.astype(np.float64))
        assert (np.abs(qdd - ref) <= M.dot_bound(Hinv, tau)).all()
        vs = kin_lib.emu_kin_forward(t, q, qd, static, 1, user=True)[2]
        ref = np.einsum("id,bdk,bd->bik", mask, S.astype(np.float64), qd.astype(np.float64))
        assert np.abs(vs - ref).max() < 1e-5 * np.abs(vs).max()
        gq = M.emu_mass_backward(t, q, *cs, static=static, waves=1, user=True)
        assert kin_lib.radial_part(t, q, gq) <= M.RADIAL
        # the adjoint: H and S against central differences; Hinv (whose fp32 forward is too rough to difference: its rounding
        # error over the step exceeds 1e-3 of the gradient here) by the rule of the inverse -- a cotangent G on Hinv is the
        # cotangent -Hinv^T G Hinv^T on H, formed in float64 from the kernel's own Hinv -- to the floor of the gradient bounds
        _fd_check(t, q.copy(), (cs[0], None, cs[2]), _hinge_coords(t), "%s static=%s" % (tag, static), static=static, waves=1, user=True)
        Hi = Hinv.astype(np.float64)
        W = -np.einsum("bki,bkl,bjl->bij", Hi, cs[1].astype(np.float64), Hi)
        ga = M.emu_mass_backward(t, q, None, cs[1], None, static=static, waves=1, user=True)
        gb = M.emu_mass_backward(t, q, W, None, None, static=static, waves=1, user=True)
        e = relerr(project_tangent(t, q, ga), project_tangent(t, q, gb))
        print("%s static=%s cotangent on Hinv against its image on H %.2e" % (tag, static, e))
        assert e < 1e-4, e
    ga = M.emu_mass_backward(t, q, *cs, static=False, waves=1, user=True)
    gb = M.emu_mass_backward(t, q, *cs, static=True, waves=1, user=True)
    e = relerr(project_tangent(t, q, gb), project_tangent(t, q, ga))
    print(tag, "adjoint, specialised against generic %.2e" % e)
    assert e < 1e-4, e


def test_the_two_functions_are_exported_and_the_abi_number_stays():
    hdr = open(os.path.join(M.ROOT, "include", "dsim.h")).read()
    for fn in ("dsim_mass_matrix", "dsim_mass_matrix_backward"):
        assert fn in capi.EXPORTS and re.search(r"\bint %s\(" % fn, hdr)
    assert len(capi.ABI["dsim_mass_matrix"][1]) == 7 and len(capi.ABI["dsim_mass_matrix_backward"][1]) == 8
    assert capi.EXPECTED_ABI == 110
