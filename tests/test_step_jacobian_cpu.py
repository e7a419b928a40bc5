"""CPU: the step Jacobian on the lane-serial host build (tests/emu/dsim_emu_jac.cpp, compiled by tests/jac_lib.py): the block
mapping of dsim_step_backward_multi / dsim_step_jacobian (dsim_core.hpp: dsim_multi_slot) around the unchanged step adjoint,
generic and specialised layouts, with the wavefront count the library picks for the model.

1. The multi sweep over all (environment, cotangent) blocks equals single sweeps bit for bit -- random cotangents, shared and
   per environment, and the Jacobian call against its identity seeds.
2. The host Jacobian against tests/golden/<env>_lin.npz (tools/gen_linearise_golden.py): every block in its own max-norm, q_in
   columns after project_tangent, bound 1e-3; tests/jac_lib.py states the exclusion rule and what the recordings put under it.
3. The binding names both calls and expects ABI 110.
"""
import numpy as np
import pytest

import jac_lib as J
from diffrl_amd import capi

VARIANTS = [(False, "generic"), (True, "specialised")]
_fwd = {}


def _ckpt(name, static):
    """forward pass of the recorded states on the harness, once per (model, variant)"""
    if (name, static) not in _fwd:
        t, inp, lin = J.case(name)
        waves = J.waves_of(t)
        qo, qdo, ck = J.emu_forward(t, inp["q"], inp["qd"], inp["act"], inp["mact"], inp["dt"], inp["S"], inp["mm"], static, waves)
        ck.setflags(write=False)
        _fwd[(name, static)] = (waves, ck)
    return _fwd[(name, static)]


def _eq(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", J.ENVS)
def test_multi_sweep_equals_single_sweeps_bit_for_bit(name, static, label):
    t, inp, lin = J.case(name)
    waves, ck = _ckpt(name, static)
    N, K = ck.shape[0], 3
    a = (inp["act"], inp["mact"], inp["dt"], inp["S"], inp["mm"])
    rng = np.random.default_rng(31)
    gq = rng.normal(size=(N, K, t.n_q)).astype(np.float32)
    gqd = rng.normal(size=(N, K, t.n_qd)).astype(np.float32)
    singles = [J.emu_backward(t, ck, *a, gq[:, k], gqd[:, k], static, waves) for k in range(K)]
    want = tuple(np.stack([s[j] for s in singles], axis=1) if singles[0][j] is not None else None for j in range(4))
    got = J.emu_backward_multi(t, ck, *a, gq, gqd, False, static, waves)
    assert all(g is None or np.isfinite(g).all() for g in got)
    assert _eq(got, want), "per-environment cotangents"
    # one shared set: every environment gets environment 0's cotangents
    singles = [J.emu_backward(t, ck, *a, np.repeat(gq[:1, k], N, 0), np.repeat(gqd[:1, k], N, 0), static, waves) for k in range(K)]
    want = tuple(np.stack([s[j] for s in singles], axis=1) if singles[0][j] is not None else None for j in range(4))
    assert _eq(J.emu_backward_multi(t, ck, *a, gq[0], gqd[0], True, static, waves), want), "shared cotangents"


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", J.ENVS)
def test_jacobian_equals_single_sweeps_and_matches_the_reference(name, static, label):
    t, inp, lin = J.case(name)
    waves, ck = _ckpt(name, static)
    N, nq, nd = ck.shape[0], t.n_q, t.n_qd
    K = nq + nd
    a = (inp["act"], inp["mact"], inp["dt"], inp["S"], inp["mm"])
    Js, Ja, Jm = J.emu_jacobian(t, ck, *a, static, waves)
    # item 1: row k is the single sweep seeded with e_k -- ALL (environment, cotangent) pairs, excluded blocks included
    eye = np.eye(K, dtype=np.float32)
    for k in range(K):
        gq, gqd, ga, gm = J.emu_backward(t, ck, *a, np.repeat(eye[k:k + 1, :nq], N, 0), np.repeat(eye[k:k + 1, nq:], N, 0), static, waves)
        assert np.array_equal(Js[:, k, :nq], gq) and np.array_equal(Js[:, k, nq:], gqd) and np.array_equal(Ja[:, k], ga), k
        assert gm is None or np.array_equal(Jm[:, k], gm), k
    # item 2: the reference's recording
    J.compare(name, label, t, inp["q"], lin, Js, Ja, Jm)
    rad = J.radial(t, inp["q"], Js[:, :, :nq])
    print(name, label, "radial part of the q_in columns %.2e" % rad)
    assert rad <= J.RADIAL


@pytest.mark.parametrize("name", J.ENVS)
def test_at_most_one_block_is_excluded(name):
    lin = J.case(name)[2]
    skip = J.excluded_blocks(lin)
    print(name, "excluded:", skip, {k: float(lin["noise_" + k]) for k in J.BLOCKS if k in lin})
    assert len(skip) <= J.MAX_EXCLUDED


def test_lean_checkpoints_give_the_same_mapping():
    """the lean adjoint recomputes the forward phases: the block mapping must not care"""
    t, inp, lin = J.case("ant")
    a = (inp["act"], inp["mact"], inp["dt"], inp["S"], inp["mm"])
    ck = J.emu_forward(t, inp["q"], inp["qd"], *a, True, 1, lean=True)[2]
    rng = np.random.default_rng(3)
    gq, gqd = rng.normal(size=(2, t.n_q)).astype(np.float32), rng.normal(size=(2, t.n_qd)).astype(np.float32)
    got = J.emu_backward_multi(t, ck, *a, gq, gqd, True, True, 1, lean=True)
    for k in range(2):
        one = J.emu_backward(t, ck, *a, np.repeat(gq[k:k + 1], ck.shape[0], 0), np.repeat(gqd[k:k + 1], ck.shape[0], 0), True, 1, lean=True)
        assert all(np.array_equal(g[:, k], o) for g, o in zip(got[:3], one[:3]))


@pytest.mark.parametrize("static,label", VARIANTS[1:])   # (the generic layout at these schedules: tests/test_emu_phases.py)
@pytest.mark.parametrize("mm", [3, 2])
@pytest.mark.parametrize("name", J.ENVS)
def test_multi_sweep_equals_single_sweeps_at_uneven_mass_matrix_groups(name, mm, static, label):
    """the block mapping at S = 7 with groups 3,3,1 and 2,2,2,1 (tests/mm_sched.py): every block reads the inverse of each group and
    the tail of the ONE checkpoint at the offsets of that schedule -- K = 3 shared cotangent pairs against three single sweeps, bit for bit"""
    import mm_sched as M
    c = M.case(name)
    t, waves = c["t"], J.waves_of(c["t"])
    a = (c["act"], c["mact"], M.DT, M.S, mm)
    qo, qdo, ck = J.emu_forward(t, c["q"], c["qd"], *a, static, waves)
    rng = np.random.default_rng(31)
    N, K = 2, 3          # (two environments: the block mapping has an environment stride to get wrong, the harness is lane-serial)
    gq, gqd = rng.normal(size=(K, t.n_q)).astype(np.float32), rng.normal(size=(K, t.n_qd)).astype(np.float32)
    b = (c["act"][:N], c["mact"][:N] if c["mact"] is not None else None, M.DT, M.S, mm)
    singles = [J.emu_backward(t, ck[:N], *b, np.repeat(gq[k:k + 1], N, 0), np.repeat(gqd[k:k + 1], N, 0), static, waves) for k in range(K)]
    want = tuple(np.stack([s[j] for s in singles], axis=1) if singles[0][j] is not None else None for j in range(4))
    got = J.emu_backward_multi(t, ck[:N], *b, gq, gqd, True, static, waves)
    assert all(g is None or np.isfinite(g).all() for g in got)
    assert _eq(got, want)
    # and the sweep is the adjoint of this schedule, not only consistent with itself: all six states against the oracle
    one = J.emu_backward(t, ck, *a, c["gq"], c["gqd"], static, waves)
    M.assert_step(name, mm, dict(q=qo, qd=qdo, gq=one[0], gqd=one[1], gact=one[2], gmact=one[3]), label="host " + label)


def test_binding_names_both_calls():
    assert "dsim_step_backward_multi" in capi.EXPORTS and "dsim_step_jacobian" in capi.EXPORTS
    assert capi.EXPECTED_ABI == 110
