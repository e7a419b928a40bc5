"""CPU: the differentiable joint dynamics (dsim_core.hpp: dsim_joint_dyn_forward / dsim_joint_dyn_backward) on the lane-serial
host build of the phase code (tests/emu/dsim_emu_dyn.cpp, compiled by tests/dyn_lib.py), generic and specialised layouts, with
the wavefront count the library picks for the model.

References: the reference simulator's own recordings -- sub_tau / sub_qdd / sub_f_s of tests/golden/<env>_step.npz for the
forward pass (the fixture generator asserts that State.joint_tau / joint_qdd / body_f_s of a one-substep call equal them bit
for bit), tests/golden/<env>_dyn.npz (tools/gen_dynamics_golden.py) for the adjoint and the composite forward pass.

Bounds (tests/dyn_lib.py has the reasoning): forward 1e-4, the project's bound for forces and accelerations of one substep;
every cotangent set in its own max-norm, adjoint 10 x the reference's recorded +-1 ulp noise of that set and tensor, floor 1e-5,
ceiling 1e-3, (state, tensor) pairs whose recorded noise exceeds 3e-4 excluded (at most three, all SNUHumanoid joint_q gradients) but still finite.  Every joint_q gradient
is compared after project_tangent; the own radial part must stay <= 1e-6 of max |gq|.

The cross-check against the step adjoint needs no reference: with one substep of length h, a fresh mass matrix, gq_out = 0 and
gqd_out = g, dsim_step_backward returns gq_in = h (d qdd / d q)^T g and gact = h (d qdd / d act)^T g, so
dsim_joint_dynamics_backward(gqdd = g) must give gq_in / h and gact / h (gqd is left out: it cancels against g).  Both run the
same forward phases, so what differs is the statement of the joint-space adjoint and the order of a few sums: a few ulp of the
largest term.  The bound is 10 x the disagreement measured on this harness (tests/dyn_lib.py: CHECK_MEASURED)."""
import numpy as np
import pytest

import dyn_lib as D
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import golden, project_tangent, relerr, template_from_golden
from kin_lib import radial_part

VARIANTS = [(False, "generic"), (True, "specialised")]
CHECK_BOUND, CHECK_H = D.CHECK_BOUND, D.CHECK_H


def _case(name):
    t = template_from_golden(name)
    return t, golden(name + "_step"), golden(name + "_dyn"), D.waves_of(t)


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", D.ENVS)
def test_forward_matches_the_reference_recordings(name, static, label):
    t, g, dyn, waves = _case(name)
    q, qd, act, mact, muscles = D.inputs(g)
    B, L = q.shape[0], t.n_links
    tau, qdd, fs = D.emu_dyn_forward(t, q, qd, act, mact, static, waves)
    errs = dict(tau=relerr(tau, g["sub_tau"]), qdd=relerr(qdd, g["sub_qdd"]), f_s=relerr(fs, g["sub_f_s"].reshape(B, L, 6)))
    print(name, label, "waves", waves, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert all(e < D.FWD_BOUND for e in errs.values()), errs
    # NULL act / muscle_act are zeros
    z = D.emu_dyn_forward(t, q, qd, np.zeros_like(act), np.zeros_like(mact) if muscles else None, static, waves)
    n = D.emu_dyn_forward(t, q, qd, None, None, static, waves)
    assert all(np.array_equal(a, b) for a, b in zip(z, n))


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", D.ENVS)
def test_adjoint_matches_the_reference_tape_adjoint(name, static, label):
    t, g, dyn, waves = _case(name)
    q, qd, act, mact, muscles = D.inputs(g)
    plan, excluded = D.adjoint_plan(name, dyn, muscles)
    print(name, label, "excluded ((state, tensor), (sets, largest recorded noise)):", excluded)
    atag = "gmact" if muscles else "gact"
    zeros = (np.zeros_like(dyn["c_tau"]), np.zeros_like(dyn["c_qdd"]), np.zeros_like(dyn["c_fs"]))
    for tag in D.COTANGENTS:
        c = D.cotangents(dyn, tag)
        gq, gqd, gact, gmact = D.emu_dyn_backward(t, q, qd, act, mact, *c, static=static, waves=waves)
        got = dict(gq=project_tangent(t, q, gq), gqd=gqd)
        got[atag] = gmact if muscles else gact
        ref = dict(gq=project_tangent(t, q, dyn["gq_" + tag]), gqd=dyn["gqd_" + tag])
        ref[atag] = dyn[atag + "_" + tag]
        assert all(np.isfinite(v).all() for v in (gq, gqd, gact)) and (gmact is None or np.isfinite(gmact).all())
        rad = radial_part(t, q, gq)
        for k in got:
            rows, bound, noise = plan[(tag, k)]
            e = D.rows_err(got[k], ref[k], rows)
            print("%s %s cotangent %-3s %-5s err %.2e  reference noise %.2e  bound %.1e" % (name, label, tag, k, e, noise, bound))
            assert e < bound, (tag, k, e, bound)
        assert rad <= D.RADIAL, (tag, rad)
        # a NULL cotangent is a zero cotangent
        full = tuple(x if x is not None else z for x, z in zip(c, zeros))
        again = D.emu_dyn_backward(t, q, qd, act, mact, *full, static=static, waves=waves)
        assert np.array_equal(gq, again[0]) and np.array_equal(gqd, again[1]) and np.array_equal(gact, again[2])


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", D.ENVS)
def test_composite_forward_matches_the_reference(name, static, label):
    """the read-out of the state a whole env-step ends in (the reference's q_out / qd_out), against comp_tau / comp_qdd / comp_f_s"""
    t, g, dyn, waves = _case(name)
    _, _, act, mact, muscles = D.inputs(g)
    B = act.shape[0]
    tau, qdd, fs = D.emu_dyn_forward(t, g["q_out"], g["qd_out"], act, mact, static, waves)
    for k, a in (("tau", tau), ("qdd", qdd), ("f_s", fs)):
        e, bound = relerr(a.reshape(B, -1), dyn["comp_" + k].reshape(B, -1)), D.composite_bound(dyn, k, 1e-4)
        print(name, label, "composite", k, "%.2e bound %.1e" % (e, bound))
        assert e < bound, (k, e, bound)


def _check(t, q, qd, act, mact, static, waves, user=False, seed=5):
    g = np.random.default_rng(seed).normal(size=qd.shape).astype(np.float32)
    gq, _, gact, gmact = D.emu_dyn_backward(t, q, qd, act, mact, None, g, None, static=static, waves=waves, user=user)
    sq, sact, smact = D.emu_step_adjoint(t, q, qd, act, mact, CHECK_H, g, static=static, waves=waves, user=user)
    errs = dict(gq=relerr(project_tangent(t, q, gq), project_tangent(t, q, sq / CHECK_H)))
    if t.n_muscles:
        errs["gmact"] = relerr(gmact, smact / CHECK_H)
    else:
        errs["gact"] = relerr(gact, sact / CHECK_H)
    return errs


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("name", D.ENVS)
def test_qdd_adjoint_equals_the_step_adjoint_of_one_substep(name, static, label):
    t, g, dyn, waves = _case(name)
    q, qd, act, mact, _ = D.inputs(g)
    errs = _check(t, q, qd, act, mact, static, waves)
    print(name, label, "vs step adjoint / h:", " ".join("%s %.2e" % kv for kv in errs.items()), "bound %.1e" % CHECK_BOUND)
    assert all(e < CHECK_BOUND for e in errs.values()), errs


@pytest.mark.parametrize("static,label", VARIANTS)
@pytest.mark.parametrize("tag,path", D.USER_MODELS)
def test_user_models_agree_with_the_step_adjoint(tag, path, static, label):
    """free, hinge, prismatic and ball joints, CSR-list subtrees (user_tree) and a 17-link row tree (user_rowtree)"""
    from test_edge_cases_cpu import _tree_states
    t = ArticulationTemplate.load(path)
    q, qd, act = _tree_states(t, np.random.default_rng(17), 6)
    tau, qdd, fs = D.emu_dyn_forward(t, q, qd, act, None, static, 1, user=True)
    assert np.isfinite(tau).all() and np.isfinite(qdd).all() and np.isfinite(fs).all()
    gen = D.emu_dyn_forward(t, q, qd, act, None, False, 1, user=True)
    assert max(relerr(a, b) for a, b in zip((tau, qdd, fs), gen)) < D.FWD_BOUND
    errs = _check(t, q, qd, act, None, static, 1, user=True)
    gq = D.emu_dyn_backward(t, q, qd, act, None, None, None, np.ones_like(fs), static=static, waves=1, user=True)[0]
    print(tag, label, "vs step adjoint / h:", " ".join("%s %.2e" % kv for kv in errs.items()), "radial %.1e" % radial_part(t, q, gq))
    assert all(e < CHECK_BOUND for e in errs.values()), errs
    assert radial_part(t, q, gq) <= D.RADIAL
