"""CPU: the step adjoint with model-parameter gradients (dsim_core.hpp: DsimParCtxT around dsim_sim_step_backward, the code of
dsim_bwd_param_kernel) on the lane-serial host build of the phase code (dsim_emu_step_backward of tests/emu/dsim_emu.cpp through
tests/par_lib.py): all six models, generic and specialised layouts, one and four wavefronts per environment, full and lean checkpoints.

Reference: tests/golden/<env>_par.npz, the reference simulator's own tape replay of three substeps (mass matrix refreshed on
substeps 0 and 2) with requires_grad on its model tensors (tools/gen_param_golden.py); the library runs the same step as
dt = 3 h, substeps = 3, mm_freq = 2.

Bounds: q_out / qd_out 1e-4 and the state gradients 1e-3 in the tensor's max-norm (gq after project_tangent), as in the step
tests; every parameter gradient tensor, folded to the reference's shapes (dofs -> links, hinge dofs -> coordinates, contact
slots -> shapes), in its own max-norm against 10 x its recorded +-1 ulp noise of the reference, floor 1e-4, ceiling 1e-3, nothing
excluded.  The state gradients of the parameter sweep equal the plain sweep's bit for bit.
"""
import numpy as np
import pytest

import par_lib as P
from oracle_lib import project_tangent, relerr

VARIANTS = [(False, 1, "generic-1w"), (False, 4, "generic-4w"), (True, 1, "specialised-1w"), (True, 4, "specialised-4w")]
MODES = [(False, "full"), (True, "lean")]
_runs = {}


def _run(name, static, waves, lean):
    """the fixture batch through forward, the parameter sweep and the plain sweep: once per kernel variant, left unchanged"""
    key = (name, static, waves, lean)
    if key not in _runs:
        t, g, (act, mact) = P.case(name)
        dt, S, mm = float(g["dt"]), int(g["substeps"]), int(g["mm_freq"])
        kw = dict(static=static, waves=waves, lean=lean)
        qo, qdo, ck = P.emu_par_forward(t, g["q_in"], g["qd_in"], act, mact, dt, S, mm, **kw)
        par = P.emu_par_backward(t, ck, act, mact, dt, S, mm, g["gq_out"], g["gqd_out"], **kw)
        plain = P.emu_par_backward(t, ck, act, mact, dt, S, mm, g["gq_out"], g["gqd_out"], want=(False, False), **kw)
        for a in [qo, qdo, ck] + [v for r in (par, plain) for v in r.values() if v is not None]:
            a.setflags(write=False)
        _runs[key] = (qo, qdo, ck, par, plain)
    return _runs[key]


@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_state_outputs_match_the_reference(name, static, waves, label, lean, mode):
    t, g, _ = P.case(name)
    qo, qdo, _, par, _ = _run(name, static, waves, lean)
    tang = lambda x: project_tangent(t, g["q_in"], x)  # noqa: E731
    ga_ref, ga = (g["gmuscle_act"], par["gmact"]) if t.n_muscles else (g["gact"], par["gact"])
    e = dict(q=relerr(qo, g["q_out"]), qd=relerr(qdo, g["qd_out"]), gq=relerr(tang(par["gq"]), tang(g["gq_in"])),
             gqd=relerr(par["gqd"], g["gqd_in"]), gact=relerr(ga, ga_ref))
    print("%s %s %s " % (name, label, mode) + " ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < P.STATE_BOUND and e["qd"] < P.STATE_BOUND, e
    assert e["gq"] < P.GRAD_BOUND and e["gqd"] < P.GRAD_BOUND and e["gact"] < P.GRAD_BOUND, e


@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_joint_parameter_gradients_match_the_reference(name, static, waves, label, lean, mode):
    t, g, _ = P.case(name)
    par = _run(name, static, waves, lean)[3]
    assert np.isfinite(par["g_dof"]).all()   # every word written (the buffer starts as NaN)
    f = P.fold(t, name, par["g_dof"], None)
    for k in P.PARAM_TENSORS[:5]:
        if "noise_" + k in g:
            err, bound = relerr(f[k], g[k]), P.param_bound(g["noise_" + k])
            print("%s %s %s %s err %.2e  reference noise %.1e  bound %.1e" % (name, label, mode, k, err, float(g["noise_" + k]), bound))
            assert err <= bound, (k, err, bound)
        else:   # the reference records an all-zero tensor (e.g. joint_target where every target_ke is 0): so do we
            assert not np.asarray(g[k]).any() and not f[k].any(), k


@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", [n for n in P.ENVS if n != "cartpole"])
def test_contact_parameter_gradients_match_the_reference(name, static, waves, label, lean, mode):
    t, g, _ = P.case(name)
    par = _run(name, static, waves, lean)[3]
    assert np.isfinite(par["g_contact"]).all()
    f = P.fold(t, name, None, par["g_contact"])["g_shape_materials"]
    err, bound = relerr(f, g["g_shape_materials"]), P.param_bound(g["noise_g_shape_materials"])
    print("%s %s %s shape_materials err %.2e  reference noise %.1e  bound %.1e" % (name, label, mode, err,
                                                                                  float(g["noise_g_shape_materials"]), bound))
    assert err <= bound, (err, bound)
    # every column (ke, kd, kf, mu) on its own scale too, by its own recorded noise: a wrong rule in one cannot hide behind another
    for j, col in enumerate(("ke", "kd", "kf", "mu")):
        ej, bj = relerr(f[..., j], g["g_shape_materials"][..., j]), P.param_bound(g["noise_g_shape_materials_cols"][j])
        print("%s %s %s shape_materials.%s err %.2e  bound %.1e" % (name, label, mode, col, ej, bj))
        assert ej <= bj, (col, ej, bj)
    # a contact that never penetrates in the three substeps has no gradient at all
    dead = ~np.asarray(g["br_active"]).any(axis=1)
    assert not par["g_contact"][dead].any()


@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_state_gradients_equal_the_plain_sweep_bit_for_bit(name, static, waves, label, lean, mode):
    par, plain = _run(name, static, waves, lean)[3:]
    for k in ("gq", "gqd", "gact", "gmact"):
        if plain[k] is not None:
            assert np.array_equal(par[k], plain[k]), k


@pytest.mark.parametrize("name", P.ENVS)
def test_null_patterns(name):
    """g_dof only, g_contact only, gact / gmuscle_act NULL: what is returned does not change"""
    t, g, (act, mact) = P.case(name)
    dt, S, mm = float(g["dt"]), int(g["substeps"]), int(g["mm_freq"])
    _, _, ck, full, _ = _run(name, False, 1, False)
    args = (t, ck, act, mact, dt, S, mm, g["gq_out"], g["gqd_out"])
    a = P.emu_par_backward(*args, want=(True, False))
    assert a["g_contact"] is None and np.array_equal(a["g_dof"], full["g_dof"]) and np.array_equal(a["gq"], full["gq"])
    b = P.emu_par_backward(*args, want=(False, True)) if t.n_contacts else None
    if b is not None:
        assert b["g_dof"] is None and np.array_equal(b["g_contact"], full["g_contact"]) and np.array_equal(b["gqd"], full["gqd"])
    c = P.emu_par_backward(*args, want_act=False)
    assert c["gact"] is None and c["gmact"] is None
    assert np.array_equal(c["g_dof"], full["g_dof"]) and np.array_equal(c["g_contact"], full["g_contact"])
    assert np.array_equal(c["gq"], full["gq"]) and np.array_equal(c["gqd"], full["gqd"])


@pytest.mark.parametrize("static,label", [(False, "generic"), (True, "specialised")])
@pytest.mark.parametrize("name", P.ENVS)
def test_set_params_equals_a_model_created_with_the_values(name, static, label):
    """values copied into the constant block give the bits of a model built from a template that holds them; without them
    the original bits are back"""
    t, g, (act, mact) = P.case(name)
    dt, S, mm = float(g["dt"]), int(g["substeps"]), int(g["mm_freq"])
    p = P.perturbed_params(t)
    run = lambda tt, pp: P.emu_par_forward(tt, g["q_in"], g["qd_in"], act, mact, dt, S, mm, params=pp, static=static)  # noqa: E731
    base = _run(name, static, 1, False)
    a, b = run(t, p), run(P.with_params(t, p), None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[1], base[1])   # the values matter
    c = run(t, None)
    assert np.array_equal(c[0], base[0]) and np.array_equal(c[1], base[1]) and np.array_equal(c[2], base[2])
    # ... and the parameter sweep under the set values equals that of the model created with them
    ga = P.emu_par_backward(t, a[2], act, mact, dt, S, mm, g["gq_out"], g["gqd_out"], params=p, static=static)
    gb = P.emu_par_backward(P.with_params(t, p), b[2], act, mact, dt, S, mm, g["gq_out"], g["gqd_out"], static=static)
    assert all(np.array_equal(ga[k], gb[k]) for k in ga if ga[k] is not None)


def test_fixtures_cover_every_rule():
    """what tools/gen_param_golden.py asserts when it records, held against the committed files"""
    for name in P.ENVS:
        t, g, _ = P.case(name)
        if t.n_contacts:
            act = np.asarray(g["br_active"])
            first, vneg = np.asarray(g["br_first"]), np.asarray(g["br_vn_neg"])
            assert first.any() and (act & ~first).any() and vneg.any() and (act & ~vneg).any(), name
            assert all(np.abs(g["g_shape_materials"][..., j]).max() > 0 for j in range(4)), name
        if g["limit_state"].any():
            assert np.asarray(g["br_low"]).any() and np.asarray(g["br_up"]).any(), name
            assert np.abs(g["g_limit_ke"]).max() > 0
    assert sum(bool(P.golden(n + "_par")["limit_state"].any()) for n in P.ENVS) >= 4
    assert sum(np.abs(P.golden(n + "_par")["g_target"]).max() > 0 for n in P.ENVS) >= 3
