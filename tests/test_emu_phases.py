"""CPU-only: the kernel phase code (diffrl_amd/csrc/dsim_core.hpp), executed lane-serially on the host
(tests/emu), against the reference goldens and the CPU oracle.  This checks the restructured
algorithm (tree-parallel kinematics, 10-parameter inertias, composite-body mass matrix, explicit
inverse) and the hand-derived adjoint; the real HIP build is checked by the -m gpu tests."""
import numpy as np
import pytest

import mm_sched as M
from emu_lib import emu_backward, emu_forward, layout
from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden

ENVS = ["cartpole", "ant", "humanoid", "snu", "hopper", "cheetah"]


@pytest.mark.parametrize("env", ENVS)
def test_layout_fits_lds(env):
    off, dims = layout(template_from_golden(env))
    assert off["total_words"] * 4 <= 160 * 1024
    assert dims["L"] <= 64 and dims["nd"] <= 64


@pytest.mark.parametrize("env", ENVS)
def test_env_step_forward_vs_reference(env):
    t = template_from_golden(env)
    g = golden(env + "_step")
    qo, qdo, _ = emu_forward(t, g["q_in"], g["qd_in"], g["act_in"], g.get("muscle_act_in"), float(g["dt"]),
                             int(g["substeps"]), int(g["mm_freq"]))
    # stated fp32 tolerance for one env-step: 1e-4; measured <= 7e-6
    assert relerr(qo, g["q_out"]) < 2e-5
    assert relerr(qdo, g["qd_out"]) < 5e-5


@pytest.mark.parametrize("env", ENVS)
def test_env_step_adjoint_vs_reference(env):
    t = template_from_golden(env)
    g = golden(env + "_step")
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    mact = g.get("muscle_act_in")
    _, _, ck = emu_forward(t, g["q_in"], g["qd_in"], g["act_in"], mact, dt, S, mm, want_ckpt=True)
    r = emu_backward(t, ck, g["act_in"], mact, dt, S, mm, g["gq_out"], g["gqd_out"])
    assert relerr(project_tangent(t, g["q_in"], r["gq"]), project_tangent(t, g["q_in"], g["gq_in"])) < 1e-4
    assert relerr(r["gqd"], g["gqd_in"]) < 1e-4
    if "gact_in" in g:
        assert relerr(r["gact"], g["gact_in"]) < 1e-4
    else:
        assert relerr(r["gmact"], g["gmuscle_act_in"]) < 1e-4


@pytest.mark.parametrize("env,mm", [("ant", 1), ("ant", 5), ("cartpole", 3), ("snu", 48)])
def test_mass_matrix_caching_groups(env, mm):
    """mm_freq that does not divide the substep count / is 1 / equals it: checkpoint groups in the adjoint"""
    t = template_from_golden(env)
    g = golden(env + "_step")
    S, dt = int(g["substeps"]), float(g["dt"])
    if env == "snu":
        S = 6
        mm = 4
    sl = slice(0, 3)
    mact = g["muscle_act_in"][sl] if "muscle_act_in" in g else None
    q, qd, act = g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl]
    o = oracle_backward(t, q, qd, act, mact, dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    qo, qdo, ck = emu_forward(t, q, qd, act, mact, dt, S, mm, want_ckpt=True)
    r = emu_backward(t, ck, act, mact, dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    assert relerr(qo, o["q_out"]) < 2e-5
    assert relerr(project_tangent(t, q, r["gq"]), project_tangent(t, q, o["gq"])) < 1e-4
    assert relerr(r["gqd"], o["gqd"]) < 1e-4


# The S = 7 schedule set on every shipped model (tests/mm_sched.py: inputs, oracle results and why seven substeps).  Bounds: the tight
# ones of the cases above (2e-5 state, 1e-4 gradients) where this harness measured well inside them against the oracle -- CartPole,
# Ant, Hopper, Cheetah <= 1e-5 in every gradient --; the stated ones (1e-4 / 1e-3) for Humanoid (6.8e-5) and
# SNUHumanoid (2.5e-4 in gqd at mm = 3, next 9.3e-5), whose figures leave no margin under 1e-4.
_TIGHT = ("cartpole", "ant", "hopper", "cheetah")


@pytest.mark.parametrize("mm", M.MMS)
@pytest.mark.parametrize("env", ENVS)
def test_mass_matrix_caching_groups_seven_substeps(env, mm):
    """test_mass_matrix_caching_groups on all six models at S = 7: group sizes 1x7 | 2,2,2,1 | 3,3,1 | 4,3 | 6,1 | 7 | 7 (mm > S);
    end state and every cotangent against the scalar oracle"""
    c = M.case(env)
    t = c["t"]
    qo, qdo, ck = emu_forward(t, c["q"], c["qd"], c["act"], c["mact"], M.DT, M.S, mm, want_ckpt=True)
    r = emu_backward(t, ck, c["act"], c["mact"], M.DT, M.S, mm, c["gq"], c["gqd"])
    tight = env in _TIGHT
    M.assert_step(env, mm, dict(q=qo, qd=qdo, **r), state_tol=2e-5 if tight else M.STATE_TOL, grad_tol=1e-4 if tight else M.GRAD_TOL,
                  label="host")


@pytest.mark.parametrize("env", ["ant", "humanoid", "snu"])
def test_quaternion_radial_component_is_the_whole_operator_level_deviation(env):
    """d loss / d joint_q at the OPERATOR boundary differs from the reference's only along each unit quaternion itself
    (the direction in which its norm changes): the reference differentiates its rotation formulas literally, also where
    they are not rotations; here the pose adjoint is a tangent-space (wrench) quantity and that component is exactly
    zero.  The deviation is quantified, not hidden behind a projection: (i) this implementation's radial part is ~0,
    (ii) the un-projected difference to the reference IS the reference's radial part, (iii) its size is reported."""
    import numpy as np
    t = template_from_golden(env)
    g = golden(env + "_step")
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    mact = g.get("muscle_act_in")
    _, _, ck = emu_forward(t, g["q_in"], g["qd_in"], g["act_in"], mact, dt, S, mm, want_ckpt=True)
    r = emu_backward(t, ck, g["act_in"], mact, dt, S, mm, g["gq_out"], g["gqd_out"])
    from oracle_lib import radial_split
    own_rad, resid, other, rad_ref = radial_split(t, g["q_in"], r["gq"], g["gq_in"])
    assert own_rad < 1e-4                       # (i)
    assert resid < 1e-4                         # (ii): ours - ref == -(reference's radial part) on the quaternion blocks
    assert other < 1e-4                         # every other coordinate: no projection needed
    print("%s: reference's radial quaternion cotangent, max |.| / max |gq| = %.3f" % (env, rad_ref))


@pytest.mark.parametrize("env", ENVS)
def test_first_substep_intermediates_vs_reference(env):
    """The forward intermediates of the first substep -- X_sc, S, v, a, world inertias, f_tot, qdd -- as the forward pass
    leaves them in the checkpoint, against the reference's own recording of the same substep (not only the boundary tensors).
    tests/test_gpu_parity.py runs the same comparison on what the hipcc-compiled kernels wrote."""
    from ckpt_fields import BOUNDS, compare_with_reference, first_substep
    t = template_from_golden(env)
    g = golden(env + "_step")
    _, _, ck = emu_forward(t, g["q_in"], g["qd_in"], g["act_in"], g.get("muscle_act_in"), float(g["dt"]), int(g["substeps"]),
                           int(g["mm_freq"]), want_ckpt=True)
    err = compare_with_reference(t, first_substep(t, ck), g, relerr)
    for k, e in err.items():
        assert e < BOUNDS[k], (k, e)


def test_forward_is_defined_on_unit_quaternions_only():
    """include/dsim.h states the precondition of dsim_step_forward with measured numbers: off the unit sphere the kernels'
    forms (10-parameter inertia, wrench form) are NOT the reference's literal formulas (quat.h:113-116, sim.py:1117-1134).
    Host harness vs the reference-order oracle on the Ant step recording with the root quaternion scaled: the error in
    qd_out grows with the distance from the manifold and is far above the 1e-4 state tolerance at |q| = 1.001 -- which is why
    the kernels check | |q|^2 - 1 | <= 2e-4 and the library refuses otherwise (tests/test_gpu_contract.py)."""
    from emu_lib import emu_forward
    from oracle_lib import oracle_forward
    g = golden("ant_step")
    t = template_from_golden("ant")
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    err = {}
    for lam in (1.0, 1.00005, 1.001, 1.01):
        q = g["q_in"].copy()
        q[:, 3:7] *= np.float32(lam)
        qo, qdo, _ = emu_forward(t, q, g["qd_in"], g["act_in"], None, dt, S, mm)
        ro, rdo, _ = oracle_forward(t, q, g["qd_in"], g["act_in"], None, dt, S, mm)
        err[lam] = relerr(qdo, rdo)
    assert err[1.0] < 1e-4
    assert err[1.00005] < 1e-3                     # inside the enforced 1e-4 ball: still within the gradient-level tolerance
    assert 1e-3 < err[1.001] < 2e-2                # measured 5.3e-3
    assert 1e-2 < err[1.01] < 0.2                  # measured 4.7e-2
    assert err[1.0] < err[1.00005] < err[1.001] < err[1.01]


@pytest.mark.parametrize("env", ["ant", "humanoid", "snu"])
def test_literal_backward_on_the_host_harness_equals_the_reference_unprojected(env):
    """dsim_step_backward_literal, host side: the adjoint phases hand (gq_1, gqd_1, adj H) to the forward-mode tangent of the first
    substep (diffrl_amd/csrc/dsim_literal.hpp), which adds the component along each quaternion that the reference's literal
    adjoint has (quat.h:232-288, spatial.h:740-798).  UN-projected against the reference's recordings (1e-3 stated; measured
    1.1e-6 / 5.8e-6 / 7.4e-6) and, with random cotangents and a step whose first mass-matrix group ends inside the step, against
    the oracle's reference-order adjoint."""
    from emu_lib import emu_backward, emu_forward
    from oracle_lib import golden, oracle_backward, relerr, template_from_golden
    t, g = template_from_golden(env), golden(env + "_step")
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    mact = g.get("muscle_act_in")
    qo, qdo, ck = emu_forward(t, g["q_in"], g["qd_in"], g["act_in"], mact, dt, S, mm, want_ckpt=True)
    plain = emu_backward(t, ck, g["act_in"], mact, dt, S, mm, g["gq_out"], g["gqd_out"])
    lit = emu_backward(t, ck, g["act_in"], mact, dt, S, mm, g["gq_out"], g["gqd_out"], literal=True)
    assert relerr(lit["gq"], g["gq_in"]) < 1e-4 and relerr(plain["gq"], g["gq_in"]) > 0.03
    for k in ("gqd", "gact", "gmact"):
        assert np.array_equal(lit[k], plain[k])
    rng = np.random.default_rng(1)
    gq, gqd = rng.normal(0, 1, g["q_in"].shape).astype(np.float32), rng.normal(0, 1, g["qd_in"].shape).astype(np.float32)
    n = min(4, g["q_in"].shape[0])
    for S2, mm2 in ((1, 1), (3, 2)):
        dt2 = dt * S2 / S
        o = oracle_backward(t, g["q_in"][:n], g["qd_in"][:n], g["act_in"][:n], mact[:n] if mact is not None else None, dt2, S2, mm2, gq[:n], gqd[:n])
        qo, qdo, ck = emu_forward(t, g["q_in"][:n], g["qd_in"][:n], g["act_in"][:n], mact[:n] if mact is not None else None, dt2, S2, mm2, want_ckpt=True)
        r = emu_backward(t, ck, g["act_in"][:n], mact[:n] if mact is not None else None, dt2, S2, mm2, gq[:n], gqd[:n], literal=True)
        assert relerr(r["gq"], o["gq"]) < 1e-3, (S2, mm2)
