"""CPU-only: the quad form of the free root's integrator and of its adjoint (dsim_core.hpp: DsimQuadRoot; dsim_math_quad.hpp:
dq_root_integrate, dq_root_integrate_adj) on the host harness, whose executor runs the quad permutations and the row shifts through
shfl.  The specialised (static) Ant paths are the ones that take the form: one step and its adjoint on the recorded step
(ant_step.npz) and on the in-contact state of tests/quad_adjoint_lib.py, through the harness's fused environment entry points with
zero observation / reward cotangents -- the harness's operator-level entry points always run the generic layout, which does
not take the form (tests/test_emu_quad_adjoint.py goes the same way).

Variants: 64 lanes per environment (the quad backend: four lanes hold the root) and 32 lanes (the lane count of the kernels with
two environments per wavefront: the scalar backend of the same source on lane 0), each with full and with lean checkpoints (lean:
integrate^T recomputes the inverse norm the full mode reads from the checkpoint).  The harness has one executor -- no helper
wavefront; the helper kernels are compared on the GPU (tests/test_gpu_quad_joint.py).  Outputs are held to the recording / the
scalar oracle with the bounds of tests/test_gpu_parity.py (state 1e-4, gradients 1e-3, max-norm relative); all variants are bit-equal
to each other."""
import numpy as np
import pytest

from emu_lib import emu, emu_env_backward, emu_env_forward, env_spec_for, mode
from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden
from quad_adjoint_lib import ant_contact_state

STATE_TOL, GRAD_TOL = 1e-4, 1e-3
VARIANTS = [(False, False), (False, True), (True, False), (True, True)]   # (32 lanes, lean)
KEYS = ("q", "qd", "gq", "gqd", "gact")


def _step(t, q, qd, act, dt, S, mm, gq, gqd, half, lean):
    """the environment scales its eight actions by 200 onto dofs 6 .. 13 (the division and the multiplication move an input by an
    ulp at most); gact is returned for those dofs (the root's six are not actuated: zeros)"""
    assert not np.any(act[:, :6]) and np.abs(act[:, 6:]).max() <= 200.0
    spec, keep = env_spec_for("ant", t)
    actions = (act[:, 6:] / np.float32(200.0)).astype(np.float32)
    n = q.shape[0]
    lib = emu()
    with mode(lib, static=True, lean=lean):
        lib.dsim_emu_set_half_wave(1 if half else 0)
        try:
            qo, qdo, _, _, ck = emu_env_forward(t, spec, q, qd, actions, dt, S, mm)
            rgq, rgqd, ga = emu_env_backward(t, spec, ck, actions, dt, S, mm, gq, gqd, np.zeros((n, spec.n_obs), np.float32),
                                             np.zeros(n, np.float32))
        finally:
            lib.dsim_emu_set_half_wave(0)
    gact = np.zeros_like(act)
    gact[:, 6:] = ga / np.float32(200.0)
    return dict(q=qo, qd=qdo, gq=rgq, gqd=rgqd, gact=gact)


@pytest.fixture(scope="module")
def t():
    return template_from_golden("ant")


@pytest.fixture(scope="module")
def recorded(t):
    """the recorded step (its first 8 environments) in every variant: computed once, never modified"""
    g = golden("ant_step")
    sl = slice(0, 8)
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    return {v: _step(t, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl], *v) for v in VARIANTS}


@pytest.fixture(scope="module")
def contact(t):
    q, qd, act = ant_contact_state()
    rng = np.random.default_rng(5)
    gq, gqd = rng.normal(size=q.shape).astype(np.float32), rng.normal(size=qd.shape).astype(np.float32)
    S, mm = 7, 3
    dt = S / 960.0
    o = oracle_backward(t, q, qd, act, None, dt, S, mm, gq, gqd)
    return q, o, {v: _step(t, q, qd, act, dt, S, mm, gq, gqd, *v) for v in VARIANTS}


@pytest.mark.parametrize("half,lean", VARIANTS)
def test_recorded_step_vs_recording(t, recorded, half, lean):
    g = golden("ant_step")
    sl = slice(0, 8)
    r = recorded[(half, lean)]
    e = dict(q=relerr(r["q"], g["q_out"][sl]), qd=relerr(r["qd"], g["qd_out"][sl]),
             gq=relerr(project_tangent(t, g["q_in"][sl], r["gq"]), project_tangent(t, g["q_in"][sl], g["gq_in"][sl])),
             gqd=relerr(r["gqd"], g["gqd_in"][sl]), gact=relerr(r["gact"][:, 6:], g["gact_in"][sl][:, 6:]))
    print("recording lanes=%d lean=%d: " % (32 if half else 64, lean) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < STATE_TOL and e["qd"] < STATE_TOL
    assert e["gq"] < GRAD_TOL and e["gqd"] < GRAD_TOL and e["gact"] < GRAD_TOL


@pytest.mark.parametrize("half,lean", VARIANTS)
def test_feet_in_contact_vs_oracle(t, contact, half, lean):
    q, o, runs = contact
    r = runs[(half, lean)]
    e = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
             gq=relerr(project_tangent(t, q, r["gq"]), project_tangent(t, q, o["gq"])), gqd=relerr(r["gqd"], o["gqd"]),
             gact=relerr(r["gact"][:, 6:], o["gact"][:, 6:]))
    print("in contact lanes=%d lean=%d: " % (32 if half else 64, lean) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < STATE_TOL and e["qd"] < STATE_TOL
    assert e["gq"] < GRAD_TOL and e["gqd"] < GRAD_TOL and e["gact"] < GRAD_TOL


@pytest.mark.parametrize("half,lean", VARIANTS[1:])
def test_variants_are_bit_equal(recorded, contact, half, lean):
    """quad backend on four lanes against the scalar backend on lane 0; saved against recomputed inverse norm.  With 32 lanes the
    library ships forward kernels only, and the harness's 32-lane adjoint sums its subtrees in another order
    (tests/test_emu_static_variants.py::test_pair_kernels_lane_count_is_bit_identical): there the state is compared with the
    64-lane run, and everything with the other 32-lane run."""
    for runs in (recorded, contact[2]):
        for k in KEYS:
            if half:
                assert np.array_equal(runs[(half, lean)][k], runs[(True, False)][k]), k
            if not half or k in ("q", "qd"):
                assert np.array_equal(runs[(half, lean)][k], runs[VARIANTS[0]][k]), k
