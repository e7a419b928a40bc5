"""CPU-only: the quad form of the Ant adjoint's body level (dsim_core.hpp: dsim_bwd_bodies_quad, four lanes per link) on the host
harness, whose executor runs the quad permutations, row shifts and row folds through shfl.  The specialised (static) Ant paths
are the ones that take the form; the step adjoint is held to the scalar oracle and to the reference's recording with the bounds
tests/test_emu_phases.py uses for the step adjoint (1e-4 on every gradient, 2e-5 on the end state).

Schedules: S = 16 with one mass-matrix group (the shipped Ant schedule; the group's first substep is a refresh substep, so the
inertia cotangents ai10m of the body level are non-zero there and zero in the fifteen others) and S = 7 with groups of 1 and of 3.
Every start state has contact rows reduced per body (agx); one is taken from the contact read-out's recording with feet on the
ground, checked below to carry contact forces."""
import numpy as np
import pytest

import mm_sched as M
from emu_lib import emu, emu_env_backward, emu_env_forward, env_spec_for, mode
from quad_adjoint_lib import ant_contact_state
from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden

GRAD_TOL, STATE_TOL = 1e-4, 2e-5


def _step(t, q, qd, act, dt, S, mm, gq, gqd):
    """one step and its adjoint through the harness's fused environment entry points -- the ones that instantiate the phase code
    with the model's compile-time layout (emu_lib.mode(static=True)), as the library's kernels do.  The environment scales its
    eight actions by 200 onto dofs 6 .. 13 (the division and the multiplication move an input by an ulp at most); gact is returned for
    those dofs (the root's six are not actuated: zeros)."""
    assert not np.any(act[:, :6]) and np.abs(act[:, 6:]).max() <= 200.0
    spec, keep = env_spec_for("ant", t)
    actions = (act[:, 6:] / np.float32(200.0)).astype(np.float32)
    n = q.shape[0]
    with mode(emu(), static=True):
        qo, qdo, _, _, ck = emu_env_forward(t, spec, q, qd, actions, dt, S, mm)
        rgq, rgqd, ga = emu_env_backward(t, spec, ck, actions, dt, S, mm, gq, gqd, np.zeros((n, spec.n_obs), np.float32),
                                         np.zeros(n, np.float32))
    gact = np.zeros_like(act)
    gact[:, 6:] = ga / np.float32(200.0)
    return dict(q=qo, qd=qdo, gq=rgq, gqd=rgqd, gact=gact)


def test_ant_step_adjoint_vs_recording_and_oracle():
    t, g = template_from_golden("ant"), golden("ant_step")
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    assert (S, mm) == (16, 16)
    r = _step(t, g["q_in"], g["qd_in"], g["act_in"], dt, S, mm, g["gq_out"], g["gqd_out"])
    e = dict(q=relerr(r["q"], g["q_out"]), qd=relerr(r["qd"], g["qd_out"]),
             gq=relerr(project_tangent(t, g["q_in"], r["gq"]), project_tangent(t, g["q_in"], g["gq_in"])),
             gqd=relerr(r["gqd"], g["gqd_in"]), gact=relerr(r["gact"][:, 6:], g["gact_in"][:, 6:]))
    print("recording S=16 mm=16: " + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < STATE_TOL and e["qd"] < 5e-5   # (tests/test_emu_phases.py: the recorded step's end state)
    assert e["gq"] < GRAD_TOL and e["gqd"] < GRAD_TOL and e["gact"] < GRAD_TOL
    sl = slice(0, 4)
    o = oracle_backward(t, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], None, dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    eo = dict(gq=relerr(project_tangent(t, g["q_in"][sl], r["gq"][sl]), project_tangent(t, g["q_in"][sl], o["gq"])),
              gqd=relerr(r["gqd"][sl], o["gqd"]), gact=relerr(r["gact"][sl][:, 6:], o["gact"][:, 6:]))
    print("oracle    S=16 mm=16: " + "  ".join("%s %.2e" % kv for kv in eo.items()))
    assert max(eo.values()) < GRAD_TOL


@pytest.mark.parametrize("mm", [1, 3])
def test_ant_seven_substeps_vs_oracle(mm):
    c = M.case("ant")
    r = _step(c["t"], c["q"], c["qd"], c["act"], M.DT, M.S, mm, c["gq"], c["gqd"])
    o = M.oracle("ant", mm)
    r["gact"][:, :6] = o["gact"][:, :6]   # (not actuated through the environment: taken out of the comparison)
    M.assert_step("ant", mm, r, state_tol=STATE_TOL, grad_tol=GRAD_TOL, label="host quad")


@pytest.mark.parametrize("S,mm", [(16, 16), (7, 3)])
def test_ant_feet_in_contact_vs_oracle(S, mm):
    t = template_from_golden("ant")
    q, qd, act = ant_contact_state()
    rng = np.random.default_rng(5)
    gq, gqd = rng.normal(size=q.shape).astype(np.float32), rng.normal(size=qd.shape).astype(np.float32)
    dt = S / 960.0
    o = oracle_backward(t, q, qd, act, None, dt, S, mm, gq, gqd)
    r = _step(t, q, qd, act, dt, S, mm, gq, gqd)
    e = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
             gq=relerr(project_tangent(t, q, r["gq"]), project_tangent(t, q, o["gq"])), gqd=relerr(r["gqd"], o["gqd"]),
             gact=relerr(r["gact"][:, 6:], o["gact"][:, 6:]))
    print("in contact S=%d mm=%d: " % (S, mm) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < STATE_TOL and e["qd"] < STATE_TOL
    assert e["gq"] < GRAD_TOL and e["gqd"] < GRAD_TOL and e["gact"] < GRAD_TOL
