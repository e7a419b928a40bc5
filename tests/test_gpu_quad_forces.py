"""-m gpu: the Ant forward kernels with the body-level constants of the quad kinematics in registers (dsim_core.hpp: DsimBodyRegs
-- the joint-frame translations and axes of the lane's chain, the centre of mass, gravity, the inertia words and the mass of its
link, loaded once in front of the substep loop by the kernels with one environment per wavefront).  What can go wrong: a constant
of the wrong link or the wrong chain position, a register block that a caller outside the substep loop reads without having
loaded it, a value that survives into a launch of another model.  So: recorded start states with feet in contact and two hinges
past their limits (an all-airborne state would leave the contact sums zero), N = 1 and 3, S = 4, mass-matrix refresh every 1, 2
and 4 substeps, step forward and adjoint against the generic kernels of the same library (which reload everything) and the scalar
oracle, every output and the checkpoint words; the kernel modes against each other bit for bit (the two-environment kernels keep the
reload: same words, same operations); the fused AntEnv; the fused adjoint against the step adjoint; launches after
Engine.set_params and a graph replay against fresh models; two models with different body constants alternating on one device.

Bounds are those of tests/test_gpu_joint_regs.py: specialised against generic kernels 1e-5; state 1e-4 and gradients 1e-3 against
the oracle; everything between two kernels of the specialised set, and between a reused and a fresh model, bit for bit."""
import copy

import numpy as np
import pytest
import torch

import test_emu_quad_forces as EQ
import test_gpu_joint_regs as jr
from oracle_lib import golden, relerr, template_from_golden

pytestmark = pytest.mark.gpu
DEV = jr.DEV
NS = [1, 3]
S4 = 4
MMS = [1, 2, 4]
KEYS = jr.KEYS
MODES = jr.MODES


@pytest.fixture(scope="module")
def t():
    return template_from_golden("ant")


def _case(t, n):
    """feet in contact (the recorded step's environments 7 ..), one hinge below its lower limit and one above its upper limit:
    the cases of the host tier, tests/test_emu_quad_forces.py"""
    return EQ.case(t, n)


def _ckpt_fields(t, ck, S):
    """ftot, tau-independent words the forward's joint-space phase saves, per substep: f_tot [L][6] and qdd [nd]"""
    from emu_lib import layout
    off, _ = layout(t)
    nd, L = t.n_qd, t.n_links
    row = off["qdd"] + nd - off["q"]
    stride = (row + 3) & ~3
    pick = lambda f, n: np.stack([ck[:, s * stride + off[f] - off["q"]:s * stride + off[f] - off["q"] + n] for s in range(S)], 1)  # noqa: E731
    return dict(ftot=pick("ftot", 6 * L), qdd=pick("qdd", nd), f_i10=pick("i10", 10 * L), a=pick("a", 6 * L))


# ---- operator level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_step_pair_vs_generic_kernels_and_oracle(t, n, mm):
    c = _case(t, n)
    spec, gen = jr._engine(t), jr._engine(t, DSIM_FORCE_GENERIC="1")
    assert spec.variant > 0 and gen.variant == 0
    a, b = jr._run(spec, c, S4, mm), jr._run(gen, c, S4, mm)
    for k in KEYS:
        e = relerr(a[k], b[k])
        print("S=4 mm=%d N=%d specialised vs generic %s %.2e" % (mm, n, k, e))
        assert e < 1e-5, (k, e)
    fa, fb = _ckpt_fields(t, a["ckpt"], S4), _ckpt_fields(t, b["ckpt"], S4)
    for k in fa:   # (body force inputs -- world inertia, acceleration -- and what the joint-space phase makes of them)
        e = relerr(fa[k], fb[k])
        print("S=4 mm=%d N=%d specialised vs generic checkpoint %s %.2e" % (mm, n, k, e))
        assert np.isfinite(fa[k]).all() and e < 1e-5, (k, e)
    assert np.abs(fa["ftot"]).max() > 0
    jr._assert_vs_oracle(t, c, a, jr._oracle_run(t, c, S4, mm, "contact"), "S=4 mm=%d N=%d oracle" % (mm, n))


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_kernel_modes_agree_bit_for_bit(t, n, mm):
    """helper, single-wave (registers), two environments per wavefront (reload) and the lean kernels: outputs and every defined
    checkpoint word (f_tot and qdd among them)"""
    c = _case(t, n)
    ref = jr._run(jr._engine(t, **MODES["helper"]), c, S4, mm)
    for name in ("single", "pair"):
        jr._same(jr._run(jr._engine(t, **MODES[name]), c, S4, mm), ref, ckpt=(t, S4, mm))
    for kw in (MODES["helper"], MODES["single"]):
        jr._same(jr._run(jr._engine(t, ckpt_mode="lean", **kw), c, S4, mm), ref)


# ---- constants must be the launch's own ------------------------------------------------------------------------------------------
def _other_bodies(t):
    """the same tree with other body constants: every mass, inertia, centre of mass and joint-frame translation changed per link"""
    t2 = copy.deepcopy(t)
    L = t.n_links
    k = (1.0 + 0.1 * np.arange(1, L + 1)).astype(np.float32)
    t2.body_I_m = (np.asarray(t.body_I_m, np.float32) * k.reshape(L, 1, 1)).astype(np.float32)   # (mass and inertia about the COM)
    xcm = np.asarray(t.joint_X_cm, np.float32).copy()
    xcm[:, :3] += np.float32(0.01) * k.reshape(L, 1)
    t2.joint_X_cm = xcm
    xpj = np.asarray(t.joint_X_pj, np.float32).copy()
    xpj[:, :3] *= (1.0 + np.float32(0.05) * k.reshape(L, 1)).astype(np.float32)
    t2.joint_X_pj = xpj
    t2.validate()
    return t2


@pytest.mark.parametrize("n", NS)
def test_two_models_with_other_body_constants_alternate(t, n):
    """model A, model B (other masses, inertias, centres of mass, joint frames), A again: every launch equals a fresh model's bit
    for bit and agrees with the generic kernels and the oracle on B's constants -- nothing is kept from launch to launch"""
    c = _case(t, n)
    t2 = _other_bodies(t)
    ea, eb = jr._engine(t, fresh=True), jr._engine(t2, fresh=True)
    assert ea.variant > 0 and eb.variant > 0
    ra1, rb, ra2 = jr._run(ea, c, S4, 2), jr._run(eb, c, S4, 2), jr._run(ea, c, S4, 2)
    jr._same(ra1, ra2, ckpt=(t, S4, 2))
    jr._same(rb, jr._run(jr._engine(t2, fresh=True), c, S4, 2), ckpt=(t, S4, 2))
    assert not np.array_equal(ra1["q"], rb["q"])
    with jr._switches(DSIM_FORCE_GENERIC="1"):
        from diffrl_amd.engine import Engine
        gen = Engine(t2, torch.device(DEV))
    assert gen.variant == 0
    g = jr._run(gen, c, S4, 2)
    for k in KEYS:
        assert relerr(rb[k], g[k]) < 1e-5, k
    jr._assert_vs_oracle(t2, c, rb, jr.oracle_backward(t2, c["q"], c["qd"], c["act"], None, c["dt"], S4, 2, c["gq"], c["gqd"]),
                         "other bodies N=%d oracle" % n)


@pytest.mark.parametrize("n", NS)
def test_launch_after_set_params_equals_fresh_model(t, n):
    c = _case(t, n)
    eng = jr._engine(t, fresh=True)
    r1 = jr._run(eng, c, S4, 2)
    t3 = jr._with_gains(t)
    p = eng.step_parameters()
    p.joint_target_ke = jr._T(t3.joint_target_ke)
    p.joint_limit_ke = jr._T(t3.joint_limit_ke)
    eng.set_params(p)
    r2 = jr._run(eng, c, S4, 2)
    jr._same(r1, jr._run(jr._engine(t, fresh=True), c, S4, 2), ckpt=(t, S4, 2))
    jr._same(r2, jr._run(jr._engine(t3, fresh=True), c, S4, 2), ckpt=(t, S4, 2))
    assert not np.array_equal(r1["q"], r2["q"])


# ---- fused environment ----------------------------------------------------------------------------------------------------------
def _env_inputs(n):
    g = golden("ant_rollout_mm1")
    rng = np.random.default_rng(29)
    acts = np.tanh(rng.normal(size=(1, n, g["actions"].shape[2]))).astype(np.float32)
    return g["q0"][:n], g["qd0"][:n], acts


@pytest.mark.parametrize("mm", [1, 2, 3, 4])
@pytest.mark.parametrize("n", NS)
def test_fused_env_step_vs_generic_kernels(n, mm):
    """one AntEnv step (16 substeps) at mm 1 .. 4: the kernel modes bit for bit, the generic kernels at the bounds of
    tests/test_gpu_joint_regs.py (1e-4 obs, rew, state; 1e-3 action gradients)"""
    q0, qd0, acts = _env_inputs(n)
    ref = jr._env_rollout(n, mm, acts, q0, qd0, **MODES["helper"])
    for name in ("single", "pair"):
        r = jr._env_rollout(n, mm, acts, q0, qd0, **MODES[name])
        for k in ref:
            assert np.array_equal(r[k], ref[k]), (name, k)
    gen = jr._env_rollout(n, mm, acts, q0, qd0, generic=True, DSIM_FORCE_GENERIC="1")
    e = {k: relerr(ref[k], gen[k]) for k in ref}
    print("AntEnv mm=%d N=%d specialised vs generic: " % (mm, n) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["obs"] < 1e-4 and e["rew"] < 1e-4 and e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["ga"] < 1e-3


@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("mode", ["helper", "single"])
@pytest.mark.parametrize("ckpt_mode", ["full", "lean"])
def test_fused_adjoint_equals_step_adjoint_on_one_checkpoint(t, ckpt_mode, mode, mm):
    """the fused forward's checkpoint (body constants from registers in both forwards), then the fused adjoint with zero cotangents
    on obs and rew against the step adjoint on that checkpoint: gq and gqd bit for bit (tests/sweep_drivers.py: why)"""
    from emu_lib import env_spec_for
    n = 3
    c = _case(t, n)
    eng = jr._engine(t, ckpt_mode=ckpt_mode, **MODES[mode])
    spec0, scale_h = env_spec_for("ant", t)
    spec = type(spec0).from_buffer_copy(spec0)
    scale = torch.tensor(scale_h, device=DEV)
    spec.act_scale = scale.data_ptr()
    na, off = int(spec.n_act), int(spec.act_offset)
    actions = np.random.default_rng(37).uniform(-0.9, 0.9, size=(n, na)).astype(np.float32)
    act = np.zeros((n, t.n_qd), np.float32)
    act[:, off:off + na] = actions * scale_h
    ta, tact = torch.tensor(actions, device=DEV), jr._T(act)
    qo, qdo, obs, rew, ck = eng.env_forward(spec, jr._T(c["q"]), jr._T(c["qd"]), ta, c["dt"], S4, mm, True)
    sq, sqd, _ = eng.forward(jr._T(c["q"]), jr._T(c["qd"]), tact, None, c["dt"], S4, mm, False)
    assert torch.equal(qo, sq) and torch.equal(qdo, sqd)
    gq, gqd = jr._T(c["gq"]), jr._T(c["gqd"])
    step = eng.backward(ck, tact, None, c["dt"], S4, mm, gq, gqd)
    fused = eng.env_backward(spec, ck, ta, c["dt"], S4, mm, gq, gqd, torch.zeros_like(obs), torch.zeros_like(rew))
    torch.cuda.synchronize()
    eng.status()
    assert torch.isfinite(step[0]).all() and step[0].abs().max() > 0
    assert torch.equal(step[0], fused[0]) and torch.equal(step[1], fused[1])


def test_two_step_graph_replay_equals_fresh_eager_model():
    """two env steps captured as one graph and replayed twice: loss and action gradients of an eager run on a fresh environment"""
    from diffrl_amd.graph import GraphedRollout
    n, mm = 3, 2
    g = golden("ant_rollout_mm1")
    q0, qd0 = g["q0"][:n], g["qd0"][:n]
    acts = np.tanh(np.random.default_rng(31).normal(size=(2, n, g["actions"].shape[2]))).astype(np.float32)

    def body_for(a):
        def body(env):
            env.initialize_trajectory()
            return -torch.stack([env.step(a_t)[1] for a_t in a.unbind(0)]).sum()
        return body

    def prepared():
        e = jr._ant_env(n, mm)
        e.clear_grad()
        e.reset()
        e.reset_with_state(jr._T(q0), jr._T(qd0))
        return e

    a1 = torch.tensor(acts, device=DEV, requires_grad=True)
    e1 = prepared()   # (held until the backward pass is done: the environment owns the model the adjoint launches run on)
    loss1 = body_for(a1)(e1)
    loss1.backward()
    torch.cuda.synchronize()
    a2 = torch.tensor(acts, device=DEV, requires_grad=True)
    e2 = prepared()
    roll = GraphedRollout(e2, body_for(a2), leaves=[a2], carry_state=False)
    for _ in range(2):
        loss2 = roll.replay()
    torch.cuda.synchronize()
    assert float(loss2) == float(loss1.detach())
    assert torch.equal(a2.grad, a1.grad)
