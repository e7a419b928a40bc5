"""CPU: the fused env adjoint with model-parameter gradients (dsim_core.hpp: dsim_env_fused_backward on DsimParCtxT, the code of
dsim_env_bwd_param_kernel) on the lane-serial host build of the phase code (tests/emu/dsim_emu_envpar.cpp through
tests/env_par_lib.py): all six models, generic and specialised layouts, one and four wavefronts per environment, full and lean
checkpoints, substeps = 4 with the mass matrix refreshed every substep, every 2nd and once.

Reference: tests/golden/<env>_envpar.npz, three steps of the reference's own env class through its episode handling with
requires_grad on its model tensors (tools/gen_env_param_golden.py).  Bound per parameter tensor, folded to the reference's
shapes, in its max-norm: max(1e-4, 10 x its recorded +-1 ulp noise of the reference).
"""
import numpy as np
import pytest

import env_par_lib as E
import par_lib as P
from oracle_lib import golden

VARIANTS = [(False, 1, "generic-1w"), (False, 4, "generic-4w"), (True, 1, "specialised-1w"), (True, 4, "specialised-4w")]
MODES = [(False, "full"), (True, "lean")]
N, S = 3, E.SUBSTEPS
_runs = {}


def _inputs(name):
    """N environments of the recording: its start states, first actions and seeded cotangents"""
    t, g, spec, keep = E.case(name)
    rs = np.random.RandomState(3)
    c = dict(q=g["q0"][-N:], qd=g["qd0"][-N:], a=g["actions"][0][-N:].copy(),
             gq=rs.normal(size=(N, t.n_q)).astype(np.float32), gqd=rs.normal(size=(N, t.n_qd)).astype(np.float32),
             gobs=rs.normal(size=(N, spec.n_obs)).astype(np.float32), grew=rs.normal(size=N).astype(np.float32),
             gobs_b=rs.normal(size=(N, spec.n_obs)).astype(np.float32))
    c["a"][0, 0] = 1.5   # a clipped action
    return t, g, spec, keep, c


def _run(name, static, waves, lean, mm):
    """forward (no episode: every environment live), the parameter adjoint and the plain adjoint under full cotangents, and both
    step adjoints under the state cotangents alone: once per kernel variant, left unchanged"""
    key = (name, static, waves, lean, mm)
    if key not in _runs:
        t, g, spec, keep, c = _inputs(name)
        dt = float(g["dt"])
        kw = dict(static=static, waves=waves, lean=lean)
        fwd = E.env_forward(t, spec, c["q"], c["qd"], c["a"], dt, S, mm, **kw)
        ck = fwd[4]
        cots = (c["gq"], c["gqd"], c["gobs"], c["grew"], c["gobs_b"])
        par = E.env_backward_params(t, spec, ck, c["a"], dt, S, mm, *cots, **kw)
        plain = E.env_backward(t, spec, ck, c["a"], dt, S, mm, *cots, **kw)
        zero = E.env_backward_params(t, spec, ck, c["a"], dt, S, mm, c["gq"], c["gqd"], None, None, None, **kw)
        act, mact = E.joint_actuation(t, spec, keep, c["a"])
        step = E.step_backward(t, ck, act, mact, dt, S, mm, c["gq"], c["gqd"], **kw)
        for r in (par, zero, step):
            for v in r.values():
                if v is not None:
                    v.setflags(write=False)
        _runs[key] = (fwd, par, plain, zero, step)
    return _runs[key]


@pytest.mark.parametrize("mm", [1, 2, 4])
@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_state_gradients_equal_the_plain_env_adjoint_bit_for_bit(name, static, waves, label, lean, mode, mm):
    """(a) gq_in / gqd_in / gactions of the parameter context are dsim_emu_env_backward's"""
    _, par, plain, _, _ = _run(name, static, waves, lean, mm)
    for k, w in zip(("gq", "gqd", "ga"), plain):
        assert np.isfinite(w).all() and np.array_equal(par[k], w), k
    assert par["ga"][0, 0] == 0.0   # the clipped action


@pytest.mark.parametrize("mm", [1, 2, 4])
@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_parameter_outputs_equal_the_step_adjoint_on_the_fused_checkpoint(name, static, waves, label, lean, mode, mm):
    """(b) with zero gobs / grew / gobs_before the parameter outputs are dsim_emu_step_backward's on the fused forward's checkpoint
    under the same gq_out / gqd_out (every environment is live), bit for bit"""
    t = E.case(name)[0]
    _, _, _, zero, step = _run(name, static, waves, lean, mm)
    assert np.isfinite(zero["g_dof"]).all() and np.array_equal(zero["g_dof"], step["g_dof"])
    assert np.abs(zero["g_dof"]).max() > 0
    if t.n_contacts:
        assert np.isfinite(zero["g_contact"]).all() and np.array_equal(zero["g_contact"], step["g_contact"])
        assert np.abs(zero["g_contact"]).max() > 0


@pytest.mark.parametrize("name", P.ENVS)
def test_null_patterns(name):
    """g_dof only, g_contact only, neither: what is returned does not change"""
    t, g, spec, keep, c = _inputs(name)
    _, full, _, _, _ = _run(name, False, 1, False, 2)
    ck = _run(name, False, 1, False, 2)[0][4]
    args = (t, spec, ck, c["a"], float(g["dt"]), S, 2, c["gq"], c["gqd"], c["gobs"], c["grew"], c["gobs_b"])
    for want in ((True, False), (False, True), (False, False)):
        r = E.env_backward_params(*args, want=want)
        assert all(np.array_equal(r[k], full[k]) for k in ("gq", "gqd", "ga"))
        assert (r["g_dof"] is None) == (not want[0]) and (r["g_contact"] is None) == (not want[1])
        if want[0]:
            assert np.array_equal(r["g_dof"], full["g_dof"])
        if want[1]:
            assert np.array_equal(r["g_contact"], full["g_contact"])


@pytest.mark.parametrize("lean,mode", MODES)
@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", P.ENVS)
def test_recorded_rollout_matches_the_reference(name, static, waves, label, lean, mode):
    """(c) the recorded rollout -- restarts included -- within max(1e-4, 10 x recorded noise) per parameter tensor"""
    t, g, spec, keep = E.case(name)
    dt, mm = float(g["dt"]), int(g["mm_freq"])
    assert int(g["substeps"]) == S and mm == E.MM
    kw = dict(static=static, waves=waves, lean=lean)
    rec, ga, g_dof, g_con = E.rollout(
        name, t, g, spec,
        lambda q, qd, a, ep: E.env_forward(t, spec, q, qd, a, dt, S, mm, episode=ep.host(), **kw),
        lambda ck, a, *cots: E.env_backward_params(t, spec, ck, a, dt, S, mm, *cots, **kw))
    E.check_recording(name, t, g, rec, ga, g_dof, g_con, show=lambda s: print(label, mode, s))


def test_every_entry_point_resolves_in_this_harness():
    """libdsim_emu_envpar.so carries every entry point the *_lib.py modules call (tests/test_emu_harness.py's scan) plus its own two"""
    import test_emu_harness as H
    assert H._missing(E.lib()) == [] and all(hasattr(E.lib(), n) for n in E.ENTRY_POINTS)


def test_recordings_cover_every_rule():
    """what tools/gen_env_param_golden.py asserts when it records, held against the committed files"""
    for name in P.ENVS:
        t, g, _, _ = E.case(name)
        done = g["done"].astype(bool)
        assert done.any() and (~done[:-1]).any(), name
        if t.n_contacts:
            assert all(np.abs(g["g_shape_materials"][..., j]).max() > 0 for j in range(4)), name
        if g["limit_state"].any():
            assert np.abs(g["g_limit_ke"][g["limit_state"]]).max() > 0, name
        for k in P.PARAM_TENSORS:
            if "noise_" + k in g:
                assert float(g["noise_" + k]) <= 1e-3, (name, k)
    assert sum(bool(golden(n + "_envpar")["limit_state"].any()) for n in P.ENVS) >= 4


@pytest.mark.parametrize("static,waves,label", VARIANTS[::3])
def test_invalid_environment_returns_zero_rows(static, waves, label):
    """(d) an environment of humanoid_exploded.npz flagged invalid returns zero rows in every output, and with sanitize_grads on
    everything that comes back is finite"""
    name = "humanoid"
    t, g, spec, keep = E.case(name)
    x = golden("humanoid_exploded")
    n = x["q0"].shape[0]
    dt = float(g["dt"])
    prog, cnt, done = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64)
    ob = np.zeros((n, spec.n_obs), np.float32)
    ep = E.make_episode(prog, done, ob, x["q0"][None].copy(), np.zeros((1, n, t.n_qd), np.float32), cnt, 1000, True, True)
    kw = dict(static=static, waves=waves)
    ck = E.env_forward(t, spec, x["q0"], x["qd0"], x["actions"][0], dt, S, E.MM, episode=ep, **kw)[4]
    assert done[1] == 1 and done[3] == 1 and done[0] == 0
    rs = np.random.RandomState(9)
    cots = (rs.normal(size=(n, t.n_q)), rs.normal(size=(n, t.n_qd)), rs.normal(size=(n, spec.n_obs)), rs.normal(size=n),
            rs.normal(size=(n, spec.n_obs)))
    spec.sanitize_grads = 1
    try:
        r = E.env_backward_params(t, spec, ck, x["actions"][0], dt, S, E.MM, *cots, **kw)
    finally:
        spec.sanitize_grads = 0
    for k, v in r.items():
        assert np.isfinite(v).all(), k
        assert not v[1].any() and not v[3].any(), k
    assert np.abs(r["g_dof"][0]).max() > 0 and np.abs(r["g_dof"][2]).max() > 0   # (the valid ones; nothing touches the ground here)


@pytest.mark.parametrize("static,waves,label", VARIANTS[::3])
def test_sanitize_scrubs_the_parameter_outputs(static, waves, label):
    """the exploded states of humanoid_exploded.npz WITHOUT the invalid-state rule: nothing flags them, the sweep runs on them and
    its parameter accumulators go non-finite.  sanitize_grads = 0: they come back as they are; 1: every output word is finite --
    the parameter outputs by the same scrub as gq / gqd / gactions -- and what was finite before is returned unchanged"""
    t, g, spec, keep = E.case("humanoid")
    x = golden("humanoid_exploded")
    n = x["q0"].shape[0]
    dt = float(g["dt"])
    kw = dict(static=static, waves=waves)
    ck = E.env_forward(t, spec, x["q0"], x["qd0"], x["actions"][0], dt, S, E.MM, **kw)[4]   # (no episode block: every step is live)
    rs = np.random.RandomState(9)
    cots = (rs.normal(size=(n, t.n_q)), rs.normal(size=(n, t.n_qd)), rs.normal(size=(n, spec.n_obs)), rs.normal(size=n), None)
    out = {}
    for on in (0, 1):
        spec.sanitize_grads = on
        try:
            out[on] = E.env_backward_params(t, spec, ck, x["actions"][0], dt, S, E.MM, *cots, **kw)
        finally:
            spec.sanitize_grads = 0
    raw, clean = out[0], out[1]
    for k in ("g_dof", "g_contact", "gq", "gqd"):
        bad = ~np.isfinite(raw[k])
        print(label, k, "non-finite words without the scrub:", int(bad.sum()), "of", bad.size)
        assert np.isfinite(clean[k]).all(), k
        assert np.array_equal(clean[k][~bad], raw[k][~bad]) and not clean[k][bad].any(), k
    assert np.isfinite(clean["ga"]).all()
    # not vacuous: the scrub had work to do in both parameter outputs
    assert (~np.isfinite(raw["g_dof"])).any() and (~np.isfinite(raw["g_contact"])).any() and (~np.isfinite(raw["gq"])).any()
    assert np.isfinite(raw["g_dof"][[0, 2]]).all() and np.abs(clean["g_dof"][[0, 2]]).max() > 0   # the sound environments


@pytest.mark.parametrize("static,waves,label", VARIANTS[::3])
@pytest.mark.parametrize("name", ["ant", "snu", "cartpole"])
def test_restarted_environment_keeps_its_reward_terms(name, static, waves, label):
    """(e) a restarted environment: non-zero parameter rows under a reward cotangent alone, unchanged when gq_out / gqd_out change"""
    t, g, spec, keep, c = _inputs(name)
    dt = float(g["dt"])
    prog, cnt, done = np.array([0, 3, 0], np.int64), np.zeros(N, np.int32), np.zeros(N, np.int64)
    pool_q, pool_qd = g["reset_q"][None, :N].copy(), g["reset_qd"][None, :N].copy()
    ep = E.make_episode(prog, done, None, pool_q, pool_qd, cnt, 4, False, False)
    kw = dict(static=static, waves=waves)
    ck = E.env_forward(t, spec, c["q"], c["qd"], c["a"], dt, S, E.MM, episode=ep, **kw)[4]
    assert done.tolist() == [0, 1, 0]
    grew = np.ones(N, np.float32)
    a = E.env_backward_params(t, spec, ck, c["a"], dt, S, E.MM, None, None, None, grew, None, **kw)
    b = E.env_backward_params(t, spec, ck, c["a"], dt, S, E.MM, c["gq"], c["gqd"], c["gobs"], grew, None, **kw)
    assert np.abs(a["g_dof"][1]).max() > 0
    for k in ("gq", "gqd", "ga", "g_dof", "g_contact"):
        assert np.array_equal(a[k][1], b[k][1]), k           # the restarted environment ignores gq_out / gqd_out / gobs
    assert not np.array_equal(a["g_dof"][0], b["g_dof"][0])  # a live one does not


@pytest.mark.parametrize("static,label", [(False, "generic"), (True, "specialised")])
@pytest.mark.parametrize("name", P.ENVS)
def test_set_values_equal_a_model_created_with_them(name, static, label):
    """(f) perturbed parameter values as the shared block: the bits of a model built from a template that holds them"""
    t, g, spec, keep, c = _inputs(name)
    dt = float(g["dt"])
    p = P.perturbed_params(t)
    cots = (c["gq"], c["gqd"], c["gobs"], c["grew"], c["gobs_b"])

    def run(tt, pp):
        fwd = E.env_forward(tt, spec, c["q"], c["qd"], c["a"], dt, S, E.MM, params=pp, static=static)
        return fwd, E.env_backward_params(tt, spec, fwd[4], c["a"], dt, S, E.MM, *cots, params=pp, static=static)

    (fa, ra), (fb, rb) = run(t, p), run(P.with_params(t, p), None)
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert all(np.array_equal(ra[k], rb[k]) for k in ra if ra[k] is not None)
    base = _run(name, static, 1, False, E.MM)
    assert not np.array_equal(fa[1], base[0][1]) and not np.array_equal(ra["g_dof"], base[1]["g_dof"])   # the values matter
