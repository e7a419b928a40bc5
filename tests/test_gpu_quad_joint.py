"""-m gpu: the quad form of the free root's integrator and of its adjoint (dsim_core.hpp: DsimQuadRoot; dsim_math_quad.hpp:
dq_root_integrate, dq_root_integrate_adj) in the Ant kernels that run it, at N = 1 and N = 3 environments.  Tolerances are those
tests/test_gpu_parity.py states: state 1e-4, gradients 1e-3 max-norm relative against the reference's recording and the scalar
oracle; everything between two kernels of this library is bit for bit.

ant_step.npz is the recorded step (S = 16, one mass-matrix group).  ant_rollout_mm1.npz records a rollout of the environment with
the mass matrix refreshed in EVERY substep: its first N environments -- they are independent -- are replayed through the fused AntEnv
(dsim_env_fwd_kernel / dsim_env_bwd_kernel, the kernels the benchmark times) and held to the recorded observations, rewards,
action gradients and end state with the tolerances of tests/test_gpu_envs.py.  The tumbling case has the root far from the
identity rotation with |w| h = 1 (one substep of 1 / 60 s at 60 rad/s), high above the ground: every term of the quaternion
products matters, and the update is far outside the small-angle regime the recordings stay in."""
import numpy as np
import pytest
import torch

from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden

pytestmark = pytest.mark.gpu
NS = [1, 3]
KEYS = ("q", "qd", "gq", "gqd", "gact")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def t():
    return template_from_golden("ant")


def _engine(t, dev, **kw):
    from diffrl_amd.engine import Engine
    return Engine(t, dev, **kw)


def _T(a, dev):
    return torch.tensor(np.ascontiguousarray(a), device=dev).reshape(-1)


def _run(eng, dev, q, qd, act, dt, S, mm, gq, gqd):
    n = q.shape[0]
    ta = _T(act, dev)
    qo, qdo, ck = eng.forward(_T(q, dev), _T(qd, dev), ta, None, dt, S, mm, True)
    r = eng.backward(ck, ta, None, dt, S, mm, _T(gq, dev), _T(gqd, dev))
    torch.cuda.synchronize()
    return dict(q=qo.cpu().numpy().reshape(n, -1), qd=qdo.cpu().numpy().reshape(n, -1), gq=r[0].cpu().numpy().reshape(n, -1),
                gqd=r[1].cpu().numpy().reshape(n, -1), gact=r[2].cpu().numpy().reshape(n, -1), ck=ck, ta=ta)


def _recorded(n):
    g = golden("ant_step")
    sl = slice(0, n)
    return g, sl, int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])


def _run_recorded(t, dev, n, **kw):
    g, sl, S, mm, dt = _recorded(n)
    return _run(_engine(t, dev, **kw), dev, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])


@pytest.fixture(scope="module")
def plain(t, dev):
    """the default (helper-wave) kernels on the recorded step, per N: shared by the comparisons below, never modified"""
    return {n: _run_recorded(t, dev, n) for n in NS}


@pytest.mark.parametrize("n", NS)
def test_recorded_step_vs_recording_and_oracle(plain, t, n):
    g, sl, S, mm, dt = _recorded(n)
    r = plain[n]
    e = dict(q=relerr(r["q"], g["q_out"][sl]), qd=relerr(r["qd"], g["qd_out"][sl]),
             gq=relerr(project_tangent(t, g["q_in"][sl], r["gq"]), project_tangent(t, g["q_in"][sl], g["gq_in"][sl])),
             gqd=relerr(r["gqd"], g["gqd_in"][sl]), gact=relerr(r["gact"], g["gact_in"][sl]))
    print("recording N=%d: " % n + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3
    o = oracle_backward(t, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], None, dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    eo = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
              gq=relerr(project_tangent(t, g["q_in"][sl], r["gq"]), project_tangent(t, g["q_in"][sl], o["gq"])),
              gqd=relerr(r["gqd"], o["gqd"]), gact=relerr(r["gact"], o["gact"]))
    print("oracle    N=%d: " % n + "  ".join("%s %.2e" % kv for kv in eo.items()))
    assert eo["q"] < 1e-4 and eo["qd"] < 1e-4
    assert eo["gq"] < 1e-3 and eo["gqd"] < 1e-3 and eo["gact"] < 1e-3


@pytest.mark.parametrize("n", NS)
def test_fused_env_replays_the_recorded_rollout(dev, n):
    """tests/test_gpu_envs.py::test_rollout_matches_reference on the first n environments of ant_rollout_mm1.npz: 1e-5 on the start
    observation, 1e-3 on observations, rewards, end state and action gradients, cosine of the action gradients above 0.9999"""
    from diffrl_amd import envs
    g = golden("ant_rollout_mm1")
    assert int(g["mm_freq"]) == 1
    H = g["actions"].shape[0]
    e = envs.AntEnv(num_envs=n, device="cuda:0", render=False, seed=0, episode_length=1000, no_grad=False, stochastic_init=False,
                    MM_caching_frequency=int(g["mm_freq"]), early_termination=False)
    assert e.fused
    e.clear_grad()
    e.reset()
    e.reset_with_state(_T(g["q0"][:n], dev), _T(g["qd0"][:n], dev))
    obs0 = e.initialize_trajectory()
    keep = g["obs0"].shape[1] - e.num_actions
    assert relerr(obs0.detach().cpu().numpy()[:, :keep], g["obs0"][:n, :keep]) < 1e-5
    acts = torch.tensor(np.ascontiguousarray(g["actions"][:, :n]), device=dev, requires_grad=True)
    loss = 0.0
    for s in range(H):
        obs, rew, done, info = e.step(acts[s])
        assert int(done.sum()) == 0
        assert relerr(obs.detach().cpu().numpy(), g["obs"][s][:n]) < 1e-3, s
        assert np.abs(rew.detach().cpu().numpy() - g["rew"][s][:n]).max() < 1e-3 * max(1.0, np.abs(g["rew"]).max()), s
        loss = loss - rew.sum()
    loss.backward()
    ga, gr = acts.grad.cpu().numpy().astype(np.float64), g["grad_actions"][:, :n].astype(np.float64)
    cos = (ga * gr).sum() / (np.linalg.norm(ga) * np.linalg.norm(gr))
    print("rollout_mm1 N=%d: action gradients %.2e  cosine %.7f" % (n, relerr(ga, gr), cos))
    assert cos > 0.9999
    assert relerr(ga, gr) < 1e-3
    assert relerr(e.state.joint_q.detach().cpu().numpy().reshape(n, -1), g["q_final"][:n]) < 1e-3


def _tumbling(t, n):
    """n start states with the root two metres up, rotated far from the identity, turning at 60 rad/s about a skew axis"""
    g = golden("ant_step")
    q, qd = g["q_in"][:n].copy(), g["qd_in"][:n].copy()
    act = g["act_in"][:n].copy()
    rng = np.random.default_rng(11)
    for e in range(n):
        r = rng.normal(size=4)
        q[e, 3:7] = (r / np.linalg.norm(r)).astype(np.float32)
        q[e, 1] = 2.0
        w = rng.normal(size=3)
        qd[e, 0:3] = (60.0 * w / np.linalg.norm(w)).astype(np.float32)
    gq, gqd = rng.normal(size=q.shape).astype(np.float32), rng.normal(size=qd.shape).astype(np.float32)
    return q, qd, act, gq, gqd


@pytest.mark.parametrize("n", NS)
def test_tumbling_root_vs_oracle(t, dev, n):
    q, qd, act, gq, gqd = _tumbling(t, n)
    S, mm, dt = 1, 1, 1.0 / 60.0
    assert abs(np.linalg.norm(qd[0, :3]) * dt / S - 1.0) < 1e-3
    o = oracle_backward(t, q, qd, act, None, dt, S, mm, gq, gqd)
    r = _run(_engine(t, dev), dev, q, qd, act, dt, S, mm, gq, gqd)
    e = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
             gq=relerr(project_tangent(t, q, r["gq"]), project_tangent(t, q, o["gq"])), gqd=relerr(r["gqd"], o["gqd"]),
             gact=relerr(r["gact"], o["gact"]))
    print("tumbling N=%d: " % n + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3


@pytest.mark.parametrize("n", NS)
def test_single_wave_kernels_match_bit_for_bit(plain, t, dev, monkeypatch, n):
    monkeypatch.setenv("DSIM_HELPER", "0")
    r = _run_recorded(t, dev, n)
    for k in KEYS:
        assert np.array_equal(r[k], plain[n][k]), k


@pytest.mark.parametrize("n", NS)
def test_two_environments_per_wave_match_bit_for_bit(plain, t, dev, monkeypatch, n):
    """DSIM_PAIR=1: the forward with 32 lanes per environment -- the scalar backend of the integrator's source on lane 0; the
    adjoint (always one environment per wave) from the checkpoint that forward wrote, the saved inverse norm included"""
    monkeypatch.setenv("DSIM_HELPER", "0")
    monkeypatch.setenv("DSIM_PAIR", "1")
    r = _run_recorded(t, dev, n)
    for k in KEYS:
        assert np.array_equal(r[k], plain[n][k]), k


@pytest.mark.parametrize("n", NS)
def test_lean_checkpoints_match_bit_for_bit(plain, t, dev, n):
    """lean: integrate^T recomputes the inverse norm that the full mode reads from the checkpoint"""
    r = _run_recorded(t, dev, n, ckpt_mode="lean")
    for k in KEYS:
        assert np.array_equal(r[k], plain[n][k]), k


@pytest.mark.parametrize("n", NS)
def test_tumbling_root_kernels_agree_bit_for_bit(t, dev, monkeypatch, n):
    """helper, single-wave and two-environments-per-wave kernels where the quaternion update is large"""
    q, qd, act, gq, gqd = _tumbling(t, n)
    out = []
    for helper, pair in (("1", "0"), ("0", "0"), ("0", "1")):
        monkeypatch.setenv("DSIM_HELPER", helper)
        monkeypatch.setenv("DSIM_PAIR", pair)
        out.append(_run(_engine(t, dev), dev, q, qd, act, 1.0 / 60.0, 1, 1, gq, gqd))
    for r in out[1:]:
        for k in KEYS:
            assert np.array_equal(r[k], out[0][k]), k


@pytest.mark.parametrize("n", NS)
def test_two_launches_agree_bit_for_bit(plain, t, dev, n):
    r = _run_recorded(t, dev, n)
    for k in KEYS:
        assert np.array_equal(r[k], plain[n][k]), k
