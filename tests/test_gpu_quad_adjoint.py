"""-m gpu: the quad form of the Ant adjoint's body level (dsim_core.hpp: dsim_bwd_bodies_quad) in every kernel that runs it, at
N = 1 and N = 3 environments.  Tolerances are those tests/test_gpu_parity.py states: state 1e-4, gradients 1e-3 max-norm relative
against the reference's recording and the scalar oracle; everything between two kernels of this library is bit for bit.

ant_step.npz is the recorded step (S = 16, one mass-matrix group).  ant_rollout_mm1.npz records a rollout of the environment with
the mass matrix refreshed in EVERY substep (ai10m != 0 throughout): its first N environments -- they are independent -- are replayed
through the fused AntEnv (dsim_env_fwd_kernel / dsim_env_bwd_kernel, the kernels the benchmark times) and held to the recorded
observations, rewards, action gradients and end state with the tolerances of tests/test_gpu_envs.py; beside it, its start states
run one operator-level step against the scalar oracle.  The in-contact state is the one of tests/test_emu_quad_adjoint.py."""
import numpy as np
import pytest
import torch

from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden
from quad_adjoint_lib import ant_contact_state

pytestmark = pytest.mark.gpu
NS = [1, 3]
KEYS = ("gq", "gqd", "gact")


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


@pytest.fixture(scope="module")
def plain(t, dev):
    """the default kernels on the recorded step, per N: shared by the comparisons below, never modified"""
    out = {}
    for n in NS:
        g, sl, S, mm, dt = _recorded(n)
        out[n] = _run(_engine(t, dev), dev, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    return out


@pytest.mark.parametrize("n", NS)
def test_step_backward_vs_recording(plain, t, n):
    g, sl, S, mm, dt = _recorded(n)
    r = plain[n]
    e = dict(q=relerr(r["q"], g["q_out"][sl]), qd=relerr(r["qd"], g["qd_out"][sl]),
             gq=relerr(project_tangent(t, g["q_in"][sl], r["gq"]), project_tangent(t, g["q_in"][sl], g["gq_in"][sl])),
             gqd=relerr(r["gqd"], g["gqd_in"][sl]), gact=relerr(r["gact"], g["gact_in"][sl]))
    print("recording N=%d: " % n + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3


def _vs_oracle(t, dev, q, qd, act, S, mm, label):
    rng = np.random.default_rng(5)
    gq, gqd = rng.normal(size=q.shape).astype(np.float32), rng.normal(size=qd.shape).astype(np.float32)
    dt = S / 960.0
    o = oracle_backward(t, q, qd, act, None, dt, S, mm, gq, gqd)
    r = _run(_engine(t, dev), dev, q, qd, act, dt, S, mm, gq, gqd)
    e = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
             gq=relerr(project_tangent(t, q, r["gq"]), project_tangent(t, q, o["gq"])), gqd=relerr(r["gqd"], o["gqd"]),
             gact=relerr(r["gact"], o["gact"]))
    print("%s S=%d mm=%d N=%d: " % (label, S, mm, q.shape[0]) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3


@pytest.mark.parametrize("n", NS)
def test_refresh_in_every_substep_vs_oracle(t, dev, n):
    g = golden("ant_rollout_mm1")
    assert int(g["mm_freq"]) == 1
    act = np.zeros((n, t.n_qd), np.float32)
    act[:, 6:] = 200.0 * g["actions"][0][:n]
    _vs_oracle(t, dev, g["q0"][:n].copy(), g["qd0"][:n].copy(), act, 16, 1, "rollout_mm1 start states")


@pytest.mark.parametrize("n", NS)
def test_fused_env_replays_the_recorded_rollout(dev, n):
    """tests/test_gpu_envs.py::test_rollout_matches_reference on the first n environments of ant_rollout_mm1.npz: 1e-5 on the start
    observation, 1e-3 on observations, rewards, end state and action gradients, cosine of the action gradients above 0.9999"""
    from diffrl_amd import envs
    g = golden("ant_rollout_mm1")
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


@pytest.mark.parametrize("S,mm", [(16, 16), (7, 3)])
def test_feet_in_contact_vs_oracle(t, dev, S, mm):
    q, qd, act = ant_contact_state()
    _vs_oracle(t, dev, q, qd, act, S, mm, "in contact")


@pytest.mark.parametrize("n", NS)
def test_single_wave_kernels_match_bit_for_bit(plain, t, dev, monkeypatch, n):
    g, sl, S, mm, dt = _recorded(n)
    monkeypatch.setenv("DSIM_HELPER", "0")
    r = _run(_engine(t, dev), dev, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    for k in KEYS + ("q", "qd"):
        assert np.array_equal(r[k], plain[n][k]), k


@pytest.mark.parametrize("n", NS)
def test_lean_checkpoints_match_bit_for_bit(plain, t, dev, n):
    g, sl, S, mm, dt = _recorded(n)
    r = _run(_engine(t, dev, ckpt_mode="lean"), dev, g["q_in"][sl], g["qd_in"][sl], g["act_in"][sl], dt, S, mm, g["gq_out"][sl], g["gqd_out"][sl])
    for k in KEYS + ("q", "qd"):
        assert np.array_equal(r[k], plain[n][k]), k


@pytest.mark.parametrize("n", NS)
def test_two_launches_agree_bit_for_bit(plain, t, dev, n):
    g, sl, S, mm, dt = _recorded(n)
    eng = _engine(t, dev)
    r = plain[n]
    again = eng.backward(r["ck"], r["ta"], None, dt, S, mm, _T(g["gq_out"][sl], dev), _T(g["gqd_out"][sl], dev))
    torch.cuda.synchronize()
    for k, x in zip(KEYS, again):
        assert np.array_equal(x.cpu().numpy().reshape(n, -1), r[k]), k


@pytest.mark.parametrize("n", NS)
def test_sweep_rows_equal_the_plain_adjoint(plain, t, dev, n):
    """row 1 of a two-cotangent sweep (row 0: another cotangent) and the state gradients of the parameter sweep"""
    g, sl, S, mm, dt = _recorded(n)
    eng = _engine(t, dev)
    r = plain[n]
    rng = np.random.default_rng(9)
    gq2 = np.stack([rng.normal(size=(n, t.n_q)).astype(np.float32), g["gq_out"][sl]], axis=1)
    gqd2 = np.stack([rng.normal(size=(n, t.n_qd)).astype(np.float32), g["gqd_out"][sl]], axis=1)
    m = eng.backward_multi(r["ck"], r["ta"], None, dt, S, mm, _T(gq2, dev), _T(gqd2, dev))
    p = eng.backward_params(r["ck"], r["ta"], None, dt, S, mm, _T(g["gq_out"][sl], dev), _T(g["gqd_out"][sl], dev))
    torch.cuda.synchronize()
    for k, x, y in zip(KEYS, m, p):
        assert np.array_equal(x.cpu().numpy().reshape(n, 2, -1)[:, 1], r[k]), ("multi", k)
        assert np.array_equal(y.cpu().numpy().reshape(n, -1), r[k]), ("params", k)
    assert torch.isfinite(p[4]).all() and torch.isfinite(p[5]).all()
