"""-m gpu: the DFlexEnv surface (step / obs / reward / autograd) against rollouts recorded from the
reference environments (tests/golden/<env>_rollout.npz, oracle/gen_golden.py:rollout_golden).
Stated tolerance for short-horizon trajectories and gradients: 1e-3 max-norm relative, cosine >= 0.9999
(BASELINE.md section 4)."""
import numpy as np
import pytest
import torch

from oracle_lib import golden, relerr

pytestmark = pytest.mark.gpu
CASES = ["cartpole", "ant", "humanoid", "snu", "hopper", "cheetah"]


def _make(env, n, no_grad=False, mm=None):
    from diffrl_amd import envs
    cls = {"cartpole": envs.CartPoleSwingUpEnv, "ant": envs.AntEnv, "humanoid": envs.HumanoidEnv,
           "snu": envs.SNUHumanoidEnv, "hopper": envs.HopperEnv, "cheetah": envs.CheetahEnv}[env]
    mm = mm or {"cartpole": 4, "ant": 16, "humanoid": 48, "snu": 8, "hopper": 16, "cheetah": 16}[env]
    kw = dict(num_envs=n, device="cuda:0", render=False, seed=0, episode_length=1000, no_grad=no_grad,
              stochastic_init=False, MM_caching_frequency=mm)
    if env in ("cartpole", "ant", "hopper", "cheetah"):
        kw["early_termination"] = False
    return cls(**kw)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("env,name", [(e, e + "_rollout") for e in CASES] + [(e, e + "_rollout_mm1") for e in ["ant", "snu", "humanoid"]])
def test_rollout_matches_reference(env, name, fused):
    """fused=True: one launch per env.step each way (obs/reward inside the kernels);
    fused=False: SimStep kernels + torch observation / reward code.
    <env>_rollout_mm1: recorded with MM_caching_frequency = 1 (the reference classes' constructor default): the mass matrix
    and its adjoint run in every substep."""
    g = golden(name)
    H, n = g["actions"].shape[0], g["actions"].shape[1]
    e = _make(env, n, mm=int(g["mm_freq"]))
    e.fused = fused
    dev = torch.device("cuda:0")
    e.clear_grad()
    e.reset()
    e.reset_with_state(torch.tensor(g["q0"], device=dev).reshape(-1), torch.tensor(g["qd0"], device=dev).reshape(-1))
    obs0 = e.initialize_trajectory()
    na = e.num_actions if getattr(e, "obs_has_actions", False) else 0
    ref0 = g["obs0"]
    keep = ref0.shape[1] - na
    assert relerr(obs0.detach().cpu().numpy()[:, :keep], ref0[:, :keep]) < 1e-5
    acts = torch.tensor(g["actions"], device=dev, requires_grad=True)
    loss = 0.0
    for t in range(H):
        obs, rew, done, info = e.step(acts[t])
        assert int(done.sum()) == 0
        assert obs.grad_fn is not None and rew.grad_fn is not None
        assert "obs_before_reset" in info and "episode_end" in info
        assert relerr(obs.detach().cpu().numpy(), g["obs"][t]) < 1e-3, t
        assert np.abs(rew.detach().cpu().numpy() - g["rew"][t]).max() < 1e-3 * max(1.0, np.abs(g["rew"]).max()), t
        loss = loss - rew.sum()
    loss.backward()
    ga, gr = acts.grad.cpu().numpy().astype(np.float64), g["grad_actions"].astype(np.float64)
    cos = (ga * gr).sum() / (np.linalg.norm(ga) * np.linalg.norm(gr))
    assert cos > 0.9999
    tol = 1e-3
    if relerr(ga, gr) >= tol:
        # conditioning probe in the reference's operation order (see tests/test_emu_fused_env.py): SNU env 0 has a
        # near-stiction foot contact, where a 1-ulp change of the start state moves the reference gradient by ~3-5e-3
        from oracle_env import rollout_grad
        from oracle_lib import template_from_golden
        rng = np.random.default_rng(0)
        q0p = (g["q0"].astype(np.float64) * (1.0 + 1e-7 * rng.normal(size=g["q0"].shape))).astype(np.float32)
        _, _, gp = rollout_grad(env, template_from_golden(env), q0p, g["qd0"], g["actions"])
        import probe_ledger
        tol = probe_ledger.accept("rollout", relerr(ga, gr), relerr(gp, gr), 1, env + " rollout")
    assert relerr(ga, gr) < tol
    assert relerr(e.state.joint_q.detach().cpu().numpy().reshape(n, -1), g["q_final"]) < 1e-3


def test_observe_kernel_on_the_generic_kernels_of_the_muscle_model(monkeypatch):
    """dsim_env_observe on SNUHumanoid's GENERIC kernels, two environments (the rollouts above launch it on the specialised set):
    the model whose LDS image needs the opt-in beyond 64 KiB -- the start observation against the recording and the torch path"""
    monkeypatch.setenv("DSIM_FORCE_GENERIC", "1")
    g = golden("snu_rollout")
    dev = torch.device("cuda:0")
    e = _make("snu", 2, mm=int(g["mm_freq"]))
    assert e.model.engine().variant == 0
    e.reset()
    e.reset_with_state(torch.tensor(g["q0"][:2], device=dev).reshape(-1), torch.tensor(g["qd0"][:2], device=dev).reshape(-1))
    obs = e.initialize_trajectory().detach().clone()
    e.fused = False
    obs_torch = e.initialize_trajectory().detach()
    keep = g["obs0"].shape[1] - (e.num_actions if getattr(e, "obs_has_actions", False) else 0)
    assert torch.isfinite(obs).all()
    assert relerr(obs.cpu().numpy()[:, :keep], g["obs0"][:2, :keep]) < 1e-5
    assert torch.allclose(obs, obs_torch, rtol=1e-4, atol=1e-5)


def test_no_grad_path_and_autoreset():
    """dflex.config.no_grad fast path (no checkpoints) gives the same states; episode_length resets work"""
    g = golden("ant_rollout")
    H, n = g["actions"].shape[0], g["actions"].shape[1]
    dev = torch.device("cuda:0")
    e = _make("ant", n, no_grad=True)
    e.episode_length = 3
    e.reset()
    e.reset_with_state(torch.tensor(g["q0"], device=dev).reshape(-1), torch.tensor(g["qd0"], device=dev).reshape(-1))
    for t in range(3):
        obs, rew, done, info = e.step(torch.tensor(g["actions"][t], device=dev))
        assert obs.grad_fn is None
        if t < 2:
            assert int(done.sum()) == 0
            assert relerr(obs.cpu().numpy(), g["obs"][t]) < 1e-3
    assert int(done.sum()) == n                       # episode_length reached -> every env reset
    assert int(e.progress_buf.sum()) == 0
    assert torch.allclose(e.state.joint_q.view(n, -1)[:, 1], torch.full((n,), 0.75, device=dev))


def test_fused_and_unfused_agree_with_resets():
    """early termination on: the fused path and the torch path flag the same envs and give the same obs"""
    dev = torch.device("cuda:0")
    from diffrl_amd import envs
    outs = []
    for fused in (True, False):
        e = envs.AntEnv(num_envs=32, device="cuda:0", no_grad=True, stochastic_init=False, MM_caching_frequency=16,
                        early_termination=True, episode_length=12)
        e.fused = fused
        e.reset()
        gen = torch.Generator().manual_seed(0)
        rec = []
        for t in range(16):
            a = (2.0 * torch.rand((32, 8), generator=gen) - 1.0).to(dev)
            obs, rew, done, _ = e.step(a)
            rec.append((obs.clone(), rew.clone(), done.clone()))
        outs.append(rec)
    for (o1, r1, d1), (o2, r2, d2) in zip(*outs):
        assert torch.equal(d1, d2)
        assert torch.allclose(o1, o2, rtol=1e-4, atol=1e-5) and torch.allclose(r1, r2, rtol=1e-4, atol=1e-5)
    assert sum(int(d.sum()) for _, _, d in outs[0]) >= 32    # the episode_length reset happened


def test_fused_episode_gradients_match_the_torch_path():
    """grad mode with restarts inside the rollout: the in-kernel episode handling (progress, done, restart, obs_before_reset,
    graph cut) gives the same outputs and the same action gradients as the reference-style torch ops + reset()"""
    dev = torch.device("cuda:0")
    from diffrl_amd import envs
    H, n = 8, 32
    gen = torch.Generator().manual_seed(3)
    acts0 = (2.0 * torch.rand((H, n, 8), generator=gen) - 1.0).to(dev)
    w = torch.randn((n, 37), generator=gen).to(dev)
    res = []
    for fused in (True, False):
        e = envs.AntEnv(num_envs=n, device="cuda:0", no_grad=False, stochastic_init=False, MM_caching_frequency=16,
                        early_termination=True, episode_length=5)
        e.fused = fused
        e.reset()
        e.progress_buf[: n // 2] = 2           # half of the environments finish their episode two steps earlier
        e.initialize_trajectory()
        a = acts0.clone().requires_grad_(True)
        loss, rec = 0.0, []
        for t in range(H):
            obs, rew, done, info = e.step(a[t])
            loss = loss - rew.sum() + 0.01 * (w * info["obs_before_reset"]).sum() + 0.01 * (w * obs).sum()
            rec.append((obs.detach().clone(), rew.detach().clone(), done.clone(), info["obs_before_reset"].detach().clone(),
                        e.progress_buf.clone()))
        loss.backward()
        res.append((rec, a.grad.clone(), e.state.joint_q.detach().clone()))
    for (o1, r1, d1, b1, p1), (o2, r2, d2, b2, p2) in zip(res[0][0], res[1][0]):
        assert torch.equal(d1, d2) and torch.equal(p1, p2)
        assert torch.allclose(o1, o2, rtol=1e-4, atol=1e-5) and torch.allclose(r1, r2, rtol=1e-4, atol=1e-5)
        assert torch.allclose(b1, b2, rtol=1e-4, atol=1e-5)
    assert sum(int(d.sum()) for _, _, d, _, _ in res[0][0]) >= n
    err, tol = relerr(res[0][1].cpu().numpy(), res[1][1].cpu().numpy()), 1e-3
    if err >= tol:
        # 1e-3 unless the REFERENCE-order gradient of this very rollout is more sensitive than that --
        # the scalar oracle (reference operation order, same episode rules and loss) from a start state moved by 1e-7
        from oracle_env import episode_rollout_grad
        from oracle_lib import template_from_golden
        prog0 = np.zeros(n, np.int64)
        prog0[: n // 2] = 2
        A, W = acts0.cpu().numpy(), w.cpu().numpy()
        g0, _ = episode_rollout_grad("ant", template_from_golden("ant"), prog0, A, W, 5)
        scale = (1.0 + 1e-7 * np.random.default_rng(0).normal(size=(n, 15))).astype(np.float32)
        g1, _ = episode_rollout_grad("ant", template_from_golden("ant"), prog0, A, W, 5, q0_scale=scale)
        tol = max(tol, 3.0 * relerr(g1, g0))
        print("fused vs torch path: %.2e, reference-order sensitivity %.2e" % (err, tol / 3.0))
    assert err < tol
    assert torch.allclose(res[0][2], res[1][2], rtol=1e-4, atol=1e-5)


def _restart_states(cls, n, steps, **kw):
    """states of the environments right after in-kernel restarts: episode_length = 1 makes every step end an episode"""
    dev = torch.device("cuda:0")
    e = cls(num_envs=n, device="cuda:0", no_grad=True, stochastic_init=True, episode_length=1, seed=3, **kw)
    e.reset()
    a = torch.zeros((n, e.num_actions), device=dev)
    qs, qds = [], []
    for _ in range(steps):
        obs, rew, done, _ = e.step(a)
        assert int(done.sum()) == n and int(e.progress_buf.sum()) == 0
        qs.append(e.state.joint_q.view(n, -1).clone())
        qds.append(e.state.joint_qd.view(n, -1).clone())
    return e, torch.cat(qs), torch.cat(qds)


@pytest.mark.parametrize("name", ["ant", "humanoid", "snu", "hopper", "cheetah", "cartpole"])
def test_in_kernel_restarts_follow_the_reset_distribution(name):
    """Every restart inside the fused step draws a FRESH start state (counter-based generator keyed by environment and
    restart number).  Its distribution must be the environment's own reset_state() -- the reference's reset(),
    envs/ant.py:199-234 etc.: first two moments of every coordinate over ~10k restarts against ~10k torch draws, the unit
    norm and the tilt-angle range of the root rotation, and no state ever repeated."""
    from diffrl_amd import envs
    cls = {"ant": envs.AntEnv, "humanoid": envs.HumanoidEnv, "snu": envs.SNUHumanoidEnv, "hopper": envs.HopperEnv,
           "cheetah": envs.CheetahEnv, "cartpole": envs.CartPoleSwingUpEnv}[name]
    kw = {"MM_caching_frequency": {"ant": 16, "humanoid": 48, "snu": 8, "hopper": 16, "cheetah": 16, "cartpole": 4}[name]}
    n, steps = 512, 20
    e, q, qd = _restart_states(cls, n, steps, **kw)
    # the same number of draws from the environment's torch reset_state()
    ref_q, ref_qd = [], []
    ids = torch.arange(n, device=q.device)
    for _ in range(steps):
        e.state.joint_q, e.state.joint_qd = e.state.joint_q.clone(), e.state.joint_qd.clone()
        e.reset_state(ids)
        ref_q.append(e.state.joint_q.view(n, -1).clone())
        ref_qd.append(e.state.joint_qd.view(n, -1).clone())
    ref_q, ref_qd = torch.cat(ref_q), torch.cat(ref_qd)
    N = q.shape[0]
    for x, r, what in ((q, ref_q, "q"), (qd, ref_qd, "qd")):
        sd = r.std(0)
        tol_mean = 5.0 * sd / N ** 0.5 + 1e-6            # 5 sigma of the sample mean
        assert ((x.mean(0) - r.mean(0)).abs() <= 2 ** 0.5 * tol_mean).all(), what
        # sample standard deviations of uniform noise: relative error ~ 0.5 / sqrt(N) -> 6 % is > 5 sigma
        live = sd > 1e-6
        assert ((x.std(0)[live] / sd[live] - 1.0).abs() < 0.06).all(), what
        assert (x.std(0)[~live] < 1e-6).all(), what         # coordinates without noise stay put
        # same support: the sample extremes of two sets of ~10k uniform draws agree to a few 1e-4 of the range
        span = (r.max(0).values - r.min(0).values)
        assert (x.min(0).values >= r.min(0).values - 0.03 * span - 1e-4).all() and \
               (x.max(0).values <= r.max(0).values + 0.03 * span + 1e-4).all(), what
    if name in ("ant", "humanoid", "snu"):
        rot, ref_rot = q[:, 3:7], ref_q[:, 3:7]
        assert ((rot.norm(dim=1) - 1.0).abs() < 1e-5).all()
        start = e.start_rotation.view(1, 4)
        ang = lambda r_: 2.0 * torch.acos(((r_ * start).sum(1)).abs().clamp(max=1.0))   # angle between r and the start rotation
        assert float(ang(rot).max()) <= float(np.pi / 24.0) + 1e-3                        # |angle| <= noise_angle / 2
        assert abs(float(ang(rot).mean()) - float(ang(ref_rot).mean())) < 0.01
    # fresh draw every time: no two restart states coincide (a 2-entry pool repeated after two restarts)
    assert torch.unique(torch.cat((q, qd), 1), dim=0).shape[0] == N
    # and the sequence depends on the seed only: same seed -> same restarts
    e2, q2, qd2 = _restart_states(cls, n, 2, **kw)
    assert torch.equal(q2, q[:2 * n]) and torch.equal(qd2, qd[:2 * n])


def test_shac_style_usage():
    """the call pattern of algorithms/shac.py:184-251 (initialize_trajectory, H steps, backward, clear)"""
    e = _make("ant", 64)
    dev = torch.device("cuda:0")
    actor = torch.nn.Linear(e.num_obs, e.num_actions).to(dev)
    obs = e.initialize_trajectory()
    total = 0.0
    for t in range(4):
        obs, rew, done, info = e.step(torch.tanh(actor(obs)))
        total = total - rew.sum()
    total.backward()
    assert all(torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0 for p in actor.parameters())
    e.clear_grad()
    assert not e.state.joint_q.requires_grad


@pytest.mark.parametrize("env,H,iters", [("cartpole", 16, 25), ("ant", 8, 15)])
def test_gradients_are_useful(env, H, iters):
    """first-order optimisation of an open-loop action sequence through the fused step improves the return"""
    e = _make(env, 32)
    dev = torch.device("cuda:0")
    acts = torch.zeros((H, 32, e.num_actions), device=dev, requires_grad=True)
    opt = torch.optim.Adam([acts], lr=0.05)
    q0, qd0 = e.get_state()
    losses = []
    for it in range(iters):
        e.clear_grad()
        e.reset_with_state(q0, qd0)
        e.initialize_trajectory()
        loss = 0.0
        for t in range(H):
            obs, rew, done, _ = e.step(torch.tanh(acts[t]))
            loss = loss - rew.mean()
        opt.zero_grad()
        loss.backward()
        assert torch.isfinite(acts.grad).all()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0] - 1e-3, losses


@pytest.mark.parametrize("name", ["ant", "humanoid", "snu", "hopper", "cheetah", "cartpole"])
def test_long_stochastic_rollouts_stay_finite(name):
    """300 steps of random actions with stochastic restarts on every environment class: finite observations and rewards,
    episodes end and restart (in-kernel), progress counters stay inside [0, episode_length)"""
    from diffrl_amd import envs
    cls = {"ant": envs.AntEnv, "humanoid": envs.HumanoidEnv, "snu": envs.SNUHumanoidEnv, "hopper": envs.HopperEnv,
           "cheetah": envs.CheetahEnv, "cartpole": envs.CartPoleSwingUpEnv}[name]
    mm = {"ant": 16, "humanoid": 48, "snu": 8, "hopper": 16, "cheetah": 16, "cartpole": 4}[name]
    n, L = 64, 120
    e = cls(num_envs=n, device="cuda:0", no_grad=True, stochastic_init=True, MM_caching_frequency=mm, episode_length=L)
    e.reset()
    gen = torch.Generator().manual_seed(5)
    dones = 0
    for t in range(300):
        a = (2.0 * torch.rand((n, e.num_actions), generator=gen) - 1.0).to("cuda:0")
        obs, rew, done, _ = e.step(a)
        dones += int(done.sum())
        if t % 50 == 49:
            e.clear_grad()          # redraws the pool of start states
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert dones >= 2 * n                              # at least the two length-based resets of every environment
    assert int(e.progress_buf.min()) >= 0 and int(e.progress_buf.max()) < L
    assert torch.isfinite(e.state.joint_q).all() and torch.isfinite(e.state.joint_qd).all()
