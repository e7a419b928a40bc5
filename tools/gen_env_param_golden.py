"""Records tests/golden/<env>_envpar.npz: gradients of a short rollout THROUGH the reference's env.step -- its own env class, its
episode handling, observations and rewards -- with respect to its MODEL tensors joint_target_ke / kd, joint_limit_ke / kd,
joint_target and shape_materials: the fixtures of dsim_env_step_backward_params.  Needs the reference checkout (it imports
oracle/ref_harness.py and oracle/gen_golden.py, which load it at run time); what it writes is recorded numbers only.

    python tools/gen_env_param_golden.py [env ...]

Recipe, per model (as episode_golden of oracle/gen_golden.py):
  * the reference's env class, n = 4 environments, H = 3 steps, stochastic_init off, early termination where the class has it,
    episode_length = 4 with the first half of the environments started at progress 2, so that they restart inside the rollout;
  * the step is shortened so that a parameter gradient can be a yardstick: sim_substeps = 4, sim_dt = 4 h with h the class's own
    substep length, MM_caching_frequency = 2 (one group that re-uses a factor, one refresh per step); the library is called with
    dt = 4 h, substeps = 4, mm_freq = 2;
  * start states: the last n of tests/golden/<env>_con.npz (CartPole: <env>_step.npz); for a model with limited hinge / slider
    joints the LAST one has one such joint moved 0.05 past its upper limit and another 0.05 below its lower limit, as
    tools/gen_param_golden.start_states does (`limit_state` [n] marks it);
  * the six model tensors become fresh leaves with requires_grad before the first step;
  * loss = sum_t (w_rew[t] * rew_t) + sum_t (w_before[t] * obs_before_reset_t) + (w_obs * obs_H), seeded weights;
  * recorded: q0, qd0, progress0, reset_q / reset_qd (the state a restart goes back to), actions, the weights, per step obs, rew,
    done, obs_before; grad_actions; the six parameter gradients per environment (g_target_ke / g_target_kd / g_limit_ke /
    g_limit_kd [n, L], g_target [n, n_q], g_shape_materials [n, shapes, 4]);
  * noise_<name>: K = 8 re-runs with q0 moved by +-1 ulp (random signs): per tensor the max deviation over the max-norm of the
    base, as tools/gen_param_golden.py.  No re-run may flip a done flag: a start state that does is REPLACED (by a state that
    does not, its velocities scaled by 0.9, 0.81, ...) and the model is recorded again;
  * asserted: every parameter the model has gets a non-zero gradient, all four contact columns are non-zero, both limit branches
    occur (the limit state starts past one limit of each kind and its limit_ke gradient is non-zero on both links); at least one
    (environment, step) restarted, and at least one live step is followed by a later step of the same episode.
If a tensor's recorded noise exceeds 1e-3 the recording is shortened to H = 2 (a 1e-2 bound is not accepted).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("ant", "humanoid", "snu", "hopper", "cartpole", "cheetah")
SEED, K_NOISE, N, H_STEPS, S, MM = 47, 8, 4, 3, 4, 2
EP_LEN, LATE = 4, 2
NOISE_MAX = 1e-3
PARAMS = ("target_ke", "target_kd", "limit_ke", "limit_kd", "target", "shape_materials")


def start_states(P, t, name):
    """(q [N, nq], qd [N, nd], limit_state [N], (upper coordinate, lower coordinate) | None)"""
    src = np.load(os.path.join(OUT, name + ("_con.npz" if t.n_contacts else "_step.npz")))
    q, qd = src["q_in"][-N:].astype(np.float32).copy(), src["qd_in"][-N:].astype(np.float32).copy()   # (those in contact)
    assert q.shape[0] == N, (name, q.shape)
    lim, lc, pair = np.zeros(N, bool), P.limited_coords(t), None
    if len(lc) >= 2:
        up, lo = lc[0], lc[1]
        q[N - 1, up] = np.float32(t.joint_limit_upper[up] + P.PAST)
        q[N - 1, lo] = np.float32(t.joint_limit_lower[lo] - P.PAST)
        lim[N - 1], pair = True, (up, lo)
    return q, qd, lim, pair


def record(P, df, envs, G, name, H):
    import torch
    from oracle_lib import template_from_golden
    t = template_from_golden(name)
    q0, qd0, lim, pair = start_states(P, t, name)
    cls, _, _, _, has_et = G.CONFIGS[name]
    L, nq, nd = t.n_links, t.n_q, t.n_qd
    gen = torch.Generator().manual_seed(SEED)
    progress0 = np.zeros(N, np.int64)
    progress0[: N // 2] = LATE
    n_act = n_obs = None
    state = {}

    def run(qv, qdv):
        torch.manual_seed(0)
        np.random.seed(0)
        kw = dict(num_envs=N, device="cpu", render=False, seed=0, episode_length=EP_LEN, no_grad=False, stochastic_init=False,
                  MM_caching_frequency=MM)
        if has_et:
            kw["early_termination"] = True
        env = getattr(envs, cls)(**kw)
        df.config.no_grad = False
        h = env.sim_dt / float(env.sim_substeps)
        env.sim_substeps, env.sim_dt = S, S * h
        model = env.model
        assert model.link_count // N == L and model.joint_dof_count // N == nd
        ns = model.shape_count // N
        env.clear_grad()
        env.reset()
        rq, rqd = env.get_state()
        env.reset_with_state(torch.tensor(qv.reshape(-1)), torch.tensor(qdv.reshape(-1)))
        env.progress_buf[:] = torch.tensor(progress0)
        leaves = dict(target_ke=model.joint_target_ke, target_kd=model.joint_target_kd, limit_ke=model.joint_limit_ke,
                      limit_kd=model.joint_limit_kd, target=model.joint_target, shape_materials=model.shape_materials)
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in leaves.items()}
        model.joint_target_ke, model.joint_target_kd = leaves["target_ke"], leaves["target_kd"]
        model.joint_limit_ke, model.joint_limit_kd = leaves["limit_ke"], leaves["limit_kd"]
        model.joint_target, model.shape_materials = leaves["target"], leaves["shape_materials"]
        env.initialize_trajectory()
        if "acts" not in state:   # (the same seeded draws for the base run and every re-run)
            state["acts"] = torch.tanh(2.0 * (2.0 * torch.rand((H, N, env.num_actions), generator=gen) - 1.0))
            state["w_rew"] = torch.randn((H, N), generator=gen)
            state["w_before"] = 0.01 * torch.randn((H, N, env.num_obs), generator=gen)
            state["w_obs"] = 0.01 * torch.randn((N, env.num_obs), generator=gen)
        acts = state["acts"].clone().requires_grad_(True)
        rec = dict(obs=[], rew=[], done=[], obs_before=[])
        loss = 0.0
        for s in range(H):
            obs, rew, done, info = env.step(acts[s])
            loss = loss + (state["w_rew"][s] * rew).sum() + (state["w_before"][s] * info["obs_before_reset"]).sum()
            for k, v in (("obs", obs), ("rew", rew), ("done", done), ("obs_before", info["obs_before_reset"])):
                rec[k].append(G.t2n(v))
        loss = loss + (state["w_obs"] * obs).sum()
        loss.backward()
        out = {k: np.stack(v) for k, v in rec.items()}
        out["grad_actions"] = G.t2n(acts.grad)
        for k, v in leaves.items():
            g = G.t2n(v.grad) if v.grad is not None else np.zeros(tuple(v.shape), np.float32)
            out["g_" + k] = g.reshape(N, ns, 4) if k == "shape_materials" else g.reshape(N, -1)
        out["reset_q"], out["reset_qd"] = G.t2n(rq).reshape(N, nq), G.t2n(rqd).reshape(N, nd)
        out["dt"] = np.float64(S * h)
        return out

    moved = [P.ulp_moved(q0, np.random.RandomState(100 + k)) for k in range(K_NOISE)]
    for attempt in range(4):
        state.clear()
        gen.manual_seed(SEED)
        base = run(q0, qd0)
        reruns = [run(qk, qd0) for qk in moved]
        flip = np.zeros(N, bool)
        for r in reruns:
            flip |= (r["done"] != base["done"]).any(axis=0)
        if not flip.any():
            break
        assert not (flip & lim).any(), "%s: the limit state flips a done flag under +-1 ulp" % name
        good = int(np.nonzero(~flip & ~lim)[0][0])
        print("%-9s states %s flip a done flag under +-1 ulp: replaced by state %d with velocities x 0.9^k" % (
            name, np.nonzero(flip)[0].tolist(), good), flush=True)
        for j, b in enumerate(np.nonzero(flip)[0]):
            q0[b], qd0[b] = q0[good], qd0[good] * np.float32(0.9 ** (attempt + 1 + j))
        moved = [P.ulp_moved(q0, np.random.RandomState(100 + k)) for k in range(K_NOISE)]
    else:
        raise AssertionError("%s: done flags still flip" % name)

    out = dict(q0=q0, qd0=qd0, progress0=progress0, limit_state=lim, actions=state["acts"].numpy(), w_rew=state["w_rew"].numpy(),
               w_before=state["w_before"].numpy(), w_obs=state["w_obs"].numpy(), episode_length=np.int64(EP_LEN),
               substeps=np.int64(S), mm_freq=np.int64(MM), **base)
    # coverage
    Cn = t.n_contacts
    has_joint = any(int(x) in P.HINGE + (2,) for x in t.joint_type)
    has_hinge = any(int(x) in P.HINGE for x in t.joint_type)
    has_target = any(int(x) in P.HINGE and t.joint_target_ke[i] != 0 for i, x in enumerate(t.joint_type))
    want = dict(target_ke=has_joint, target_kd=has_joint, target=has_target, limit_kd=has_hinge, limit_ke=pair is not None,
                shape_materials=Cn > 0)
    for k, w in want.items():
        assert (not w) or np.abs(base["g_" + k]).max() > 0, (name, k)
    assert np.abs(base["grad_actions"]).max() > 0, name
    if Cn:
        assert all(np.abs(base["g_shape_materials"][..., j]).max() > 0 for j in range(4)), name
    if pair is not None:   # both limit branches: the limit state starts above one upper and below one lower limit
        b = int(np.nonzero(lim)[0][0])
        link_of = {int(t.joint_q_start[i]): i for i in range(L)}
        assert q0[b, pair[0]] > t.joint_limit_upper[pair[0]] and q0[b, pair[1]] < t.joint_limit_lower[pair[1]], name
        assert base["g_limit_ke"][b, link_of[pair[0]]] != 0 and base["g_limit_ke"][b, link_of[pair[1]]] != 0, name
    done = base["done"].astype(bool)   # [H, N]
    assert done.any(), "%s: no restart recorded" % name
    assert (~done[:-1]).any(), "%s: no live step that is followed by a later step of its episode" % name
    for k in ["grad_actions"] + ["g_" + p for p in PARAMS]:
        if np.abs(base[k]).max() > 0:
            out["noise_" + k] = P.tensor_noise([r[k] for r in reruns], base[k])
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in out.values())
    print("%-9s H=%d restarts %d of %d  " % (name, H, int(done.sum()), done.size) + "  ".join(
        "%s %.1e" % (k[6:], out[k]) for k in sorted(out) if k.startswith("noise_")), flush=True)
    ints = ("progress0", "limit_state", "episode_length", "substeps", "mm_freq", "done", "dt")
    return {k: (np.asarray(v, np.float32) if k not in ints else np.asarray(v)) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import gen_param_golden as P
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        out = record(P, df, envs, G, name, H_STEPS)
        if max(float(out[k]) for k in out if k.startswith("noise_g_")) > NOISE_MAX:
            print("%-9s a tensor's noise exceeds %.0e at H = %d: recorded again at H = 2" % (name, NOISE_MAX, H_STEPS), flush=True)
            out = record(P, df, envs, G, name, 2)
        np.savez_compressed(os.path.join(OUT, name + "_envpar.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1:])
