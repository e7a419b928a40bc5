"""Inertia: the short-horizon policy optimisation of examples/shac_lite.py with two terms written on the joint-space inertia of
the states the rollout visits (Model.mass_matrix): the kinetic energy 0.5 qd^T H(q) qd of the whole robot, and the task-space
inverse inertia J H^-1 J^T of one foot -- the mobility of that foot, the inverse of the operational-space inertia an impedance
or natural-gradient term would use -- with J the foot's Jacobian, made of the motion axes of the dofs that move it
(Model.link_dof_mask).

The Ant starts in the air, so the environment first runs --settle steps without actions until the feet are on the ground.  Every
iteration then runs an H-step rollout with the policy in the loop from that same state (so that the printed losses are values
of one objective); after each env.step the mass matrix, its inverse and the motion axes of the new state are read from the
differentiable read-out, and energy_weight * kinetic energy - mobility_weight * trace(J Hinv J^T) (mean over environments and
steps) is added to the negative discounted reward.  The gradient reaches the actor through the adjoint of the read-out and of the
steps.  With --graph the whole rollout (policy, env.step, read-out, loss, backward) is one HIP-graph submission per iteration.

    python examples/inertia_lite.py --graph
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def foot_jacobian_mask(model, foot=None):
    """[nd] float: 1 for the dofs that move the foot link (default: the last link no other link hangs on), the row of
    Model.link_dof_mask -- made once, outside a capture"""
    t = model.template()
    parent = set(int(p) for p in t.joint_parent)
    feet = [i for i in range(t.n_links) if i not in parent]
    return model.link_dof_mask[feet[-1] if foot is None else foot].to(torch.float32)

def settle(env, steps):
    """`steps` env.step calls without actions and without gradients (the Ant lands on its feet), then a snapshot of the state
    for start_from"""
    with torch.no_grad():
        zero = torch.zeros((env.num_envs, env.num_actions), device=env.state.joint_q.device)
        for _ in range(steps):
            env.step(zero)
        return (env.state.joint_q.detach().clone(), env.state.joint_qd.detach().clone(), env.actions.detach().clone(),
                env.progress_buf.clone())


def start_from(env, snap):
    """puts the environment back to a snapshot of settle (what GraphedRollout does before every replay)"""
    st = type(env.state)(act_like=env.model.joint_qd, model=env.model)
    st.joint_q, st.joint_qd = snap[0].clone(), snap[1].clone()
    env.state, env.actions, env.progress_buf = st, snap[2].clone(), snap[3].clone()


def rollout_loss(env, policy, horizon, jmask, gamma=0.99, energy_weight=0.01, mobility_weight=0.01, stat=None):
    """-discounted reward + energy_weight * kinetic energy - mobility_weight * trace(J Hinv J^T) of one rollout from the env's
    start state; policy(obs, t) -> actions, jmask: the mask of foot_jacobian_mask.  No host synchronisation: capturable by
    GraphedRollout.  stat (optional, [3]): receives the loss, the mean kinetic energy and the mean mobility."""
    n = env.num_envs
    dev = env.state.joint_q.device
    obs = env.initialize_trajectory()
    disc = torch.ones(n, device=dev)
    total, energy, mobility = 0.0, 0.0, 0.0
    for t in range(horizon):
        obs, rew, done, info = env.step(policy(obs, t))
        H, Hinv, S = env.model.mass_matrix(env.state)
        qd = env.state.joint_qd.view(n, -1)
        energy = energy + 0.5 * torch.einsum("bi,bij,bj->b", qd, H, qd).sum()
        J = (jmask.view(1, -1, 1) * S.view(n, -1, 6)).transpose(1, 2)            # [n, 6, nd]
        mobility = mobility + torch.einsum("bki,bij,bkj->b", J, Hinv, J).sum()   # trace(J Hinv J^T)
        total = total - (disc * rew).sum()
        disc = torch.where(done.bool(), torch.ones_like(disc), disc * gamma)   # restart the discount with the episode
    loss = (total + energy_weight * energy - mobility_weight * mobility) / (n * horizon)
    if stat is not None:
        stat.copy_(torch.stack([loss.detach(), energy.detach() / (n * horizon), mobility.detach() / (n * horizon)]))
    return loss


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--energy-weight", type=float, default=0.01)
    ap.add_argument("--mobility-weight", type=float, default=0.01)
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    from diffrl_amd import envs
    from diffrl_amd.graph import GraphedRollout
    torch.manual_seed(a.seed)
    env = envs.AntEnv(num_envs=a.envs, device="cuda:0", no_grad=False, stochastic_init=False, MM_caching_frequency=16,
                      early_termination=False, episode_length=1000, seed=a.seed)
    dev = torch.device("cuda:0")
    actor = torch.nn.Sequential(torch.nn.Linear(env.num_obs, 128), torch.nn.ELU(), torch.nn.Linear(128, 64), torch.nn.ELU(),
                                torch.nn.Linear(64, env.num_actions)).to(dev)
    opt = torch.optim.Adam(actor.parameters(), lr=a.lr, betas=(0.7, 0.95), capturable=a.graph)
    stat = torch.zeros(3, device=dev)     # loss, mean kinetic energy and mean foot mobility of the last rollout

    env.reset()
    snap = settle(env, a.settle)
    jmask = foot_jacobian_mask(env.model)

    def body(e):
        return rollout_loss(e, lambda obs, t: torch.tanh(actor(obs)), a.horizon, jmask, a.gamma, a.energy_weight, a.mobility_weight, stat)

    roll = GraphedRollout(env, body, leaves=list(actor.parameters()), carry_state=False) if a.graph else None
    hist = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        if roll is not None:
            roll.replay()
        else:
            opt.zero_grad(set_to_none=True)
            start_from(env, snap)
            body(env).backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 1.0)
        opt.step()
        hist.append(stat.clone())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    hist = torch.stack(hist).cpu().tolist()
    print("loss: first iteration %.6f, last iteration %.6f; kinetic energy %.4f -> %.4f; foot mobility %.4f -> %.4f; "
          "%.1f ms per iteration (%s)" % (hist[0][0], hist[-1][0], hist[0][1], hist[-1][1], hist[0][2], hist[-1][2],
                                          el / a.iters * 1e3, "graph" if a.graph else "eager"))
    return hist


if __name__ == "__main__":
    main()
