"""Smooth locomotion: the short-horizon policy optimisation of examples/shac_lite.py with an ACCELERATION penalty -- a loss term
written on joint_qdd (Model.joint_dynamics), which no position or velocity output can express.

Every iteration runs an H-step rollout with the policy in the loop from the same start state (so that the printed losses are
values of one objective); after each env.step the joint accelerations of the new
state under the actuation just applied are read from the differentiable dynamic read-out, and 1e-4 * qdd^2 (mean over
environments and steps) is added to the negative discounted reward.  The gradient reaches the actor through the adjoint of the
read-out (state AND actuation) and of the steps.  With --graph the whole rollout (policy, env.step, read-out, loss, backward) is
one HIP-graph submission per iteration.

    python examples/smooth_lite.py --graph
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--acc-penalty", type=float, default=1e-4)
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
    H, n = a.horizon, a.envs
    stat = torch.zeros(2, device=dev)     # loss and mean squared acceleration of the last rollout
    root = torch.zeros((n, 6), device=dev)   # the free root is not actuated

    def body(e):
        obs = e.initialize_trajectory()
        disc = torch.ones(n, device=dev)
        total, acc = 0.0, 0.0
        for t in range(H):
            act = torch.tanh(actor(obs))
            obs, rew, done, info = e.step(act)
            # the fused env path keeps no joint_act tensor: the actuation to evaluate is the env's own action scaling
            joint_act = torch.cat([root, act.clamp(-1.0, 1.0) * e.action_strength], dim=1).reshape(-1)
            _, qdd, _ = e.model.joint_dynamics(e.state, joint_act=joint_act)
            total = total - (disc * rew).sum()
            acc = acc + qdd.pow(2).sum()
            disc = torch.where(done.bool(), torch.ones_like(disc), disc * a.gamma)   # restart the discount with the episode
        loss = (total + a.acc_penalty * acc) / (n * H)
        stat.copy_(torch.stack([loss.detach(), acc.detach() / (H * qdd.numel())]))
        return loss

    env.reset()
    roll = GraphedRollout(env, body, leaves=list(actor.parameters()), carry_state=False) if a.graph else None
    hist = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        if roll is not None:
            roll.replay()
        else:
            opt.zero_grad(set_to_none=True)
            env.reset()
            body(env).backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 1.0)
        opt.step()
        hist.append(stat.clone())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    hist = torch.stack(hist).cpu().tolist()
    print("loss: first iteration %.4f, last iteration %.4f; mean qdd^2 %.1f -> %.1f; %.1f ms per iteration (%s)"
          % (hist[0][0], hist[-1][0], hist[0][1], hist[-1][1], el / a.iters * 1e3, "graph" if a.graph else "eager"))
    return hist


if __name__ == "__main__":
    main()
