"""System identification through env.step: fit the simulator to recorded OBSERVATIONS.  An Ant is driven for H steps by a fixed
action sequence under "true" parameters -- the friction coefficient mu of every ground contact and the joint damping
joint_target_kd scaled away from the model's values -- and only what a policy would see is recorded: the observation of every
step.  Starting from the model's own values, the two scales are recovered by Adam from the squared distance to the recording.
Nothing leaves the fused path: env.set_step_parameters(p) puts the values on the model, env.step() is one launch each way, and its
adjoint (dsim_env_step_backward_params) returns the parameter gradient of every step, which autograd sums over the rollout and
carries back to the two scales.  examples/sysid_lite.py does the same at the operator level, from recorded joint states.

The Ant starts in the air, so the environment first runs --settle steps without actions until the feet are on the ground.  With
--graph the whole rollout (building the parameter tensors from the two scales, setting them, H steps, loss, backward) is one
HIP-graph submission per iteration: the values are set inside the graph, so the optimiser's in-place updates are seen by the next
replay.

    python examples/sysid_env_lite.py --graph
"""
import argparse
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from sysid_lite import scaled, settle, start_from  # noqa: E402


def rollout(env, params, actions):
    """sets the parameters, then H env.step calls from the env's current state: observations [H, n, n_obs]"""
    env.set_step_parameters(params)
    return torch.stack([env.step(a)[0] for a in actions])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--true-mu-scale", type=float, default=1.5)
    ap.add_argument("--true-kd-scale", type=float, default=2.0)
    ap.add_argument("--settle", type=int, default=12)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    from diffrl_amd import envs
    from diffrl_amd.graph import GraphedRollout
    torch.manual_seed(a.seed)
    dev = torch.device("cuda:0")
    env = envs.AntEnv(num_envs=a.envs, device="cuda:0", no_grad=False, stochastic_init=False, MM_caching_frequency=16,
                      early_termination=False, episode_length=1000, seed=a.seed)
    env.reset()
    snap = settle(env, a.settle)
    actions = 2.0 * torch.rand((a.horizon, env.num_envs, env.num_actions), device=dev) - 1.0

    base = env.model.step_parameters()
    true = torch.log(torch.tensor([a.true_mu_scale, a.true_kd_scale], device=dev))
    with torch.no_grad():   # the recording
        start_from(env, snap)
        obs_ref = rollout(env, scaled(base, true), actions)
    theta = torch.zeros(2, device=dev, requires_grad=True)   # log-scales of (mu, joint_target_kd): the model's own values
    opt = torch.optim.Adam([theta], lr=a.lr, capturable=a.graph)
    stat = torch.zeros(1, device=dev)

    def body(e):
        loss = ((rollout(e, scaled(base, theta), actions) - obs_ref) ** 2).mean()
        stat.copy_(loss.detach().view(1))
        return loss

    start_from(env, snap)
    roll = GraphedRollout(env, body, leaves=[theta], carry_state=False) if a.graph else None
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
        opt.step()
        hist.append(torch.cat([stat, torch.exp(theta.detach())]))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    env.set_step_parameters(None)
    hist = torch.stack(hist).cpu().tolist()
    print("loss: first iteration %.6e, last iteration %.6e; mu scale %.3f (true %.3f), joint_target_kd scale %.3f (true %.3f); "
          "%.1f ms per iteration (%s)" % (hist[0][0], hist[-1][0], hist[-1][1], a.true_mu_scale, hist[-1][2], a.true_kd_scale,
                                          el / a.iters * 1e3, "graph" if a.graph else "eager"))
    return hist


if __name__ == "__main__":
    main()
