"""Domain randomisation per environment: the loop of examples/shac_lite.py on Ant, every environment with ground friction and joint
PD gains of its own (DFlexEnv.randomize_step_parameters: the template's values times one uniform factor per environment and
field).  The population is ONE fused launch per env.step all the same, and with --graph the whole rollout (policy, env.step, loss,
backward) stays one HIP-graph submission per iteration: the parameter values live in a per-environment block on the device that
the captured launches read.

    python examples/domain_rand_lite.py --envs 256 --iters 60 --graph
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--spread", type=float, default=0.5, help="factors are drawn from [1 - spread, 1 + spread)")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    from diffrl_amd import envs
    from diffrl_amd.graph import GraphedRollout
    torch.manual_seed(a.seed)
    env = envs.AntEnv(num_envs=a.envs, device="cuda:0", no_grad=False, stochastic_init=True, MM_caching_frequency=16,
                      episode_length=1000, seed=a.seed)
    dev = torch.device("cuda:0")
    # one draw per environment, before anything is captured (the first call reserves the per-environment block)
    rng = (1.0 - a.spread, 1.0 + a.spread)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    p = env.randomize_step_parameters({"contact_material": {"mu": rng, "kf": rng}, "joint_target_ke": rng, "joint_target_kd": rng},
                                      generator=gen)
    mu = p.contact_material[:, :, 3]
    print("friction coefficient of the first contact over the environments: %.3f .. %.3f" % (float(mu[:, 0].min()), float(mu[:, 0].max())))
    actor = torch.nn.Sequential(torch.nn.Linear(env.num_obs, 128), torch.nn.ELU(), torch.nn.Linear(128, 64), torch.nn.ELU(),
                                torch.nn.Linear(64, env.num_actions)).to(dev)
    opt = torch.optim.Adam(actor.parameters(), lr=a.lr, betas=(0.7, 0.95), capturable=a.graph)
    H, n = a.horizon, a.envs
    stat = torch.zeros(2, device=dev)     # loss and mean reward per step of the last rollout

    def body(e):
        obs = e.initialize_trajectory()
        disc = torch.ones(n, device=dev)
        total, rsum = 0.0, 0.0
        for t in range(H):
            obs, rew, done, info = e.step(torch.tanh(actor(obs)))
            total = total - (disc * rew).sum()
            rsum = rsum + rew.detach().mean()
            disc = torch.where(done.bool(), torch.ones_like(disc), disc * a.gamma)   # restart the discount with the episode
        loss = total / (n * H)
        stat.copy_(torch.stack([loss.detach(), rsum / H]))
        return loss

    env.reset()
    roll = GraphedRollout(env, body, leaves=list(actor.parameters()), carry_state=True) if a.graph else None
    hist = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        if roll is not None:
            roll.replay()
        else:
            opt.zero_grad(set_to_none=True)
            body(env).backward()
        torch.nn.utils.clip_grad_norm_(actor.parameters(), 1.0)
        opt.step()
        hist.append(stat.clone())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    hist = torch.stack(hist).cpu().tolist()
    k = max(1, a.iters // 6)
    print("loss: first %d iters %.4f, last %d iters %.4f; mean reward/step %.3f -> %.3f; %.1f ms per iteration (%s), %.2e env-steps/s"
          % (k, sum(h[0] for h in hist[:k]) / k, k, sum(h[0] for h in hist[-k:]) / k, hist[0][1], hist[-1][1], el / a.iters * 1e3,
             "graph" if a.graph else "eager", a.iters * n * H / el))
    env.model.engine().reset_params()
    return hist


if __name__ == "__main__":
    main()
