"""Reaching with a link frame: open-loop actions of an Ant are optimised through the differentiable simulator so that one foot
moves to a target point -- a loss written on a LINK's pose and twist (Model.body_kinematics), not on the joint coordinates.

Every iteration runs H env.steps from the same start state; after each step the foot's frame X_sc and spatial twist v_s are
read from the state, and the loss is the mean squared distance of the foot to the target plus a small penalty on the velocity
of that point.  Its gradient reaches the actions through the adjoint of the kinematics and of the steps.  With --graph the
whole rollout (H steps, kinematics, loss, backward) is one HIP-graph submission per iteration.

    python examples/reach_lite.py --envs 64 --horizon 16 --iters 30 --graph
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
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--link", type=int, default=2, help="the link that reaches (Ant: 2 = lower link of the first leg)")
    ap.add_argument("--vel-penalty", type=float, default=1e-3)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    from diffrl_amd import envs
    from diffrl_amd.graph import GraphedRollout
    torch.manual_seed(a.seed)
    dev = torch.device("cuda:0")
    n, H = a.envs, a.horizon
    env = envs.AntEnv(num_envs=n, device="cuda:0", no_grad=False, stochastic_init=False, MM_caching_frequency=16,
                      early_termination=False, episode_length=1000, seed=a.seed)
    env.reset()
    L = env.model.links_per_articulation
    with torch.no_grad():   # the target: 15 cm above and 10 cm ahead of where the foot starts
        p0 = env.model.body_kinematics(env.state)[0].view(n, L, 7)[:, a.link, :3].clone()
    target = p0 + torch.tensor([0.10, 0.15, 0.0], device=dev)
    u = torch.zeros((H, n, env.num_actions), device=dev, requires_grad=True)   # actions = tanh(u)
    opt = torch.optim.Adam([u], lr=a.lr, capturable=a.graph)

    def body(e):
        e.initialize_trajectory()
        total = 0.0
        for u_t in u.unbind(0):
            e.step(torch.tanh(u_t))
            xsc, _, vs = e.model.body_kinematics(e.state)
            p = xsc.view(n, L, 7)[:, a.link, :3]
            tw = vs.view(n, L, 6)[:, a.link]
            vp = tw[:, 3:] + torch.linalg.cross(tw[:, :3], p)   # velocity of the point of the link at p: v + w x p
            total = total + (p - target).pow(2).sum() + a.vel_penalty * vp.pow(2).sum()
        return total / (n * H)

    roll = GraphedRollout(env, body, leaves=[u], carry_state=False) if a.graph else None
    hist = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(a.iters):
        if roll is not None:
            loss = roll.replay()
        else:
            opt.zero_grad(set_to_none=True)
            env.reset()
            loss = body(env)
            loss.backward()
            loss = loss.detach()
        opt.step()
        hist.append(loss.clone())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    hist = torch.stack(hist).cpu().tolist()
    for it, v in enumerate(hist):
        print("iter %3d  loss %.6f" % (it, v))
    print("loss %.6f -> %.6f in %d iterations; %.1f ms per iteration (%s)" % (hist[0], hist[-1], a.iters, el / a.iters * 1e3,
                                                                              "graph" if a.graph else "eager"))
    return hist


if __name__ == "__main__":
    main()
