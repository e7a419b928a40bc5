"""System identification: fit the simulator to recorded motion.  An Ant is driven open loop for H steps by a fixed action sequence
under "true" parameters -- the friction coefficient mu of every ground contact and the joint damping joint_target_kd scaled away
from the model's values -- and the trajectory (q, qd) is recorded.  Starting from the model's own values, the two scales are
recovered by Adam from the squared distance to the recording: the step is differentiable in its parameters
(SemiImplicitIntegrator.forward(..., params=p), Model.step_parameters()), so the gradient reaches the scales through the parameter
adjoint of every step and, through the state adjoint, through all the steps behind it.

The Ant starts in the air, so the environment first runs --settle steps without actions until the feet are on the ground.  With
--graph the whole rollout (building the parameter tensors from the two scales, H steps, loss, backward) is one HIP-graph submission
per iteration: the parameter tensors are rebuilt inside the graph, so the optimiser's in-place updates are seen by the next replay.

    python examples/sysid_lite.py --graph
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def settle(env, steps):
    """`steps` env.step calls without actions and without gradients (the Ant lands on its feet), then a snapshot of the state"""
    with torch.no_grad():
        zero = torch.zeros((env.num_envs, env.num_actions), device=env.state.joint_q.device)
        for _ in range(steps):
            env.step(zero)
        return (env.state.joint_q.detach().clone(), env.state.joint_qd.detach().clone(), env.actions.detach().clone(),
                env.progress_buf.clone())


def start_from(env, snap):
    st = type(env.state)(act_like=env.model.joint_qd, model=env.model)
    st.joint_q, st.joint_qd = snap[0].clone(), snap[1].clone()
    env.state, env.actions, env.progress_buf = st, snap[2].clone(), snap[3].clone()


def scaled(base, log_scales):
    """the model's parameters with mu and joint_target_kd multiplied by exp(log_scales): a StepParameters whose tensors carry the
    graph back to log_scales"""
    s = torch.exp(log_scales)
    one = torch.ones(3, device=log_scales.device)
    p = type(base)(**{k: getattr(base, k) for k in base.FIELDS})
    p.contact_material = base.contact_material * torch.cat([one, s[0:1]]).view(1, 4)
    p.joint_target_kd = base.joint_target_kd * s[1]
    return p


def rollout(env, params, joint_acts):
    """open loop from the env's current state: [H, n, n_q] and [H, n, n_qd]"""
    st, n = env.state, env.num_envs
    qs, qds = [], []
    for a in joint_acts:
        st.joint_act = a
        st = env.integrator.forward(env.model, st, env.sim_dt, env.sim_substeps, env.MM_caching_frequency, params=params)
        qs.append(st.joint_q.view(n, -1))
        qds.append(st.joint_qd.view(n, -1))
    env.state = st
    return torch.stack(qs), torch.stack(qds)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--true-mu-scale", type=float, default=1.5)
    ap.add_argument("--true-kd-scale", type=float, default=2.0)
    ap.add_argument("--qd-weight", type=float, default=0.01)
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
    n, nd = env.num_envs, env.model.dofs_per_articulation
    acts = torch.zeros((a.horizon, n, nd), device=dev)
    acts[:, :, 6:] = (2.0 * torch.rand((a.horizon, n, env.num_actions), device=dev) - 1.0) * env.action_strength
    joint_acts = [acts[t].reshape(-1) for t in range(a.horizon)]

    base = env.model.step_parameters()
    true = torch.log(torch.tensor([a.true_mu_scale, a.true_kd_scale], device=dev))
    with torch.no_grad():   # the recording
        start_from(env, snap)
        q_ref, qd_ref = rollout(env, scaled(base, true), joint_acts)
    theta = torch.zeros(2, device=dev, requires_grad=True)   # log-scales of (mu, joint_target_kd): the model's own values
    opt = torch.optim.Adam([theta], lr=a.lr, capturable=a.graph)
    stat = torch.zeros(1, device=dev)

    def body(e):
        q, qd = rollout(e, scaled(base, theta), joint_acts)
        loss = ((q - q_ref) ** 2).mean() + a.qd_weight * ((qd - qd_ref) ** 2).mean()
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
    env.model.engine().reset_params()
    hist = torch.stack(hist).cpu().tolist()
    print("loss: first iteration %.6e, last iteration %.6e; mu scale %.3f (true %.3f), joint_target_kd scale %.3f (true %.3f); "
          "%.1f ms per iteration (%s)" % (hist[0][0], hist[-1][0], hist[-1][1], a.true_mu_scale, hist[-1][2], a.true_kd_scale,
                                          el / a.iters * 1e3, "graph" if a.graph else "eager"))
    return hist


if __name__ == "__main__":
    main()
