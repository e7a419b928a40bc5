"""Gradient-growth diagnostic: the step Jacobians A_t = d (q', qd') / d (q, qd) along an Ant rollout with random actions.

Every step is SemiImplicitIntegrator.linearize -- one forward launch that keeps its checkpoint and one Jacobian launch of
num_envs * (n_q + n_qd) workgroups.  Per step the largest singular value of A_t and of the running product A_t ... A_1 (median
and maximum over the environments) is printed: where the product grows, a short-horizon gradient through those steps does too.
The numbers are a read-out; nothing is claimed about them beyond being finite.  With --graph the whole rollout (every forward
and Jacobian launch) is captured once and replayed as one HIP-graph submission; the singular values are computed from the
replay's Jacobians afterwards.

    python examples/jacobian_lite.py --graph
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    from diffrl_amd import envs
    dev = torch.device("cuda:0")
    env = envs.AntEnv(num_envs=a.envs, device="cuda:0", no_grad=True, stochastic_init=False, MM_caching_frequency=16,
                      early_termination=False, episode_length=1000, seed=a.seed)
    env.reset()
    model, integ = env.model, env.integrator
    n, T = a.envs, a.steps
    nq, nd = model.coords_per_articulation, model.dofs_per_articulation
    K = nq + nd
    gen = torch.Generator().manual_seed(a.seed)
    actions = torch.tanh(2.0 * torch.rand((T, n, env.num_actions), generator=gen) - 1.0).to(dev)
    # the free root is not actuated; the env's own action scaling
    joint_act = torch.cat([torch.zeros((T, n, nd - env.num_actions), device=dev), actions * env.action_strength], dim=2)
    q0, qd0 = env.state.joint_q.detach().clone(), env.state.joint_qd.detach().clone()
    A_all = torch.zeros((T, n, K, K), device=dev)

    def rollout():
        q, qd = q0, qd0
        for t in range(T):
            st = model.state()
            st.joint_q, st.joint_qd, st.joint_act = q, qd, joint_act[t].reshape(-1)
            out, A, B = integ.linearize(model, st, env.sim_dt, env.sim_substeps, env.MM_caching_frequency)
            A_all[t].copy_(A)
            q, qd = out.joint_q, out.joint_qd

    if a.graph:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            rollout()   # warm-up, as torch.cuda.graph requires
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            rollout()
        A_all.zero_()
        graph.replay()
    else:
        rollout()
    torch.cuda.synchronize(dev)
    model.engine().status()

    A = A_all.cpu().double()
    P = torch.eye(K, dtype=torch.float64).expand(n, K, K).clone()
    print("Ant, %d environments, %d steps, random actions (%s)" % (n, T, "graph replay" if a.graph else "eager"))
    print("step  sigma_max(A_t) median / max    sigma_max(A_t ... A_1) median / max")
    rows = []
    for t in range(T):
        P = A[t] @ P
        s1, sp = torch.linalg.matrix_norm(A[t], ord=2), torch.linalg.matrix_norm(P, ord=2)
        rows.append((float(s1.median()), float(s1.max()), float(sp.median()), float(sp.max())))
        print("%4d  %12.4e / %-12.4e    %12.4e / %-12.4e" % ((t + 1,) + rows[-1]))
    assert all(torch.isfinite(torch.tensor(r)).all() for r in rows), "non-finite Jacobian"
    return rows


if __name__ == "__main__":
    main()
