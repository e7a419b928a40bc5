"""Records tests/golden/<env>_lin.npz: the reference simulator's Jacobian of one env-step, the fixtures of the step Jacobian
(dsim_step_backward_multi / dsim_step_jacobian).  Needs the reference checkout (it imports oracle/ref_harness.py and
oracle/gen_golden.py, which load it at run time); what it writes is recorded numbers only.

    python tools/gen_linearise_golden.py [env ...]

Recipe, per model (inputs: the first B = 2 states q_in, qd_in, act_in / muscle_act_in of tests/golden/<env>_step.npz with that
fixture's dt, substeps and mm_freq; K = n_q + n_qd):
  * the reference runs ONCE on B * K replicated environments: environment (b, k) = b * K + k starts from state b and receives
    the one-hot cotangent e_k on (q_out | qd_out) -- the loss is sum_{b,k} out[b * K + k][k].  The reference's environments
    are independent, so its one backward pass is K backward passes per state: row k of the gradients of environment (b, k)
    is row k of the Jacobian of state b;
  * recorded blocks: J_qq [B][n_q][n_q] = d q_out / d q_in, J_q_qd [B][n_q][n_qd] = d q_out / d qd_in, J_qd_q [B][n_qd][n_q],
    J_qd_qd [B][n_qd][n_qd], J_act [B][K][n_qd] and, for the muscle model, J_muscle [B][K][M] (its J_act is recorded too:
    the joint actuation is an input of that model as well, held at zero);
  * noise_<block> (a scalar each): the same run from (q, qd) moved by +-1 ulp, 4 sign patterns (every replica of a state gets the
    state's own pattern): the largest deviation of the block over the patterns and states divided by the block's own max-norm
    (the q_in columns after project_tangent) -- the reference's own fp32 noise, in the norm the tests compare in;
  * states: the row indices of the step fixture that were used (SNUHumanoid: one state if two do not fit 100 KB).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("ant", "humanoid", "snu", "hopper", "cartpole", "cheetah")
BLOCKS = ("J_qq", "J_q_qd", "J_qd_q", "J_qd_qd", "J_act", "J_muscle")
N_PATTERNS, MAX_BYTES = 4, 100 * 1000


def ulp_moved(a, rs):
    sgn = rs.choice([-1.0, 1.0], size=a.shape).astype(np.float32)
    return np.nextafter(a, a + sgn * np.float32(1.0)).astype(np.float32)


def split(t, q, gq, gqd, ga, gm, B):
    """gradients of the B * K environments -> the Jacobian blocks (q_in columns projected onto the tangent space)"""
    from oracle_lib import project_tangent
    nq, nd = t.n_q, t.n_qd
    K = nq + nd
    gq = project_tangent(t, np.repeat(q, K, axis=0), gq).reshape(B, K, nq)
    gqd, ga = gqd.reshape(B, K, nd), ga.reshape(B, K, nd)
    out = dict(J_qq=gq[:, :nq], J_q_qd=gqd[:, :nq], J_qd_q=gq[:, nq:], J_qd_qd=gqd[:, nq:], J_act=ga)
    if gm is not None:
        out["J_muscle"] = gm.reshape(B, K, -1)
    return out


def record(df, envs, G, name, B):
    import torch
    from oracle_lib import template_from_golden
    g = np.load(os.path.join(OUT, name + "_step.npz"))
    t = template_from_golden(name)
    nq, nd = t.n_q, t.n_qd
    K = nq + nd
    N = B * K
    q, qd = g["q_in"][:B], g["qd_in"][:B]
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    env = G.make_env(envs, name, N, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    M = model.muscle_count // N
    assert model.joint_coord_count // N == nq and model.joint_dof_count // N == nd and abs(env.sim_dt - dt) < 1e-12
    sel = torch.zeros(N, K)   # environment (b, k) reads output coordinate k
    sel[torch.arange(N), torch.arange(N) % K] = 1.0

    def run(qv, qdv):
        st = model.state()
        st.joint_q = torch.tensor(np.repeat(qv, K, axis=0).reshape(-1), dtype=torch.float32, requires_grad=True)
        st.joint_qd = torch.tensor(np.repeat(qdv, K, axis=0).reshape(-1), dtype=torch.float32, requires_grad=True)
        act = torch.tensor(np.repeat(g["act_in"][:B], K, axis=0)).clone().requires_grad_(True)
        st.joint_act = act.view(-1)
        mact = None
        if M > 0:
            mact = torch.tensor(np.repeat(g["muscle_act_in"][:B], K, axis=0)).clone().requires_grad_(True)
            model.muscle_activation = mact.view(-1)
        so = integ.forward(model, st, dt, S, mm)
        out = torch.cat([so.joint_q.view(N, nq), so.joint_qd.view(N, nd)], dim=1)
        (out * sel).sum().backward()
        z = lambda x: x.grad.numpy().copy() if x.grad is not None else np.zeros(tuple(x.shape), np.float32)  # noqa: E731
        return (split(t, qv, z(st.joint_q).reshape(N, nq), z(st.joint_qd).reshape(N, nd), z(act).reshape(N, nd),
                      z(mact).reshape(N, M) if M > 0 else None, B), so.joint_q.detach().numpy().reshape(N, nq)[::K].copy())

    base, q_out = run(q, qd)
    assert np.array_equal(q_out, g["q_out"][:B]), "the replicated environments do not reproduce the step fixture"
    out = {k: np.asarray(v, np.float32) for k, v in base.items()}
    dev = {k: 0.0 for k in base}
    for p in range(N_PATTERNS):
        rs = np.random.RandomState(300 + p)
        r, _ = run(ulp_moved(q, rs), ulp_moved(qd, rs))
        for k in base:
            dev[k] = max(dev[k], float(np.abs(np.asarray(r[k], np.float64) - np.asarray(base[k], np.float64)).max()))
    for k in base:
        out["noise_" + k] = np.float32(dev[k] / (np.abs(base[k]).max() + 1e-30))
    out["states"] = np.arange(B, dtype=np.int32)
    assert all(np.isfinite(v).all() for v in out.values())
    print("%-9s B=%d K=%d  noise " % (name, B, K) + "  ".join("%s %.1e" % (k, out["noise_" + k]) for k in BLOCKS if k in base),
          flush=True)
    return out


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        path = os.path.join(OUT, name + "_lin.npz")
        for B in (2, 1):
            np.savez_compressed(path, **record(df, envs, G, name, B))
            if os.path.getsize(path) <= MAX_BYTES:
                break
            print("%s: %d bytes with %d states, recording fewer" % (name, os.path.getsize(path), B), flush=True)
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print("%s: %d bytes" % (path, os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
