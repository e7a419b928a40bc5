"""Records tests/golden/<env>_mass.npz: gradients of the reference simulator's joint-space inertia model.H and motion axes
State.joint_S_s with respect to joint_q, the fixtures of the differentiable mass matrix read-out (dsim_mass_matrix_backward).
Needs the reference checkout (it imports oracle/ref_harness.py and oracle/gen_golden.py, which load it at run time); what it
writes is recorded numbers only.

    python tools/gen_mass_golden.py [env ...]

Recipe, per model (q = q_in of tests/golden/<env>_step.npz, qd = act = 0, B states, a private Tape per run):
  * integrator._simulate(tape, model, s_in, s1, h, update_mass_matrix=True); model.H and s1.joint_S_s must equal sub_H and
    sub_S_s of the step fixture bit for bit (the forward references of the tests are those two arrays, not copies here);
  * tape.adjoints[model.H] = W and / or tape.adjoints[s1.joint_S_s] = W_S, tape.replay(), read tape.adjoints[s_in.joint_q];
    the adjoint on joint_qd must be exactly zero;
  * seeded normal c_H, c_Hinv [B, nd, nd] (both non-symmetric) and c_S [B * nd, 6]; four sets -> gq_H, gq_Hinv, gq_S, gq_all.
    The reference keeps no inverse on its tape (it factorises H + diag(armature) inside its solve), so a cotangent on
    Hinv = (H + diag(armature))^-1 is carried to model.H by the rule of the inverse: W = -Hi c_Hinv Hi, Hi the float64 inverse
    of that run's own H + diag(joint_armature) (Hi is symmetric, so no transposes appear);
  * noise_gq_<set> [B]: K = 8 runs with q moved by +-1 ulp (random signs), W recomputed per run: per state the max deviation of
    its row after project_tangent, over the max-norm of the base tensor -- the reference's own fp32 noise on the scale of THAT
    set (the method of tools/gen_dynamics_golden.py).
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
SEED, K_NOISE = 29, 8
SETS = (("H", ("H",)), ("Hinv", ("Hinv",)), ("S", ("S",)), ("all", ("H", "Hinv", "S")))


def ulp_moved(a, rs):
    sgn = rs.choice([-1.0, 1.0], size=a.shape).astype(np.float32)
    return np.nextafter(a, a + sgn * np.float32(1.0)).astype(np.float32)


def row_noise(runs, base):
    """[B]: max deviation of each state's row over the runs / max-norm of the whole base tensor"""
    B = base.shape[0]
    b = np.asarray(base, np.float64).reshape(B, -1)
    dev = np.max([np.abs(np.asarray(r, np.float64).reshape(B, -1) - b).max(axis=1) for r in runs], axis=0)
    return dev / (np.abs(b).max() + 1e-30)


def record(df, envs, G, name):
    import torch
    from oracle_lib import project_tangent, template_from_golden
    g = np.load(os.path.join(OUT, name + "_step.npz"))
    arm = np.diag(np.load(os.path.join(OUT, name + "_model.npz"))["joint_armature"].astype(np.float64))
    t = template_from_golden(name)
    q = g["q_in"]
    B = q.shape[0]
    env = G.make_env(envs, name, B, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    nd = model.joint_dof_count // B
    gen = torch.Generator().manual_seed(SEED)
    c = dict(H=torch.randn(B, nd, nd, generator=gen).numpy(), Hinv=torch.randn(B, nd, nd, generator=gen).numpy(),
             S=torch.randn(B * nd, 6, generator=gen).numpy())
    out = dict(c_H=c["H"], c_Hinv=c["Hinv"], c_S=c["S"])

    def run(qv, keys, check=False):
        s_in, s1 = model.state(), model.state()
        s_in.joint_q = torch.tensor(qv.reshape(-1), dtype=torch.float32, requires_grad=True)
        s_in.joint_qd = torch.zeros(B * nd, requires_grad=True)
        s_in.joint_act = torch.zeros(B * nd)
        tape = df.adjoint.Tape()
        integ._simulate(tape, model, s_in, s1, env.sim_dt / env.sim_substeps, update_mass_matrix=True)
        H = model.H.detach().numpy().copy().reshape(B, nd, nd)
        if check:
            assert np.array_equal(H, g["sub_H"].reshape(B, nd, nd))
            assert np.array_equal(s1.joint_S_s.detach().numpy().reshape(g["sub_S_s"].shape), g["sub_S_s"])
        A = np.zeros((B, nd, nd))
        if "H" in keys:
            A += c["H"]
        if "Hinv" in keys:
            for b in range(B):
                Hi = np.linalg.inv(H[b].astype(np.float64) + arm)
                A[b] -= Hi @ c["Hinv"][b].astype(np.float64) @ Hi
        if "H" in keys or "Hinv" in keys:
            tape.adjoints[model.H] = torch.tensor(A.reshape(-1).astype(np.float32))
        if "S" in keys:
            tape.adjoints[s1.joint_S_s] = torch.tensor(c["S"].copy())
        tape.replay()
        gqd = tape.adjoints.get(s_in.joint_qd)
        assert gqd is None or not gqd.numpy().any()
        return tape.adjoints[s_in.joint_q].numpy().copy().reshape(B, -1)

    moved = [ulp_moved(q, np.random.RandomState(100 + k)) for k in range(K_NOISE)]
    for tag, keys in SETS:
        out["gq_" + tag] = run(q, keys, check=True)
        base = project_tangent(t, q, out["gq_" + tag])
        out["noise_gq_" + tag] = row_noise([project_tangent(t, q, run(qk, keys)) for qk in moved], base)
    assert all(np.isfinite(v).all() for v in out.values())
    print("%-9s B=%d nd=%d  noise " % (name, B, nd) + "  ".join(
        "%s %.1e" % (tag, out["noise_gq_" + tag].max()) for tag, _ in SETS), flush=True)
    return {k: np.asarray(v, np.float32) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        np.savez_compressed(os.path.join(OUT, name + "_mass.npz"), **record(df, envs, G, name))


if __name__ == "__main__":
    main(sys.argv[1:])
