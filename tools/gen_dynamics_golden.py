"""Records tests/golden/<env>_dyn.npz: the reference simulator's State.joint_tau / joint_qdd / body_f_s and their gradients,
the fixtures of the differentiable joint dynamics (dsim_joint_dynamics_backward).  Needs the reference checkout (it imports
oracle/ref_harness.py and oracle/gen_golden.py, which load it at run time); what it writes is recorded numbers only.

    python tools/gen_dynamics_golden.py [env ...]

Recipe, per model (inputs: q_in, qd_in, act_in / muscle_act_in of tests/golden/<env>_step.npz, B states):
  * direct: so = integrator.forward(model, state, sim_dt / sim_substeps, 1, 1); so.joint_tau / joint_qdd / body_f_s are read
    BEFORE any backward pass (the reference's tape replay re-executes the contact atomic_adds into body_f_s) and must equal
    sub_tau / sub_qdd / sub_f_s of the step fixture bit for bit; seeded normal cotangents c_tau, c_qdd, c_fs; four backward
    passes -- each tensor alone, then all three -- -> gq_*, gqd_*, gact_* (gmact_* for the muscle model);
  * noise_gq / noise_gqd / noise_gact (noise_gmact) [B]: K = 8 copies of (q, qd) moved by +-1 ulp (random signs), all three
    cotangents together: per state the max deviation of its row over the K runs, divided by the max-norm of the whole base
    tensor (gq after project_tangent) -- the reference's own fp32 noise; noise_<t>_<set> [B] for set = tau, qdd, fs: the same
    for each single-cotangent run, on the scale of THAT run's base tensor (the three gradients are parts of a sum that cancel:
    a part's noise relative to its own size is not the sum's);
  * composite: so1 = forward(model, state, sim_dt, substeps, mm_freq), so1.joint_act = state.joint_act (the muscle activations
    stay on the model), so2 = forward(model, so1, sim_dt / substeps, 1, 1) and the same loss on so2's three tensors: comp_tau,
    comp_qdd, comp_f_s, comp_gq_in, comp_gqd_in, comp_gact (comp_gmuscle_act), and the same +-1 ulp noise of the three forward
    tensors and the three gradients: comp_noise_<name> [B].
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
KEYS = ("joint_tau", "joint_qdd", "body_f_s")
SEED, K_NOISE = 23, 8
SETS = (("tau", KEYS[:1]), ("qdd", KEYS[1:2]), ("fs", KEYS[2:]), ("all", KEYS))


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
    t = template_from_golden(name)
    q, qd = g["q_in"], g["qd_in"]
    B = q.shape[0]
    env = G.make_env(envs, name, B, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    L, nd, M = model.link_count // B, model.joint_dof_count // B, model.muscle_count // B
    a_in = g["muscle_act_in"] if M > 0 else g["act_in"]
    atag = "gmact" if M > 0 else "gact"
    gen = torch.Generator().manual_seed(SEED)
    cs = {k: torch.randn(n, generator=gen) for k, n in zip(KEYS, ((B * nd,), (B * nd,), (B * L, 6)))}
    out = dict(c_tau=cs[KEYS[0]].numpy().reshape(B, nd), c_qdd=cs[KEYS[1]].numpy().reshape(B, nd),
               c_fs=cs[KEYS[2]].numpy().reshape(B, L, 6))
    S, mm = int(g["substeps"]), int(g["mm_freq"])

    def start(qv, qdv):
        st = model.state()
        st.joint_q = torch.tensor(qv.reshape(-1), dtype=torch.float32, requires_grad=True)
        st.joint_qd = torch.tensor(qdv.reshape(-1), dtype=torch.float32, requires_grad=True)
        act = torch.tensor(a_in).clone().requires_grad_(True)
        if M > 0:
            model.muscle_activation = act.view(-1)
            st.joint_act = torch.zeros(B * nd)
        else:
            st.joint_act = act.view(-1)
        return st, act

    def finish(so, st, act, keys):
        fwd = [getattr(so, k).detach().numpy().copy() for k in KEYS]   # before the backward pass
        sum((getattr(so, k) * cs[k]).sum() for k in keys).backward()
        z = lambda x, like: x.grad.numpy().copy() if x.grad is not None else np.zeros(like.shape, np.float32)  # noqa: E731
        return (z(st.joint_q, st.joint_q).reshape(B, -1), z(st.joint_qd, st.joint_qd).reshape(B, -1), z(act, act).reshape(B, -1), fwd)

    def direct(qv, qdv, keys):
        st, act = start(qv, qdv)
        return finish(integ.forward(model, st, env.sim_dt / env.sim_substeps, 1, 1), st, act, keys)

    def composite(qv, qdv):
        st, act = start(qv, qdv)
        so1 = integ.forward(model, st, env.sim_dt, S, mm)
        so1.joint_act = st.joint_act
        r = finish(integ.forward(model, so1, env.sim_dt / S, 1, 1), st, act, KEYS)
        return r + (so1.joint_q.detach().numpy().reshape(B, -1).copy(),)

    for tag, keys in SETS:
        out["gq_" + tag], out["gqd_" + tag], out[atag + "_" + tag], fw = direct(q, qd, keys)
        assert np.array_equal(fw[0].reshape(B, nd), g["sub_tau"]) and np.array_equal(fw[1].reshape(B, nd), g["sub_qdd"])
        assert np.array_equal(fw[2].reshape(B, L, 6), g["sub_f_s"].reshape(B, L, 6))
    cq, cqd, ca, cf, q1 = composite(q, qd)
    assert np.array_equal(q1, g["q_out"])
    out.update(comp_tau=cf[0].reshape(B, nd), comp_qdd=cf[1].reshape(B, nd), comp_f_s=cf[2].reshape(B, L, 6), comp_gq_in=cq,
               comp_gqd_in=cqd)
    out["comp_gmuscle_act" if M > 0 else "comp_gact"] = ca

    d_runs, c_runs, s_runs = [], [], {tag: [] for tag, _ in SETS[:3]}
    for k in range(K_NOISE):
        rs = np.random.RandomState(100 + k)
        q1, qd1 = ulp_moved(q, rs), ulp_moved(qd, rs)
        r = direct(q1, qd1, KEYS)
        d_runs.append((project_tangent(t, q, r[0]), r[1], r[2]))
        for tag, keys in SETS[:3]:
            r = direct(q1, qd1, keys)
            s_runs[tag].append((project_tangent(t, q, r[0]), r[1], r[2]))
        r = composite(q1, qd1)
        c_runs.append((project_tangent(t, q, r[0]), r[1], r[2]) + tuple(r[3]))
    base = (project_tangent(t, q, out["gq_all"]), out["gqd_all"], out[atag + "_all"])
    for j, nm in enumerate(("gq", "gqd", atag)):
        out["noise_" + nm] = row_noise([r[j] for r in d_runs], base[j])
    for tag, _ in SETS[:3]:   # each single-cotangent set on ITS OWN scale: the parts of the sum cancel, their noise does not
        sbase = (project_tangent(t, q, out["gq_" + tag]), out["gqd_" + tag], out[atag + "_" + tag])
        for j, nm in enumerate(("gq", "gqd", atag)):
            out["noise_%s_%s" % (nm, tag)] = row_noise([r[j] for r in s_runs[tag]], sbase[j])
    cbase = (project_tangent(t, q, cq), cqd, ca) + tuple(cf)
    for j, nm in enumerate(("gq", "gqd", atag, "tau", "qdd", "f_s")):
        out["comp_noise_" + nm] = row_noise([r[j] for r in c_runs], cbase[j])
    assert all(np.isfinite(v).all() for v in out.values())
    print("%-9s B=%d  direct noise gq %.1e gqd %.1e %s %.1e | composite fwd %.1e %.1e %.1e grad %.1e %.1e %.1e" % (
        (name, B, out["noise_gq"].max(), out["noise_gqd"].max(), atag, out["noise_" + atag].max()) +
        tuple(out["comp_noise_" + n].max() for n in ("tau", "qdd", "f_s", "gq", "gqd", atag))), flush=True)
    print("          direct gq noise per state: " + " ".join("%.1e" % v for v in out["noise_gq"]), flush=True)
    for tag, _ in SETS[:3]:
        print("          set %-3s noise per state, " % tag + "; ".join(
            "%s: %s" % (nm, " ".join("%.1e" % v for v in out["noise_%s_%s" % (nm, tag)])) for nm in ("gq", "gqd", atag)), flush=True)
    return {k: np.asarray(v, np.float32) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        np.savez_compressed(os.path.join(OUT, name + "_dyn.npz"), **record(df, envs, G, name))


if __name__ == "__main__":
    main(sys.argv[1:])
