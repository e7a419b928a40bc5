"""Records tests/golden/<env>_par.npz: gradients of a short step of the reference simulator with respect to its MODEL tensors --
joint_target_ke / kd, joint_limit_ke / kd, joint_target, shape_materials -- the fixtures of dsim_step_backward_params.  Needs the
reference checkout (it imports oracle/ref_harness.py and oracle/gen_golden.py, which load it at run time); what it writes is
recorded numbers only.

    python tools/gen_param_golden.py [env ...]

Recipe, per model (B states, a private Tape per run):
  * start states: q_in, qd_in and the actuation of tests/golden/<env>_con.npz (penetrating contacts on both friction branches and
    both signs of the normal velocity; CartPole, which has no contacts: its <env>_step.npz states) and, for every model with
    limited hinge / slider joints, two more: copies of a start state with one such joint moved 0.05 past its upper limit and
    another 0.05 below its lower limit (`limit_state` [B] marks them);
  * requires_grad on model.joint_target_ke / kd, joint_limit_ke / kd, joint_target and shape_materials; S = 3 calls of
    integrator._simulate at the environment's own substep length h, update_mass_matrix on substeps 0 and 2 (mm_freq = 2: one
    group that re-uses a factor, one refresh); the same step for the library is dt = 3 h, substeps = 3, mm_freq = 2;
  * seeded normal cotangents gq_out, gqd_out on the final joint_q / joint_qd, tape.replay(); recorded: q_out, qd_out, gq_in,
    gqd_in, gact (muscle models: gmuscle_act) and the adjoints of the six model tensors, which the reference replicates per
    environment: g_target_ke / g_target_kd / g_limit_ke / g_limit_kd [B, L], g_target [B, n_q], g_shape_materials [B, shapes, 4];
  * coverage, asserted: every recorded parameter gradient is non-zero for every model that has the parameter, and both limit
    branches occur;
  * branches [B, S, ...]: per substep the limit flags of every coordinate and, per contact, active / friction regime / sign of vn
    (float64 statement, tests/con_lib.contacts, on the reference's own body_X_sc / body_v_s of that substep);
  * noise_<name>: K = 8 re-runs with q moved by +-1 ulp (random signs): per tensor the max deviation over the max-norm of the base
    (gq_in after project_tangent; noise_g_shape_materials_cols [4]: the same for each of the columns ke, kd, kf, mu alone).  No re-run may flip a branch: a state that does is REPLACED (by a state that keeps its
    branches, its velocities scaled by 0.9, 0.81, ... -- different states with the same regimes) and the model is recorded again, so that
    the reference alone is inside the bound on every committed state.
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
SEED, K_NOISE, S, MM = 31, 8, 3, 2
PAST = 0.05
HINGE = (0, 1)   # prismatic, revolute
PARAMS = ("target_ke", "target_kd", "limit_ke", "limit_kd", "target", "shape_materials")


def ulp_moved(a, rs):
    sgn = rs.choice([-1.0, 1.0], size=a.shape).astype(np.float32)
    return np.nextafter(a, a + sgn * np.float32(1.0)).astype(np.float32)


def tensor_noise(runs, base):
    b = np.asarray(base, np.float64)
    return np.float64(max(np.abs(np.asarray(r, np.float64) - b).max() for r in runs) / (np.abs(b).max() + 1e-30))


def limited_coords(t):
    """coordinates of hinge / slider joints with finite limits"""
    out = []
    for i in range(t.n_links):
        if int(t.joint_type[i]) in HINGE:
            c = int(t.joint_q_start[i])
            if np.isfinite(t.joint_limit_lower[c]) and np.isfinite(t.joint_limit_upper[c]) and abs(t.joint_limit_upper[c]) < 1e3 \
                    and abs(t.joint_limit_lower[c]) < 1e3:
                out.append(c)
    return out


def start_states(t, name):
    src = np.load(os.path.join(OUT, name + ("_con.npz" if t.n_contacts else "_step.npz")))
    q, qd = src["q_in"].astype(np.float32), src["qd_in"].astype(np.float32)
    a = (src["muscle_act_in"] if t.n_muscles > 0 else src["act_in"]).astype(np.float32)
    lim = np.zeros(len(q), bool)
    lc = limited_coords(t)
    if len(lc) >= 2:
        for n, b in enumerate((0, len(q) // 2)):
            up, lo = lc[(2 * n) % len(lc)], lc[(2 * n + 1) % len(lc)]
            q1 = q[b].copy()
            q1[up] = np.float32(t.joint_limit_upper[up] + PAST)
            q1[lo] = np.float32(t.joint_limit_lower[lo] - PAST)
            q, qd, a, lim = np.vstack([q, q1[None]]), np.vstack([qd, qd[b][None]]), np.vstack([a, a[b][None]]), np.append(lim, True)
    return q, qd, a, lim


def record(df, envs, G, name):
    import torch
    import con_lib
    from oracle_lib import project_tangent, template_from_golden
    t = template_from_golden(name)
    q, qd, a_in, lim = start_states(t, name)
    B = q.shape[0]
    env = G.make_env(envs, name, B, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    L, nq, nd, M = t.n_links, t.n_q, t.n_qd, t.n_muscles
    Cn, ns = t.n_contacts, model.shape_count // B
    assert model.link_count // B == L and model.joint_dof_count // B == nd
    h = env.sim_dt / float(env.sim_substeps)
    ptensors = dict(target_ke=model.joint_target_ke, target_kd=model.joint_target_kd, limit_ke=model.joint_limit_ke,
                    limit_kd=model.joint_limit_kd, target=model.joint_target, shape_materials=model.shape_materials)
    for k, v in ptensors.items():
        # (leaves of their own: the adjoints are looked up by tensor)
        ptensors[k] = v.detach().clone().requires_grad_(True)
    model.joint_target_ke, model.joint_target_kd = ptensors["target_ke"], ptensors["target_kd"]
    model.joint_limit_ke, model.joint_limit_kd = ptensors["limit_ke"], ptensors["limit_kd"]
    model.joint_target, model.shape_materials = ptensors["target"], ptensors["shape_materials"]
    gen = torch.Generator().manual_seed(SEED)
    c_q, c_qd = torch.randn(B * nq, generator=gen), torch.randn(B * nd, generator=gen)
    lower, upper = np.asarray(t.joint_limit_lower, np.float64), np.asarray(t.joint_limit_upper, np.float64)
    hinge_c = np.zeros(nq, bool)
    for i in range(L):
        if int(t.joint_type[i]) in HINGE:
            hinge_c[int(t.joint_q_start[i])] = True

    def run(qv, qdv, av):
        s = model.state()
        s.joint_q = torch.tensor(qv.reshape(-1), dtype=torch.float32, requires_grad=True)
        s.joint_qd = torch.tensor(qdv.reshape(-1), dtype=torch.float32, requires_grad=True)
        act = torch.tensor(av.reshape(-1)).clone().requires_grad_(True)   # (flat: the tape looks adjoints up by tensor)
        if M > 0:
            model.muscle_activation = act
            jact = torch.zeros(B * nd)
        else:
            jact = act
        tape = df.adjoint.Tape()
        s_in, first = s, s
        br = dict(low=[], up=[], active=[], first=[], vn_neg=[])
        for i in range(S):
            s_in.joint_act = jact
            s_out = model.state()
            integ._simulate(tape, model, s_in, s_out, h, update_mass_matrix=(i % MM) == 0)
            qi = s_in.joint_q.detach().numpy().astype(np.float64).reshape(B, nq)
            br["low"].append(hinge_c[None] & (qi < lower[None]))
            br["up"].append(hinge_c[None] & (qi > upper[None]))
            if Cn:
                X = s_out.body_X_sc.detach().numpy().astype(np.float64).reshape(B, L, 7)
                V = s_out.body_v_s.detach().numpy().astype(np.float64).reshape(B, L, 6)
                aux = [con_lib.contacts(t, X[b], V[b])[4] for b in range(B)]
                act_ = np.stack([x["active"] for x in aux])
                br["active"].append(act_)
                br["first"].append(act_ & np.stack([x["a1"] < x["a2"] for x in aux]))
                br["vn_neg"].append(act_ & np.stack([x["vn"] < 0 for x in aux]))
            s_in = s_out
        out = dict(q_out=s_in.joint_q.detach().numpy().reshape(B, nq).copy(), qd_out=s_in.joint_qd.detach().numpy().reshape(B, nd).copy())
        tape.adjoints[s_in.joint_q] = c_q.clone()
        tape.adjoints[s_in.joint_qd] = c_qd.clone()
        tape.replay()
        z = lambda x, n: tape.adjoints[x].numpy().reshape(B, -1).copy() if x in tape.adjoints else np.zeros((B, n), np.float32)  # noqa: E731
        out["gq_in"], out["gqd_in"] = z(first.joint_q, nq), z(first.joint_qd, nd)
        out["gmuscle_act" if M > 0 else "gact"] = z(act, M if M > 0 else nd)
        for k, v in ptensors.items():
            if k == "shape_materials":
                out["g_" + k] = z(v, ns * 4).reshape(B, ns, 4)
            else:
                out["g_" + k] = z(v, v.numel() // B)
        branches = {k: np.stack(v, axis=1) for k, v in br.items() if v}
        return out, branches

    moved = [ulp_moved(q, np.random.RandomState(100 + k)) for k in range(K_NOISE)]
    for attempt in range(4):
        base, br0 = run(q, qd, a_in)
        reruns = [run(qk, qd, a_in) for qk in moved]
        flip = np.zeros(B, bool)
        for _, brk in reruns:
            for k in br0:
                flip |= (brk[k] != br0[k]).reshape(B, -1).any(axis=1)
        if not flip.any():
            break
        good = int(np.nonzero(~flip & ~lim)[0][0])
        print("%-9s states %s flip a branch under +-1 ulp: replaced by state %d with velocities x 0.9^k, k = %d .." % (
            name, np.nonzero(flip)[0].tolist(), good, attempt + 1), flush=True)
        for j, b in enumerate(np.nonzero(flip)[0]):   # (each replacement a state of its own: 0.9, 0.81, ...)
            q[b], qd[b], a_in[b], lim[b] = q[good], qd[good] * np.float32(0.9 ** (attempt + 1 + j)), a_in[good], False
        moved = [ulp_moved(q, np.random.RandomState(100 + k)) for k in range(K_NOISE)]
    else:
        raise AssertionError("%s: branch flips remain" % name)

    out = dict(q_in=q, qd_in=qd, limit_state=lim, gq_out=c_q.numpy().reshape(B, nq), gqd_out=c_qd.numpy().reshape(B, nd),
               dt=np.float64(S * h), substeps=np.int64(S), mm_freq=np.int64(MM), **base)
    out["muscle_act_in" if M > 0 else "act_in"] = a_in
    for k, v in br0.items():
        out["br_" + k] = v
    # coverage
    has_joint = any(int(x) in HINGE + (2,) for x in t.joint_type)
    has_hinge = any(int(x) in HINGE for x in t.joint_type)
    has_limit = len(limited_coords(t)) >= 2
    # (d tau / d target = target_ke: a model whose hinges all have target_ke = 0 has no gradient there)
    has_target = any(int(x) in HINGE and t.joint_target_ke[i] != 0 for i, x in enumerate(t.joint_type))
    want = dict(target_ke=has_joint, target_kd=has_joint, target=has_target, limit_kd=has_hinge, limit_ke=has_limit,
                shape_materials=Cn > 0)
    for k, w in want.items():
        assert (not w) or np.abs(base["g_" + k]).max() > 0, (name, k)
    assert np.abs(base["gmuscle_act" if M > 0 else "gact"]).max() > 0, name
    if Cn:
        assert all(np.abs(base["g_shape_materials"][..., j]).max() > 0 for j in range(4)), name
    if has_limit:
        assert br0["low"].any() and br0["up"].any(), name
    tang = lambda g: project_tangent(t, q, g)  # noqa: E731
    for k in base:
        if k == "gq_in":
            out["noise_" + k] = tensor_noise([tang(r[0][k]) for r in reruns], tang(base[k]))
        elif np.abs(base[k]).max() > 0:
            out["noise_" + k] = tensor_noise([r[0][k] for r in reruns], base[k])
    if Cn:   # (ke, kd, kf, mu) are four parameters of different units: each column on its own scale as well
        out["noise_g_shape_materials_cols"] = np.array([tensor_noise([r[0]["g_shape_materials"][..., j] for r in reruns],
                                                                     base["g_shape_materials"][..., j]) for j in range(4)])
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in out.values())
    print("%-9s B=%d (%d limit states) h=%.5f  " % (name, B, int(lim.sum()), h) + "  ".join(
        "%s %.1e" % (k[6:], np.max(out[k])) for k in sorted(out) if k.startswith("noise_")), flush=True)
    keep = ("limit_state", "substeps", "mm_freq", "dt")
    return {k: (np.asarray(v, np.float32) if k not in keep and not k.startswith("br_") else np.asarray(v)) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        np.savez_compressed(os.path.join(OUT, name + "_par.npz"), **record(df, envs, G, name))


if __name__ == "__main__":
    main(sys.argv[1:])
