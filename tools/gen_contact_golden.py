"""Records tests/golden/<env>_con.npz: the ground-contact read-out of the reference simulator and its gradients, the fixtures of
dsim_ground_contacts / dsim_ground_contacts_backward.  Needs the reference checkout (it imports oracle/ref_harness.py and
oracle/gen_golden.py, which load it at run time); what it writes is recorded numbers only.

    python tools/gen_contact_golden.py [env ...]

Recipe, per model with contacts (C per environment):
  * inputs q_in, qd_in (act_in / muscle_act_in for the composite), stored in the fixture: the B0 states of
    tests/golden/<env>_step.npz and, for Humanoid, Hopper and Cheetah -- whose step states hold a handful of active contacts in
    one friction branch and none with vn < 0 -- four of those states with the root LOWERED until the deepest contact point is a
    given depth inside the ground, and a vertical root velocity added (LOWERED below; `lowered` [B] marks them).  The generator
    asserts that every model's states hold active contacts with a1 < a2, a1 >= a2, vn < 0 and vn >= 0 (`coverage`);
  * so = integrator.forward(model, state, sim_dt / sim_substeps, 1, 1) with zero actuation: with ONE substep so.body_X_sc /
    body_v_s belong to the input state and carry a grad_fn (X_sc, v_s in the fixture; for the step states they equal sub_X_sc /
    sub_v_s of the step fixture bit for bit);
  * link_wrench: the reference's own eval_rigid_contacts_art on (so.body_X_sc, so.body_v_s) and a zeroed body_f_s, through its
    stand-alone autograd launcher (adjoint.launch_torch), all contacts in one launch;
  * force [B][C][3]: the same kernel with the contact arrays sliced to one slot k of every environment (k + C arange(B)): each
    contact lands on its own row of the zeroed body_f_s, whose force half is the contact's f_total;
  * point, vel: the reference has no tensor of them: the float64 statement (tests/con_lib.contacts) on the recorded X_sc / v_s;
  * seeded normal cotangents c_point, c_vel, c_force, c_lw; gq_<set>, gqd_<set> for set = point, vel, force, lw, all: force and
    lw back-propagated through the reference to joint_q / joint_qd (alone, and together for `all`), point and vel by the
    statement's adjoint chained with kin_lib.fk_adjoint (held to the reference by the kinematics fixtures);
  * noise_<tensor> [B] and noise_gq_<set> / noise_gqd_<set> [B]: K = 8 copies of (q, qd) moved by +-1 ulp (random signs): per
    state the max deviation of its row over the K runs, divided by the max-norm of the whole base tensor (gq after
    project_tangent), each set on its own scale -- the reference's own fp32 noise;
  * fwd_bound_<tensor> (comp_fwd_bound_<tensor>): the bound a forward comparison against this fixture uses, 1e-4 in the tensor's
    max-norm unless the reference's own recorded noise alone exceeds a tenth of that: then 10 x that noise (SNUHumanoid's force
    and link_wrench, whose largest entries are sums of contact terms that cancel);
  * edge [B][C]: |point.y| < 1e-4, where fp32 rounding may flip the contact's active set (tests/con_lib.EDGE): asserted to be at
    most 1 % of the contacts and in at most one state; comp_edge likewise for the composite;
  * composite: so1 = forward(model, state, sim_dt, substeps, mm_freq) with the recorded actuation, so2 = forward(model, so1,
    sim_dt / substeps, 1, 1) for the frames of so1's state, the contact tensors of it as above and the loss over all four (point
    and vel enter through their linearisation (gX_sc, gv_s) = con_lib.contacts_adjoint on so2.body_X_sc / body_v_s):
    comp_q, comp_qd, comp_point, comp_vel, comp_force, comp_lw, comp_gq_in, comp_gqd_in, comp_gact (comp_gmuscle_act) and
    comp_noise_<name> [B] as above.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("ant", "humanoid", "snu", "hopper", "cheetah")
SEED, K_NOISE = 29, 8
# (index of the step state, depth of the deepest contact point, vertical root velocity added)
LOWERED = {"humanoid": ((0, 0.004, -0.6), (2, 0.03, 0.4), (3, 0.012, -0.15), (5, 0.045, -1.5)),
           "hopper": ((0, 0.004, -0.6), (3, 0.03, 0.4), (4, 0.012, -0.15), (7, 0.05, -1.5)),
           "cheetah": ((0, 0.004, -0.6), (2, 0.03, 0.4), (5, 0.012, -0.15), (6, 0.05, -1.5))}


def ulp_moved(a, rs):
    sgn = rs.choice([-1.0, 1.0], size=a.shape).astype(np.float32)
    return np.nextafter(a, a + sgn * np.float32(1.0)).astype(np.float32)


def row_noise(runs, base):
    """[B]: max deviation of each state's row over the runs / max-norm of the whole base tensor"""
    B = base.shape[0]
    b = np.asarray(base, np.float64).reshape(B, -1)
    dev = np.max([np.abs(np.asarray(r, np.float64).reshape(B, -1) - b).max(axis=1) for r in runs], axis=0)
    return dev / (np.abs(b).max() + 1e-30)


def vertical_root(t, q, qd):
    """(coordinate, dof) of the root whose unit change moves every contact point / point velocity by +1 along y"""
    import con_lib
    p0, v0 = con_lib.forward(t, q, qd)[:2]
    jq = jd = None
    for j in range(min(7, t.n_q)):
        q1 = np.array(q, np.float64)
        q1[j] += 1e-3
        if np.allclose((con_lib.forward(t, q1, qd)[0][:, 1] - p0[:, 1]) / 1e-3, 1.0, atol=1e-6):
            jq = j
    for d in range(min(6, t.n_qd)):
        qd1 = np.array(qd, np.float64)
        qd1[d] += 1.0
        if np.allclose(con_lib.forward(t, q, qd1)[1][:, 1] - v0[:, 1], 1.0, atol=1e-9):
            jd = d
    assert jq is not None and jd is not None
    return jq, jd


def input_states(t, name, g):
    import con_lib
    q, qd = g["q_in"].astype(np.float32), g["qd_in"].astype(np.float32)
    a = (g["muscle_act_in"] if t.n_muscles > 0 else g["act_in"]).astype(np.float32)
    low = np.zeros(len(q), bool)
    for src, depth, dv in LOWERED.get(name, ()):
        jq, jd = vertical_root(t, q[src], qd[src])
        q1, qd1 = q[src].copy(), qd[src].copy()
        q1[jq] -= np.float32(con_lib.forward(t, q1, qd1)[0][:, 1].min() + depth)
        qd1[jd] += np.float32(dv)
        q, qd, a, low = np.vstack([q, q1[None]]), np.vstack([qd, qd1[None]]), np.vstack([a, a[src][None]]), np.append(low, True)
    cov = con_lib.coverage(t, q, qd)
    assert min(cov.values()) > 0, (name, cov)
    return q, qd, a, low, cov


def record(df, envs, G, name):
    import torch
    import con_lib
    from oracle_lib import project_tangent, template_from_golden
    g = np.load(os.path.join(OUT, name + "_step.npz"))
    t = template_from_golden(name)
    q, qd, a_in, lowered, cov = input_states(t, name, g)
    B, B0 = q.shape[0], g["q_in"].shape[0]
    env = G.make_env(envs, name, B, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    L, nd, M, Cn = model.link_count // B, model.joint_dof_count // B, model.muscle_count // B, model.contact_count // B
    assert Cn == t.n_contacts and L == t.n_links
    atag = "gmuscle_act" if M > 0 else "gact"
    S, mm = int(g["substeps"]), int(g["mm_freq"])
    kernel, launch = df.sim.eval_rigid_contacts_art, df.adjoint.launch_torch
    carr = (model.contact_body0, model.contact_point0, model.contact_dist, model.contact_material)
    gen = torch.Generator().manual_seed(SEED)
    cs = {k: torch.randn(n, generator=gen) for k, n in (("point", (B, Cn, 3)), ("vel", (B, Cn, 3)), ("force", (B, Cn, 3)), ("lw", (B, L, 6)))}
    cn = {k: v.numpy().astype(np.float64) for k, v in cs.items()}
    out = dict(q_in=q, qd_in=qd, lowered=lowered, coverage=np.array([cov[k] for k in sorted(cov)], np.int64),
               **{"c_" + k: v.numpy() for k, v in cs.items()})
    out["muscle_act_in" if M > 0 else "act_in"] = a_in

    def start(qv, qdv, act=None):
        st = model.state()
        st.joint_q = torch.tensor(qv.reshape(-1), dtype=torch.float32, requires_grad=True)
        st.joint_qd = torch.tensor(qdv.reshape(-1), dtype=torch.float32, requires_grad=True)
        act = torch.tensor(act).clone().requires_grad_(True) if act is not None else None
        if M > 0:
            model.muscle_activation = act.view(-1) if act is not None else torch.zeros(B * M)
            st.joint_act = torch.zeros(B * nd)
        else:
            st.joint_act = act.view(-1) if act is not None else torch.zeros(B * nd)
        return st, act

    def contact_tensors(X, V, want_force=True, want_lw=True):
        """the reference's kernel on (X, V): (force [B][C][3] | None, link_wrench [B][L][6] | None), with grad_fn"""
        zero = torch.zeros(B * L, 6)
        lw = force = None
        if want_lw:
            lw = launch(kernel, B * Cn, [X, V, *carr, model.shape_materials], [zero], "cpu")[0].view(B, L, 6)
        if want_force:
            cols = []
            for k in range(Cn):
                idx = k + Cn * torch.arange(B)
                fk = launch(kernel, B, [X, V] + [c[idx].contiguous() for c in carr] + [model.shape_materials], [zero], "cpu")[0]
                cols.append(fk[carr[0][idx].long(), 3:6])
            force = torch.stack(cols, dim=1)
        return force, lw

    def statement(X, V):
        X, V = X.detach().numpy().astype(np.float64).reshape(B, L, 7), V.detach().numpy().astype(np.float64).reshape(B, L, 6)
        r = [con_lib.contacts(t, X[b], V[b]) for b in range(B)]
        return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])

    def grads(st, act=None):
        z = lambda x: x.grad.numpy().reshape(B, -1).copy() if x.grad is not None else np.zeros((B, x.numel() // B), np.float32)  # noqa: E731
        return (z(st.joint_q), z(st.joint_qd)) + ((z(act),) if act is not None else ())

    def direct(qv, qdv, keys):
        """reference run for the sets of force / lw in `keys` -> (gq, gqd, fwd dict)"""
        st, _ = start(qv, qdv)
        so = integ.forward(model, st, env.sim_dt / env.sim_substeps, 1, 1)
        force, lw = contact_tensors(so.body_X_sc, so.body_v_s, "force" in keys, "lw" in keys)
        point, vel = statement(so.body_X_sc, so.body_v_s)
        fwd = dict(point=point, vel=vel, X_sc=so.body_X_sc.detach().numpy().reshape(B, L, 7).copy(),
                   v_s=so.body_v_s.detach().numpy().reshape(B, L, 6).copy())
        loss = 0.0
        if force is not None:
            fwd["force"] = force.detach().numpy().copy()
            loss = loss + (force * cs["force"]).sum()
        if lw is not None:
            fwd["lw"] = lw.detach().numpy().copy()
            loss = loss + (lw * cs["lw"]).sum()
        loss.backward()
        return grads(st) + (fwd,)

    def statement_grads(qv, qdv, keys):
        """gradients of the point / vel sets in `keys` by the float64 statement"""
        z3 = np.zeros((B, Cn, 3))
        return con_lib.adjoint_batch(t, qv.astype(np.float64), qdv.astype(np.float64), cn["point"] if "point" in keys else z3,
                                     cn["vel"] if "vel" in keys else z3, None, None)

    def all_sets(qv, qdv):
        r = {}
        gf = direct(qv, qdv, ("force",))
        gl = direct(qv, qdv, ("lw",))
        gb = direct(qv, qdv, ("force", "lw"))
        gp, gv = statement_grads(qv, qdv, ("point",)), statement_grads(qv, qdv, ("vel",))
        r["force"], r["lw"], r["point"], r["vel"] = gf[:2], gl[:2], gp, gv
        r["all"] = (gb[0] + gp[0] + gv[0], gb[1] + gp[1] + gv[1])
        return r, gb[2]

    base, fwd = all_sets(q, qd)
    assert np.array_equal(fwd["X_sc"][:B0], g["sub_X_sc"].reshape(B0, L, 7)) and np.array_equal(fwd["v_s"][:B0], g["sub_v_s"].reshape(B0, L, 6))
    out.update(X_sc=fwd["X_sc"], v_s=fwd["v_s"], point=fwd["point"], vel=fwd["vel"], force=fwd["force"], link_wrench=fwd["lw"])
    for tag, (gq, gqd) in base.items():
        out["gq_" + tag], out["gqd_" + tag] = gq, gqd
    edge = np.abs(fwd["point"][:, :, 1]) < con_lib.EDGE
    assert edge.sum() <= 0.01 * B * Cn and (edge.any(axis=1)).sum() <= 1, (name, edge.sum(), edge.any(axis=1))
    out["edge"] = edge
    # the reference's tensors against the statement, and its link_wrench against the gather of its per-contact forces
    st64 = con_lib.forward_batch(t, q.astype(np.float64), qd.astype(np.float64))
    keep = ~edge
    e_force = np.abs(fwd["force"] - st64[2])[keep].max() / np.abs(st64[2]).max()
    e_gather = np.abs(con_lib.gather_link_wrench(t, fwd["point"], fwd["force"]) - fwd["lw"]).max() / np.abs(fwd["lw"]).max()
    assert not fwd["force"][(fwd["point"][:, :, 1] >= 0) & keep].any()   # exactly zero where the point does not penetrate

    runs, fruns = {tag: [] for tag in base}, {k: [] for k in ("point", "vel", "force", "lw")}
    for k in range(K_NOISE):
        rs = np.random.RandomState(100 + k)
        q1, qd1 = ulp_moved(q, rs), ulp_moved(qd, rs)
        r, f1 = all_sets(q1, qd1)
        for tag in base:
            runs[tag].append((project_tangent(t, q, r[tag][0]), r[tag][1]))
        for kk in fruns:
            fruns[kk].append(f1[kk])
    for kk, nm in (("point", "point"), ("vel", "vel"), ("force", "force"), ("lw", "link_wrench")):
        out["noise_" + nm] = row_noise(fruns[kk], fwd[kk])
        out["fwd_bound_" + nm] = np.float64(max(1e-4, 10.0 * out["noise_" + nm].max()))
    for tag in base:
        out["noise_gq_" + tag] = row_noise([r[0] for r in runs[tag]], project_tangent(t, q, base[tag][0]))
        out["noise_gqd_" + tag] = row_noise([r[1] for r in runs[tag]], base[tag][1])

    def composite(qv, qdv):
        st, act = start(qv, qdv, a_in)
        so1 = integ.forward(model, st, env.sim_dt, S, mm)
        so1.joint_act = torch.zeros(B * nd)   # (the read-out does not depend on the actuation; the muscle activations stay on the model)
        so2 = integ.forward(model, so1, env.sim_dt / S, 1, 1)
        X, V = so2.body_X_sc, so2.body_v_s
        force, lw = contact_tensors(X, V)
        point, vel = statement(X, V)
        Xn, Vn = X.detach().numpy().astype(np.float64).reshape(B, L, 7), V.detach().numpy().astype(np.float64).reshape(B, L, 6)
        lin = [con_lib.contacts_adjoint(t, Xn[b], Vn[b], cn["point"][b], cn["vel"][b], np.zeros((Cn, 3)), np.zeros((L, 6))) for b in range(B)]
        gX = torch.tensor(np.stack([x[0] for x in lin]), dtype=torch.float32).view(B * L, 7)
        gV = torch.tensor(np.stack([x[1] for x in lin]), dtype=torch.float32).view(B * L, 6)
        # (read BEFORE the backward pass: the reference's reverse kernels re-execute the atomic_adds into their output)
        r = dict(q=so1.joint_q.detach().numpy().reshape(B, -1).copy(), qd=so1.joint_qd.detach().numpy().reshape(B, -1).copy(),
                 point=point, vel=vel, force=force.detach().numpy().copy(), lw=lw.detach().numpy().copy())
        ((force * cs["force"]).sum() + (lw * cs["lw"]).sum() + (X * gX).sum() + (V * gV).sum()).backward()
        r["gq_in"], r["gqd_in"], r["gact"] = grads(st, act)
        return r

    cb = composite(q, qd)
    assert np.array_equal(cb["q"][:B0], g["q_out"])
    cname = dict(q="comp_q", qd="comp_qd", point="comp_point", vel="comp_vel", force="comp_force", lw="comp_lw",
                 gq_in="comp_gq_in", gqd_in="comp_gqd_in", gact="comp_" + atag)
    for k, nm in cname.items():
        out[nm] = cb[k]
    out["comp_edge"] = np.abs(cb["point"][:, :, 1]) < con_lib.EDGE
    assert out["comp_edge"].sum() <= 0.01 * B * Cn and out["comp_edge"].any(axis=1).sum() <= 1, (name, out["comp_edge"].sum())
    cruns = []
    for k in range(K_NOISE):
        rs = np.random.RandomState(100 + k)
        r = composite(ulp_moved(q, rs), ulp_moved(qd, rs))
        r["gq_in"] = project_tangent(t, q, r["gq_in"])
        cruns.append(r)
    for k, nm in cname.items():
        b = project_tangent(t, q, cb[k]) if k == "gq_in" else cb[k]
        out["comp_noise_" + nm[5:]] = row_noise([r[k] for r in cruns], b)
    for k in ("point", "vel", "force", "lw"):
        out["comp_fwd_bound_" + k] = np.float64(max(1e-4, 10.0 * out["comp_noise_" + k].max()))
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in out.values())
    print("%-9s B=%d (%d lowered) C=%d coverage %s edge %d  force vs statement %.1e  lw vs gather %.1e" % (
        name, B, int(lowered.sum()), Cn, cov, int(edge.sum()), e_force, e_gather), flush=True)
    print("          fwd noise " + " ".join("%s %.1e (bound %.1e)" % (n, out["noise_" + n].max(), out["fwd_bound_" + n])
                                             for n in ("point", "vel", "force", "link_wrench")), flush=True)
    for tag in base:
        print("          set %-5s noise gq %.1e gqd %.1e   max|gq| %.3e" % (tag, out["noise_gq_" + tag].max(), out["noise_gqd_" + tag].max(),
                                                                              np.abs(out["gq_" + tag]).max()), flush=True)
    print("          composite noise " + " ".join("%s %.1e" % (nm[5:], out["comp_noise_" + nm[5:]].max()) for nm in cname.values()) +
          "  comp edge %d" % int(out["comp_edge"].sum()), flush=True)
    keep32 = ("lowered", "coverage", "edge", "comp_edge")
    return {k: (np.asarray(v, np.float32) if k not in keep32 else np.asarray(v)) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        np.savez_compressed(os.path.join(OUT, name + "_con.npz"), **record(df, envs, G, name))


if __name__ == "__main__":
    main(sys.argv[1:])
