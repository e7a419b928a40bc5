"""Records tests/golden/<env>_kin.npz: the reference simulator's State.body_X_sc / body_X_sm / body_v_s gradients, the
fixtures of the differentiable body kinematics (dsim_body_kinematics_backward).  Needs the reference checkout (it imports
oracle/ref_harness.py and oracle/gen_golden.py, which load it at run time); what it writes is recorded numbers only.

    python tools/gen_kinematics_golden.py [env ...]

Recipe, per model (inputs: q_in, qd_in of tests/golden/<env>_step.npz, B states):
  * so = integrator.forward(model, state, sim_dt / sim_substeps, 1, 1) with zero joint_act: with ONE substep the returned State's
    body_X_sc / body_X_sm / body_v_s belong to the input state and carry a grad_fn;
  * seeded normal cotangents c_Xsc, c_Xsm, c_vs; four backward passes -- each tensor alone, then all three -- -> gq_*, gqd_*;
  * sens_gq, sens_gqd: the combined gradient from K = 4 copies of the inputs moved by +-1 ulp (random signs): max-norm relative
    deviation from the base run (gq after project_tangent) -- the reference's own fp32 noise;
  * composite: so1 = forward(model, state, sim_dt, substeps, mm_freq) with the step fixture's act_in / muscle_act_in, then
    so2 = forward(model, so1, sim_dt / substeps, 1, 1) and the same loss on so2's three tensors (the kinematics of so1.joint_q,
    joint_qd): comp_X_sc, comp_X_sm, comp_v_s, comp_gact (comp_gmuscle_act), comp_gq_in, comp_gqd_in.
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
KEYS = ("body_X_sc", "body_X_sm", "body_v_s")
SEED, K_SENS = 23, 4


def record(df, envs, G, name):
    import torch
    from oracle_lib import project_tangent, relerr, template_from_golden
    g = np.load(os.path.join(OUT, name + "_step.npz"))
    t = template_from_golden(name)
    q, qd = g["q_in"], g["qd_in"]
    B = q.shape[0]
    env = G.make_env(envs, name, B, no_grad=False, stochastic=False)
    df.config.no_grad = False
    model, integ = env.model, env.integrator
    L, nd, M = model.link_count // B, model.joint_dof_count // B, model.muscle_count // B
    gen = torch.Generator().manual_seed(SEED)
    cs = {k: torch.randn(n, generator=gen) for k, n in zip(KEYS, ((B * L, 7), (B * L, 7), (B * L, 6)))}
    out = dict(c_Xsc=cs[KEYS[0]].numpy().reshape(B, L, 7), c_Xsm=cs[KEYS[1]].numpy().reshape(B, L, 7),
               c_vs=cs[KEYS[2]].numpy().reshape(B, L, 6))

    def kin_grad(qv, qdv, keys):
        st = model.state()
        st.joint_q = torch.tensor(qv.reshape(-1), dtype=torch.float32, requires_grad=True)
        st.joint_qd = torch.tensor(qdv.reshape(-1), dtype=torch.float32, requires_grad=True)
        st.joint_act = torch.zeros(model.joint_dof_count)
        if M > 0:
            model.muscle_activation = torch.zeros(model.muscle_count)
        so = integ.forward(model, st, env.sim_dt / env.sim_substeps, 1, 1)
        sum((getattr(so, k) * cs[k]).sum() for k in keys).backward()
        gqd = st.joint_qd.grad if st.joint_qd.grad is not None else torch.zeros_like(st.joint_qd)
        return (st.joint_q.grad.numpy().reshape(B, -1).copy(), gqd.numpy().reshape(B, -1).copy(),
                [getattr(so, k).detach().numpy().copy() for k in KEYS])

    for tag, keys in (("Xsc", KEYS[:1]), ("Xsm", KEYS[1:2]), ("vs", KEYS[2:]), ("all", KEYS)):
        out["gq_" + tag], out["gqd_" + tag], xs = kin_grad(q, qd, keys)
    # the one-substep State belongs to the input state: it reproduces the step fixture's first-substep tensors
    assert np.array_equal(xs[0].reshape(B, L, 7), g["sub_X_sc"].reshape(B, L, 7)) and np.array_equal(xs[2].reshape(B, L, 6), g["sub_v_s"].reshape(B, L, 6))
    pq = project_tangent(t, q, out["gq_all"])
    worst = [0.0, 0.0]
    for k in range(K_SENS):
        rs = np.random.RandomState(100 + k)
        sgn = rs.choice([-1.0, 1.0], size=q.shape).astype(np.float32)
        q1 = np.nextafter(q, q + sgn * np.float32(1.0)).astype(np.float32)
        sgn = rs.choice([-1.0, 1.0], size=qd.shape).astype(np.float32)
        qd1 = np.nextafter(qd, qd + sgn * np.float32(1.0)).astype(np.float32)
        gq1, gqd1, _ = kin_grad(q1, qd1, KEYS)
        worst = [max(worst[0], relerr(project_tangent(t, q, gq1), pq)), max(worst[1], relerr(gqd1, out["gqd_all"]))]
    out["sens_gq"], out["sens_gqd"] = np.float64(worst[0]), np.float64(worst[1])

    # composite: a whole env-step, then the kinematics of its end state
    st = model.state()
    st.joint_q = torch.tensor(q.reshape(-1), dtype=torch.float32, requires_grad=True)
    st.joint_qd = torch.tensor(qd.reshape(-1), dtype=torch.float32, requires_grad=True)
    if M > 0:
        act = torch.tensor(g["muscle_act_in"]).clone().requires_grad_(True)
        model.muscle_activation = act.view(-1)
        st.joint_act = torch.zeros(B * nd)
    else:
        act = torch.tensor(g["act_in"]).clone().requires_grad_(True)
        st.joint_act = act.view(-1)
    S, mm = int(g["substeps"]), int(g["mm_freq"])
    so1 = integ.forward(model, st, env.sim_dt, S, mm)
    assert np.array_equal(so1.joint_q.detach().numpy().reshape(B, -1), g["q_out"])
    if M == 0:
        so1.joint_act = torch.zeros(B * nd)
    so2 = integ.forward(model, so1, env.sim_dt / S, 1, 1)
    sum((getattr(so2, k) * cs[k]).sum() for k in KEYS).backward()
    out["comp_X_sc"] = so2.body_X_sc.detach().numpy().reshape(B, L, 7)
    out["comp_X_sm"] = so2.body_X_sm.detach().numpy().reshape(B, L, 7)
    out["comp_v_s"] = so2.body_v_s.detach().numpy().reshape(B, L, 6)
    out["comp_gmuscle_act" if M > 0 else "comp_gact"] = act.grad.numpy().reshape(B, -1)
    out["comp_gq_in"] = st.joint_q.grad.numpy().reshape(B, -1)
    out["comp_gqd_in"] = st.joint_qd.grad.numpy().reshape(B, -1)
    assert all(np.isfinite(v).all() for v in out.values())
    print("%-9s B=%d  sens gq %.2e gqd %.2e  max|gq_all| %.3e  composite max|gact| %.3e" % (
        name, B, worst[0], worst[1], np.abs(out["gq_all"]).max(), act.grad.abs().max().item()), flush=True)
    return {k: (np.asarray(v, np.float32) if np.ndim(v) else v) for k, v in out.items()}


def main(argv):
    import gen_golden as G
    import ref_harness
    df, envs = ref_harness.load_reference()
    for name in (argv or NAMES):
        np.savez_compressed(os.path.join(OUT, name + "_kin.npz"), **record(df, envs, G, name))


if __name__ == "__main__":
    main(sys.argv[1:])
