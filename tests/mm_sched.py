"""Test infrastructure: the inputs and oracle results of the mass-matrix refresh-schedule tests, shared by the host tier
(tests/test_emu_phases.py, tests/test_emu_fused_env.py, tests/test_step_jacobian_cpu.py) and the GPU tier
(tests/test_gpu_mm_schedules.py).  Computed once per process, handed out read-only.

Operator level: the first 6 states of tests/golden/<env>_step.npz, cotangents from default_rng(11), S = 7 substeps of the
reference's substep length (dt = S / 960), mm in MMS.  Seven substeps is the smallest count that gives, over MMS, a two-ahead
prefetch across a group switch, a middle group, a trailing group of one substep and a trailing group of more than one:
  mm  1: 1,1,1,1,1,1,1    mm 2: 2,2,2,1    mm 3: 3,3,1    mm 4: 4,3    mm 6: 6,1    mm 7: 7    mm 9: 7 (mm > S)

Environment level: H = 3 steps from the first environments of tests/golden/<env>_rollout.npz at the environments' own substep
counts, MM_caching_frequency from ENV_MM (uneven last groups, among them a last group of one substep); loss = -sum(rew).

Bounds (none of them probed): state 1e-4, gradients 1e-3 max-norm relative (joint_q cotangents after
project_tangent), rollout cosine > 0.9999.
"""
import numpy as np

from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden

ENVS = ["cartpole", "ant", "humanoid", "snu", "hopper", "cheetah"]
S = 7
DT = S / 960.0
MMS = [1, 2, 3, 4, 6, 7, 9]
N_STATES = 6
STATE_TOL, GRAD_TOL, COS_MIN = 1e-4, 1e-3, 0.9999

H = 3
ENV_SUBSTEPS = {"cartpole": 4, "ant": 16, "humanoid": 48, "snu": 48, "hopper": 16, "cheetah": 16}
# group sizes: cartpole 3+1 | hopper 6,6,4 | cheetah 5,5,5,1 | ant 5,5,5,1 and 6,6,4 | humanoid 4 x 10 + 8 | snu 9 x 5 + 3
ENV_MM = [("cartpole", 3), ("hopper", 6), ("cheetah", 5), ("ant", 5), ("ant", 6), ("humanoid", 10), ("snu", 5)]

_cases, _oracle, _rollouts, _rollout_oracle = {}, {}, {}, {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def case(env):
    """dict: t (template), q, qd, act, mact (None without muscles), gq, gqd -- [6, .] float32 each"""
    if env not in _cases:
        t, g = template_from_golden(env), golden(env + "_step")
        sl = slice(0, N_STATES)
        rng = np.random.default_rng(11)
        c = dict(t=t, q=g["q_in"][sl].copy(), qd=g["qd_in"][sl].copy(), act=g["act_in"][sl].copy(),
                 mact=g["muscle_act_in"][sl].copy() if "muscle_act_in" in g else None,
                 gq=rng.normal(size=(N_STATES, t.n_q)).astype(np.float32), gqd=rng.normal(size=(N_STATES, t.n_qd)).astype(np.float32))
        assert c["q"].shape[0] == N_STATES
        _cases[env] = _frozen(c)
    return _cases[env]


def oracle(env, mm):
    """oracle_backward of case(env) at (S, mm): q_out, qd_out, gq, gqd, gact, gmact"""
    if (env, mm) not in _oracle:
        c = case(env)
        _oracle[(env, mm)] = _frozen(oracle_backward(c["t"], c["q"], c["qd"], c["act"], c["mact"], DT, S, mm, c["gq"], c["gqd"]))
    return _oracle[(env, mm)]


def step_errors(env, mm, got):
    """errors of got = dict(q, qd, gq, gqd, gact[, gmact]) ([6, .] arrays) against oracle(env, mm): name -> max-norm relative error"""
    c, o = case(env), oracle(env, mm)
    t = c["t"]
    err = dict(q=relerr(got["q"], o["q_out"]), qd=relerr(got["qd"], o["qd_out"]),
               gq=relerr(project_tangent(t, c["q"], got["gq"]), project_tangent(t, c["q"], o["gq"])),
               gqd=relerr(got["gqd"], o["gqd"]), gact=relerr(got["gact"], o["gact"]))
    if c["mact"] is not None:
        err["gmact"] = relerr(got["gmact"], o["gmact"])
    return err


def assert_step(env, mm, got, state_tol=STATE_TOL, grad_tol=GRAD_TOL, label=""):
    """prints every figure, then asserts it; -> the figures"""
    err = step_errors(env, mm, got)
    print("mm-schedule %s %s S=%d mm=%d: %s" % (label, env, S, mm, "  ".join("%s %.2e" % kv for kv in err.items())))
    for k, e in err.items():
        assert np.isfinite(e) and e < (state_tol if k in ("q", "qd") else grad_tol), (env, mm, k, e)
    return err


def rollout_case(env, n=4):
    """dict: t, q0, qd0 [n, .], actions [H, n, n_act]; n = min(n, what the recording has)"""
    if (env, n) not in _rollouts:
        g = golden(env + "_rollout")
        k = min(n, g["q0"].shape[0])
        assert g["actions"].shape[0] >= H
        _rollouts[(env, n)] = _frozen(dict(t=template_from_golden(env), q0=g["q0"][:k].copy(), qd0=g["qd0"][:k].copy(),
                                           actions=g["actions"][:H, :k].copy()))
    return _rollouts[(env, n)]


def rollout_oracle(env, mm):
    """(obs [H, n, n_obs], rew [H, n], d(-sum rew)/d actions [H, n, n_act]) of rollout_case(env) through the torch environment
    surface with the scalar oracle as integrator, at MM_caching_frequency = mm"""
    if (env, mm) not in _rollout_oracle:
        from oracle_env import rollout_grad
        c = rollout_case(env)
        out = rollout_grad(env, c["t"], c["q0"], c["qd0"], c["actions"].copy(), mm_freq=mm)
        for a in out:
            a.setflags(write=False)
        _rollout_oracle[(env, mm)] = out
    return _rollout_oracle[(env, mm)]


def assert_rollout(env, mm, obs, rew, ga, label=""):
    """obs / rew per step at the state tolerance, the action gradient at the gradient tolerance and the cosine; prints the
    figures first; -> them"""
    o_obs, o_rew, o_ga = rollout_oracle(env, mm)
    a, r = np.asarray(ga, np.float64), np.asarray(o_ga, np.float64)
    fig = dict(obs=max(relerr(obs[s], o_obs[s]) for s in range(H)),
               rew=float(np.abs(np.asarray(rew, np.float64) - o_rew).max() / max(1.0, np.abs(o_rew).max())),
               grad=relerr(a, r), one_minus_cos=1.0 - float((a * r).sum() / (np.linalg.norm(a) * np.linalg.norm(r))))
    print("mm-schedule rollout %s %s S=%d mm=%d H=%d: %s" % (label, env, ENV_SUBSTEPS[env], mm, H,
                                                            "  ".join("%s %.2e" % kv for kv in fig.items())))
    assert all(np.isfinite(v) for v in fig.values()), fig
    assert fig["obs"] < STATE_TOL and fig["rew"] < STATE_TOL, (env, mm, fig)
    assert fig["grad"] < GRAD_TOL and 1.0 - fig["one_minus_cos"] > COS_MIN, (env, mm, fig)
    return fig
