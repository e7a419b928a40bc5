"""CPU tier: the whole binding layer of diffrl_amd/engine.py against a recording stand-in for the library (tests/engine_stub.py).
Nothing is loaded, nothing runs on a GPU: the refusals below include calls that, without the check they test, would hand a
kernel a buffer that is too small -- they must never be tried against real kernels.

Two models from the goldens: CartPole (no muscles, no quaternion, NO contacts: its contact outputs have no elements) and SNUHumanoid
(muscles).  N = 2 environments, S = 3 substeps, mass-matrix frequency 2, K = 2 cotangent rows.

(a) READOUTS against include/dsim.h; (b) every launching method with valid arguments and every None it accepts: argument count,
roles in header order, shapes of what it allocates; (c) every tensor argument one element short, float64, strided, of the other
model's width: DsimError and NO call; (d) the calls of (b), autograd included, equal those recorded from the previous version of
engine.py, call for call (tests/golden/engine_binding_calls.json; `python tests/test_engine_binding_cpu.py ENGINE.py OUT.json`
records them from any version of the file); (e) autograd through the read-outs: one cotangent per output read, no launch for
none, gradients in the input shapes."""
import importlib.util
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]   # (for the run as a script, below)

import diffrl_amd.capi as capi                                     # noqa: E402
import diffrl_amd.engine as engine_module                          # noqa: E402
from engine_stub import FakeLib, LITERAL_SCRATCH, recording, stub_class   # noqa: E402
from oracle_lib import template_from_golden                        # noqa: E402

GOLDEN =os.path.join(ROOT, "tests", "golden", "engine_binding_calls.json")
MODELS = ("cartpole", "snu")
N, S, MM, K, DT = 2, 3, 2, 2, 1.0 / 60.0
N_ACT, N_OBS = 3, 7   # of the fused environment surface: unlike every width of the two models
WORDS = FakeLib().dsim_ckpt_floats_mm(None, S, MM)
I64, I32 = torch.int64, torch.int32


def _spec():
    return capi.make_env_spec(capi.ENV_CARTPOLE, capi.REW_CARTPOLE, N_ACT, N_OBS, None)


class Method:
    """One way of calling a launching method of Engine: `call(engine, a)` with a = {argument name: tensor | None}; `shapes`
    gives every tensor argument's valid shape (2-D and flat alike: the engine goes by the element count), a dtype after the
    shape where it is not float32; `optional`: the ones that may be None; `own_copy`: the ones the method makes contiguous itself
    (a strided one is accepted)."""

    def __init__(self, name, call, shapes, optional=(), own_copy=()):
        self.name, self.call, self.shapes, self.optional, self.own_copy = name, call, shapes, optional, own_copy

    def args(self, e, without=()):
        def make(k, v):
            dtype = v[-1] if isinstance(v[-1], torch.dtype) else torch.float32
            return e.T(k, *[s for s in v if isinstance(s, int)], dtype=dtype)
        return {k: None if k in without else make(k, v) for k, v in self.shapes.items()}


def methods(t, mod):
    """every launching method of mod.Engine on a model of template t"""
    nq, nd, M, L, Cn = t.n_q, t.n_qd, t.n_muscles, t.n_links, t.n_contacts
    K2 = nq + nd
    state = dict(q=(N, nq), qd=(N * nd,))
    acts = dict(act=(N, nd), **(dict(muscle_act=(N * M,)) if M else {}))
    ck = dict(ckpt=(N, WORDS), **acts)
    cot = dict(gq_out=(N, nq), gqd_out=(N * nd,))
    ep = dict(progress=(N, I64), reset_q=(1, N, nq), reset_qd=(1, N * nd), reset_count=(N, I32), noise_q=(nq,), noise_qd=(nd,))

    def episode(a, want_obs_before):
        return mod.EpisodeIO(a["progress"], a["reset_q"], a["reset_qd"], a["reset_count"], 100, True, True, want_obs_before,
                             noise_q=a["noise_q"], noise_qd=a["noise_qd"], noise_angle=0.25, seed=7)

    g = lambda a, k: a.get(k)   # noqa: E731
    out = [
        Method("body_transforms", lambda e, a: e.body_transforms(a["q"]), dict(q=(N, nq)), own_copy=("q",)),
        Method("body_kinematics_forward", lambda e, a: e.body_kinematics_forward(a["q"], a["qd"]), state, ("qd",)),
        Method("body_kinematics_backward", lambda e, a: e.body_kinematics_backward(a["q"], a["qd"], a["gX_sc"], a["gX_sm"], a["gv_s"]),
               dict(state, gX_sc=(N * L, 7), gX_sm=(N * L * 7,), gv_s=(N * L, 6)), ("qd", "gX_sc", "gX_sm", "gv_s")),
        Method("joint_dynamics_forward", lambda e, a: e.joint_dynamics_forward(a["q"], a["qd"], a["act"], g(a, "muscle_act")),
               dict(state, **acts), ("act", "muscle_act")),
        Method("joint_dynamics_backward",
               lambda e, a: e.joint_dynamics_backward(a["q"], a["qd"], a["act"], g(a, "muscle_act"), a["gtau"], a["gqdd"], a["gf_s"]),
               dict(state, **acts, gtau=(N, nd), gqdd=(N * nd,), gf_s=(N * L, 6)), ("act", "muscle_act", "gtau", "gqdd", "gf_s")),
        Method("ground_contacts_forward", lambda e, a: e.ground_contacts_forward(a["q"], a["qd"]), state),
        Method("ground_contacts_backward",
               lambda e, a: e.ground_contacts_backward(a["q"], a["qd"], a["gpoint"], a["gvel"], a["gforce"], a["glink_wrench"]),
               dict(state, gpoint=(N * Cn, 3), gvel=(N * Cn * 3,), gforce=(N, Cn, 3), glink_wrench=(N * L, 6)),
               ("gpoint", "gvel", "gforce", "glink_wrench")),
        Method("mass_matrix_forward", lambda e, a: e.mass_matrix_forward(a["q"]), dict(q=(N, nq))),
        Method("mass_matrix_backward", lambda e, a: e.mass_matrix_backward(a["q"], a["gH"], a["gHinv"], a["gS"]),
               dict(q=(N * nq,), gH=(N, nd, nd), gHinv=(N * nd * nd,), gS=(N * nd, 6)), ("gH", "gHinv", "gS")),
        Method("forward", lambda e, a: e.forward(a["q"], a["qd"], a["act"], g(a, "muscle_act"), DT, S, MM, True, keep_q_in=True),
               dict(state, **acts)),
        Method("forward_no_ckpt", lambda e, a: e.forward(a["q"], a["qd"], a["act"], g(a, "muscle_act"), DT, S, MM, False),
               dict(state, **acts)),
    ]
    for name, kw in (("backward", {}), ("backward_literal", dict(literal=True))):
        out.append(Method(name, lambda e, a, kw=kw: e.backward(a["ckpt"], a["act"], g(a, "muscle_act"), DT, S, MM, a["gq_out"],
                                                                a["gqd_out"], **kw), dict(ck, **cot), own_copy=("gq_out", "gqd_out")))
    for shared, lead in ((False, (N, K)), (True, (K,))):
        out.append(Method("backward_multi_shared" if shared else "backward_multi",
                          lambda e, a, shared=shared: e.backward_multi(a["ckpt"], a["act"], g(a, "muscle_act"), DT, S, MM, a["gq_out"],
                                                                       a["gqd_out"], shared=shared),
                          dict(ck, gq_out=lead + (nq,), gqd_out=lead + (nd,)), own_copy=("gq_out", "gqd_out")))
    out.append(Method("step_jacobian", lambda e, a: e.step_jacobian(a["ckpt"], a["act"], g(a, "muscle_act"), DT, S, MM), ck))
    for dof, con in ((True, True), (True, False), (False, True)):
        out.append(Method("backward_params_%d%d" % (dof, con),
                          lambda e, a, dof=dof, con=con: e.backward_params(a["ckpt"], a["act"], g(a, "muscle_act"), DT, S, MM, a["gq_out"],
                                                                           a["gqd_out"], want_dof=dof, want_contact=con),
                          dict(ck, **cot), own_copy=("gq_out", "gqd_out")))
    F = mod.StepParameters.FIELDS
    out.append(Method("set_params", lambda e, a: e.set_params([a[f] for f in F]),
                      dict(zip(F, [(L,)] * 4 + [(nq,), (Cn, 4)])), F))
    env_in = dict(state, actions=(N, N_ACT))
    out += [
        Method("env_forward", lambda e, a: e.env_forward(_spec(), a["q"], a["qd"], a["actions"], DT, S, MM, True), env_in),
        Method("env_forward_no_ckpt", lambda e, a: e.env_forward(_spec(), a["q"], a["qd"], a["actions"], DT, S, MM, False, episode=None),
               env_in),
        Method("env_forward_episode",
               lambda e, a: e.env_forward(_spec(), a["q"], a["qd"], a["actions"], DT, S, MM, True, episode(a, True)),
               dict(env_in, **ep), ("noise_q", "noise_qd")),
        Method("env_forward_episode_no_grad",
               lambda e, a: e.env_forward(_spec(), a["q"], a["qd"], a["actions"], DT, S, MM, False, episode(a, False)),
               dict(env_in, **ep), ("noise_q", "noise_qd")),
        Method("env_backward",
               lambda e, a: e.env_backward(_spec(), a["ckpt"], a["actions"], DT, S, MM, a["gq_out"], a["gqd_out"], a["gobs"], a["grew"],
                                           a["gobs_before_reset"]),
               dict(ckpt=(N, WORDS), actions=(N * N_ACT,), **cot, gobs=(N, N_OBS), grew=(N,), gobs_before_reset=(N * N_OBS,)),
               ("gq_out", "gqd_out", "gobs", "grew", "gobs_before_reset")),
        Method("env_observe", lambda e, a: e.env_observe(_spec(), a["q"], a["qd"], a["stored_actions"]),
               dict(state, stored_actions=(N, N_ACT))),
    ]
    return out


def _loss(outs, read):
    return sum(o.sum() for i, o in enumerate(outs) if i in read and o is not None)


def autograd_cases(t, mod):
    """(name, run(engine)) through the autograd functions and the public differentiable methods: forward, then backward of a loss"""
    nq, nd, M = t.n_q, t.n_qd, t.n_muscles

    def leaves(e, *names):
        shapes = dict(q=(N, nq), qd=(N, nd), act=(N * nd,), muscle_act=(N, M), actions=(N, N_ACT))
        return [e.T(k, *shapes[k]).requires_grad_() for k in names]

    def step(e, fn, extra=()):
        q, qd, act = leaves(e, "q", "qd", "act")
        mact = leaves(e, "muscle_act")[0] if M else None
        qo, qdo = fn.apply(e, DT, S, MM, q, qd, act, mact, *extra)
        (qo.sum() + qdo.sum()).backward()
        assert q.grad.shape == q.shape and qd.grad.shape == qd.shape and act.grad.shape == act.shape
        assert mact is None or mact.grad.shape == mact.shape
        return q, qd, act, mact

    def step_params(e):
        params = [p.requires_grad_() for p in e.step_parameters().tensors()]
        step(e, mod.SimStepParams, params)
        assert all(p.grad is not None and p.grad.shape == p.shape for p in params)

    def env_step(e):
        q, qd, a = leaves(e, "q", "qd", "actions")
        qo, qdo, obs, rew = mod.EnvStep.apply(e, _spec(), None, DT, S, MM, q, qd, a)
        (obs.sum() + rew.sum()).backward()
        assert q.grad.shape == q.shape and a.grad.shape == a.shape

    def readout(e, name, inputs, read):
        x = leaves(e, *inputs)
        _loss(getattr(e, name)(*x), read).backward()
        for v in x:
            assert v.grad is not None and v.grad.shape == v.shape, (name, inputs)

    out = [("SimStep", lambda e: step(e, mod.SimStep)), ("SimStepParams", step_params), ("EnvStep", env_step)]
    for name, inputs, n_out in (("body_kinematics", ("q", "qd"), 3), ("body_kinematics", ("q",), 2),
                                ("joint_dynamics", ("q", "qd", "act") + (("muscle_act",) if M else ()), 3),
                                ("joint_dynamics", ("q", "qd"), 3), ("ground_contacts", ("q", "qd"), 4), ("mass_matrix", ("q",), 3)):
        out.append(("%s(%s) all outputs" % (name, ", ".join(inputs)),
                    lambda e, name=name, inputs=inputs, n_out=n_out: readout(e, name, inputs, range(n_out))))
    return out


def valid_calls(model, mod):
    """{case: the calls the stub recorded} for every method with all its arguments, with each optional one None, with each
    self-copied one strided, and for the autograd cases"""
    t = template_from_golden(model)
    Stub = stub_class(mod)
    rec = {}

    def run(name, fn):
        e = Stub(t)
        made = fn(e)   # (the tensors handed in)
        with recording(e) as calls:
            made(e)
        assert calls, name
        rec[name] = calls

    for m in methods(t, mod):
        for without in [()] + [(k,) for k in m.optional if k in m.shapes]:
            run("%s without %s" % (m.name, without[0]) if without else m.name,
                lambda e, m=m, without=without: (lambda e, a=m.args(e, without): m.call(e, a)))
        for k in m.own_copy:
            def strided(e, m=m, k=k):
                a = m.args(e)
                a[k] = e.T(k, *a[k].shape[:-1], 2 * a[k].shape[-1])[..., ::2]
                assert not a[k].is_contiguous()
                return lambda e: m.call(e, a)
            run("%s strided %s" % (m.name, k), strided)
    if not t.n_muscles:   # a model without muscles ignores muscle_act, whatever it is (the step; the read-outs: through autograd)
        for m in methods(t, mod):
            if "act" in m.shapes and not m.name.startswith("joint_dynamics"):
                run("%s ignored muscle_act" % m.name,
                    lambda e, m=m: (lambda e, a=dict(m.args(e), muscle_act=e.T("muscle_act", 5)): m.call(e, a)))
    for name, fn in autograd_cases(t, mod):
        run("autograd " + name, lambda e, fn=fn: fn)
    return rec


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def _header_pointers(fn):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsim.h")).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % fn, src).group(1).split(",")
    names = [p.split()[-1].lstrip("*") for p in params if "*" in p]
    assert names[0] == "m" and names[-1] == "hip_stream", names
    return names[1:-1], len(params)


@pytest.mark.parametrize("name", sorted(engine_module.READOUTS))
def test_readout_table_matches_the_header(name):
    r = engine_module.READOUTS[name]
    ins, outs = [i[0] for i in r.inputs], [o[0] for o in r.outputs]
    fwd, n_fwd = _header_pointers(r.forward)
    bwd, n_bwd = _header_pointers(r.backward)
    assert fwd == ins + outs
    assert bwd == ins + ["g" + o for o in outs] + ["g" + i for i in ins]
    assert len(fwd) + 3 == n_fwd == len(capi.ABI[r.forward][1])       # + m, n_envs, hip_stream
    assert len(bwd) + 3 == n_bwd == len(capi.ABI[r.backward][1])


# ---- (b), (d) ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return {model: valid_calls(model, engine_module) for model in MODELS}


def _role(a):
    return a[0] if isinstance(a, list) else a


@pytest.mark.parametrize("model", MODELS)
def test_valid_calls_have_the_arguments_of_the_abi(recorded, model):
    for case, calls in recorded[model].items():
        for c in calls:
            assert len(c[1:]) + 1 == len(capi.ABI[c[0]][1]), (case, c[0])   # + hip_stream, which _call appends
            assert c[1] == "model"


@pytest.mark.parametrize("model", MODELS)
def test_valid_calls_hand_every_pointer_the_tensor_of_its_role(recorded, model):
    """the pointer arguments of a recorded call, in the header's order: an input carries the role of the header's name, or is None
    where it was None or dropped; what the engine allocates is "new" (no elements: "empty")"""
    t = template_from_golden(model)
    checked = 0
    for case, calls in recorded[model].items():
        if case.startswith("autograd") or " strided " in case:
            continue
        for c in calls:
            if c[0] == "dsim_model_set_params":
                assert _role(c[3]) == engine_module.StepParameters.FIELDS[c[2]]
                continue
            for name, a in _pointers(c).items():
                if _role(a) not in ("new", "empty", None):
                    assert _role(a) == {"q_in": "q", "qd_in": "qd"}.get(name, name), (case, c[0], name, a)
                    checked += 1
                if name == "muscle_act" and t.n_muscles == 0:
                    assert a is None, (case, c[0])
                if name in ("q", "q_in") or (name == "ckpt" and not c[0].endswith("_forward")):
                    assert a is not None, (case, c[0])
    assert checked > 100


def _pointers(c):
    """{name in the header: what was recorded} for the float pointers of a recorded call (not the model, the spec, the episode)"""
    names = [n for n in _header_pointers(c[0])[0] if n not in ("env", "episode")]
    ptrs = [a for a, ty in zip(c[1:], capi.ABI[c[0]][1]) if ty is capi.C.c_void_p][1:]
    assert len(ptrs) == len(names), c[0]
    return dict(zip(names, ptrs))


def _shape(rec, case, fn, arg):
    (c,) = [c for c in rec[case] if c[0] == fn]
    a = _pointers(c)[arg]
    return None if a is None else tuple(a[3])


@pytest.mark.parametrize("model", MODELS)
def test_allocated_outputs_have_the_shapes_of_the_interface(recorded, model):
    t = template_from_golden(model)
    nq, nd, M, L, Cn = t.n_q, t.n_qd, t.n_muscles, t.n_links, t.n_contacts
    rec = recorded[model]
    want = {
        ("body_kinematics_forward", "dsim_body_kinematics"): dict(X_sc=(N * L, 7), X_sm=(N * L, 7), v_s=(N * L, 6)),
        ("body_kinematics_forward without qd", "dsim_body_kinematics"): dict(X_sc=(N * L, 7), X_sm=(N * L, 7), v_s=None),
        ("body_kinematics_backward", "dsim_body_kinematics_backward"): dict(gq=(N * nq,), gqd=(N * nd,)),
        ("body_kinematics_backward without qd", "dsim_body_kinematics_backward"): dict(gq=(N * nq,), gqd=None),
        ("joint_dynamics_forward", "dsim_joint_dynamics"): dict(tau=(N * nd,), qdd=(N * nd,), f_s=(N * L, 6)),
        ("joint_dynamics_backward without act", "dsim_joint_dynamics_backward"):
            dict(gq=(N * nq,), gqd=(N * nd,), gact=(N * nd,), gmuscle_act=(N * M,) if M else None),
        ("ground_contacts_forward", "dsim_ground_contacts"):
            dict(point=(N * Cn, 3), vel=(N * Cn, 3), force=(N * Cn, 3), link_wrench=(N * L, 6)),
        ("ground_contacts_backward", "dsim_ground_contacts_backward"): dict(gq=(N * nq,), gqd=(N * nd,)),
        ("mass_matrix_forward", "dsim_mass_matrix"): dict(H=(N, nd, nd), Hinv=(N, nd, nd), S=(N * nd, 6)),
        ("mass_matrix_backward", "dsim_mass_matrix_backward"): dict(gq=(N * nq,)),
        ("backward", "dsim_step_backward"): dict(gq_in=(N * nq,), gqd_in=(N * nd,), gact=(N * nd,), gmuscle_act=(N * M,) if M else None),
        ("backward_literal", "dsim_step_backward_literal"): dict(gq_in=(N * nq,), scratch=(N, LITERAL_SCRATCH)),
        ("backward_multi_shared", "dsim_step_backward_multi"):
            dict(gq_in=(N, K, nq), gqd_in=(N, K, nd), gact=(N, K, nd), gmuscle_act=(N, K, M) if M else None),
        ("step_jacobian", "dsim_step_jacobian"):
            dict(J_state=(N, nq + nd, nq + nd), J_act=(N, nq + nd, nd), J_muscle=(N, nq + nd, M) if M else None),
        ("backward_params_10", "dsim_step_backward_params"): dict(g_dof=(N, 5, nd), g_contact=None),
        ("backward_params_01", "dsim_step_backward_params"): dict(g_dof=None, g_contact=(N, Cn, 4)),
        ("forward", "dsim_step_forward"): dict(q_out=(N, nq), qd_out=(N * nd,), ckpt=(N, WORDS)),
        ("forward_no_ckpt", "dsim_step_forward"): dict(ckpt=None),
        ("env_forward_episode", "dsim_env_step_forward"): dict(q_out=(N, nq), qd_out=(N * nd,), obs=(N, N_OBS), rew=(N,), ckpt=(N, WORDS)),
        ("env_forward_no_ckpt", "dsim_env_step_forward"): dict(obs=(N, N_OBS), ckpt=None),
        ("env_backward", "dsim_env_step_backward"): dict(gq_in=(N * nq,), gqd_in=(N * nd,), gactions=(N, N_ACT)),
        ("env_observe", "dsim_env_observe"): dict(obs=(N, N_OBS), rew=(N,)),
    }
    for (case, fn), shapes in want.items():
        for arg, shape in shapes.items():
            assert _shape(rec, case, fn, arg) == shape, (case, arg)
    assert rec["env_forward_episode"][0][-1][0] == "Episode" and rec["env_forward_no_ckpt"][0][-1] is None


@pytest.mark.parametrize("model", MODELS)
def test_the_library_is_driven_as_by_the_previous_engine(recorded, model):
    """(d): call for call what the engine.py before the read-out table recorded for the same cases"""
    want = json.load(open(GOLDEN))[model]
    got = json.loads(json.dumps(recorded[model]))
    assert sorted(got) == sorted(want)
    mismatches = [(case, a, b) for case in want for a, b in zip(got[case], want[case]) if a != b]
    mismatches += [case for case in want if len(got[case]) != len(want[case])]
    print("%s: %d recorded calls compared, %d mismatches" % (model, sum(len(v) for v in want.values()), len(mismatches)))
    assert not mismatches, mismatches[:3]


def test_direct_joint_dynamics_drops_muscle_act_on_a_model_without_muscles():
    """the one call that differs from the previous engine.py on purpose, and so is not part of (d): joint_dynamics_forward /
    _backward called directly with a muscle_act tensor on CartPole used to pass its pointer on; NULL now, as through autograd"""
    t = template_from_golden("cartpole")
    for m in methods(t, engine_module):
        if m.name.startswith("joint_dynamics"):
            e = stub_class(engine_module)(t)
            a = dict(m.args(e), muscle_act=e.T("muscle_act", 5))
            with recording(e) as calls:
                out = m.call(e, a)
            (c,) = calls
            p = _pointers(c)
            assert p["muscle_act"] is None and _role(p["act"]) == "act" and len(c[1:]) + 1 == len(capi.ABI[c[0]][1])
            assert m.name.endswith("forward") or out[3] is None   # (no gradient buffer for it either)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _refusals(model):
    """(id, method, argument, how it is spoiled) for every tensor argument of every method that the model does not ignore"""
    t, other = template_from_golden(model), template_from_golden(MODELS[1 - MODELS.index(model)])
    mine, theirs = {m.name: m for m in methods(t, engine_module)}, {m.name: m for m in methods(other, engine_module)}
    out = []
    for m in mine.values():
        for k, v in m.shapes.items():
            numel = 1
            for s in v:
                numel *= s if isinstance(s, int) else 1
            if numel == 0:
                continue   # (nothing to get wrong: contact slots of a model without contacts)
            hows = ["short", "dtype"] + ([] if k in m.own_copy else ["strided"])
            # (joint_q alone, in the other model's size: another number of environments if it divides, and as such accepted)
            if theirs[m.name].shapes.get(k, v) != v and not (len(m.shapes) == 1 and N * other.n_q % t.n_q == 0):
                hows.append("other")
            out += [("%s-%s-%s" % (m.name, k, how), m.name, k, how) for how in hows]
    return out


def _spoil(e, m, k, how, other):
    a = m.args(e)
    t = a[k]
    if how == "short":
        a[k] = e.T(k, t.numel() - 1, dtype=t.dtype)
    elif how == "dtype":
        a[k] = e.T(k, *t.shape, dtype=torch.float64 if t.dtype == torch.float32 else torch.float32)
    elif how == "strided":
        a[k] = e.T(k, *t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]
    else:
        a[k] = other.args(e)[k]
    return a


@pytest.mark.parametrize("model", MODELS)
def test_spoiled_arguments_are_refused_before_any_call(model):
    t, other = template_from_golden(model), template_from_golden(MODELS[1 - MODELS.index(model)])
    mine, theirs = {m.name: m for m in methods(t, engine_module)}, {m.name: m for m in methods(other, engine_module)}
    Stub = stub_class(engine_module)
    cases = _refusals(model)
    assert len(cases) > 150
    for cid, name, k, how in cases:
        e = Stub(t)
        a = _spoil(e, mine[name], k, how, theirs[name])
        with recording(e) as calls:
            with pytest.raises(capi.DsimError):
                mine[name].call(e, a)
                pytest.fail("%s was accepted" % cid)
        assert calls == [], cid


@pytest.mark.parametrize("model", MODELS)
def test_missing_required_arguments_are_refused_before_any_call(model):
    """None where the library needs a tensor: DsimError, not a NULL handed to a kernel"""
    t = template_from_golden(model)
    Stub = stub_class(engine_module)
    n = 0
    for m in methods(t, engine_module):
        for k in m.shapes:
            if k in m.optional or m.name == "body_transforms":   # (body_transforms detaches q first: AttributeError on None)
                continue
            e = Stub(t)
            a = m.args(e, (k,))
            with recording(e) as calls:
                with pytest.raises(capi.DsimError):
                    m.call(e, a)
                    pytest.fail("%s without %s was accepted" % (m.name, k))
            assert calls == [], (m.name, k)
            n += 1
    assert n > 40


def test_set_params_names_the_elements():
    e = stub_class(engine_module)(template_from_golden("snu"))
    with pytest.raises(capi.DsimError, match="joint_target_ke has 3 elements"):
        e.set_params([e.T("joint_target_ke", 3)] + [None] * 5)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
READS = [("body_kinematics", ("q", "qd"), 3), ("body_kinematics", ("q",), 2), ("joint_dynamics", ("q", "qd", "act", "muscle_act"), 3),
         ("ground_contacts", ("q", "qd"), 4), ("mass_matrix", ("q",), 3)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name,inputs,n_out", READS, ids=["%s-%d" % (r[0], len(r[1])) for r in READS])
def test_autograd_asks_only_for_what_the_loss_reads(model, name, inputs, n_out):
    t = template_from_golden(model)
    r = engine_module.READOUTS[name]
    shapes = dict(q=(N, t.n_q), qd=(N, t.n_qd), act=(N, t.n_qd), muscle_act=(N, max(t.n_muscles, 1)))
    for read in [()] + [(i,) for i in range(n_out)]:
        e = stub_class(engine_module)(t)
        x = [e.T(k, *shapes[k]).requires_grad_() for k in inputs]
        through, raw = [], getattr(e, name + "_backward")   # autograd goes through the public method: a caller can wrap it
        setattr(e, name + "_backward", lambda *a: (through.append(a), raw(*a))[1])
        with recording(e) as calls:
            outs = getattr(e, name)(*x)
            assert len(outs) == len(r.outputs) and all(o is not None for o in outs[:n_out]) and all(o is None for o in outs[n_out:])
            (_loss(outs, read) if read else x[0].sum() * 0).backward()
        fwd, bwd = [c for c in calls if c[0] == r.forward], [c for c in calls if c[0] == r.backward]
        assert len(fwd) == 1 and len(calls) == len(fwd) + len(bwd) and len(through) == len(bwd)
        empty = bool(read) and outs[read[0]].numel() == 0   # contacts of a model without any: nothing to differentiate
        if not read:
            assert bwd == []
            continue
        (c,) = bwd
        cots = c[3 + len(r.inputs):3 + len(r.inputs) + len(r.outputs)]
        assert [g is not None for g in cots] == [i == read[0] and not empty for i in range(len(r.outputs))], (read, cots)
        for v, (k, _, _) in zip(x, r.inputs):
            if k == "muscle_act" and t.n_muscles == 0:
                assert v.grad is None
            else:
                assert v.grad.shape == v.shape == (N, v.shape[1])


if __name__ == "__main__":   # python tests/test_engine_binding_cpu.py ENGINE.py OUT.json: the calls of (d) from that version of the file
    spec = importlib.util.spec_from_file_location("diffrl_amd._engine_recorded", sys.argv[1])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    rec = {model: valid_calls(model, mod) for model in MODELS}
    json.dump(rec, open(sys.argv[2], "w"), separators=(",", ":"))
    print({m: (len(v), sum(len(c) for c in v.values())) for m, v in rec.items()})
