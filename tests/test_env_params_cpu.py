"""CPU: the binding layer of the per-environment step parameters (Engine.set_env_params / reset_params / fold_param_grads with
per_env=True), driven through the recording stand-in of the HIP library (tests/engine_stub.py): which calls reach the library, with
which tensors, and what is refused before any of them.

The fold is held against tests/par_lib.py's float64 fold of what the lane-serial host build of dsim_bwd_param_kernel's phase code
returns for the Ant and Humanoid fixtures: 1e-5 in each tensor's max-norm (a link sums at most three float32 terms, 3 x 2^-24
relative; the sum over the fixture's environments a few more)."""
import json
import os

import numpy as np
import pytest
import torch

import diffrl_amd.engine as engine_module
import par_lib as P
from diffrl_amd import capi
from engine_stub import recording, stub_class
from oracle_lib import relerr, template_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = engine_module.StepParameters.FIELDS
N = 3


def _stub(model="snu"):
    t = template_from_golden(model)
    return t, stub_class(engine_module)(t)


def _shapes(t, n=None):
    lead = () if n is None else (n,)
    return dict(zip(F, [lead + (t.n_links,)] * 4 + [lead + (t.n_q,), lead + (t.n_contacts, 4)]))


@pytest.mark.parametrize("model", ["cartpole", "snu"])
def test_set_env_params_records_the_reservation_and_one_call_per_field(model):
    t, e = _stub(model)
    sh = _shapes(t, N)
    a = {k: e.T(k, *sh[k]) for k in F}
    with recording(e) as calls:
        e.set_env_params(engine_module.EnvStepParameters(**a))
    assert calls[0] == ["dsim_model_reserve_env_params", "model", N]
    fields = [f for f in range(6) if f < 5 or t.n_contacts]   # (the contact field of a model without contacts: no call)
    assert [c[0] for c in calls[1:]] == ["dsim_model_set_env_params"] * len(fields)
    for c, f in zip(calls[1:], fields):
        assert c[1:4] == ["model", f, N]
        assert c[4] == [F[f], int(np.prod(sh[F[f]])), "torch.float32", list(sh[F[f]])]
    # the same n again: no second reservation; None entries are left out
    with recording(e) as calls:
        e.set_env_params([a[F[0]], None, None, None, a[F[4]], None])
    assert [c[:4] for c in calls] == [["dsim_model_set_env_params", "model", 0, N], ["dsim_model_set_env_params", "model", 4, N]]
    # another n: reserved again
    b = e.T(F[1], N + 1, t.n_links)
    with recording(e) as calls:
        e.set_env_params([None, b, None, None, None, None])
    assert calls == [["dsim_model_reserve_env_params", "model", N + 1],
                     ["dsim_model_set_env_params", "model", 1, N + 1, [F[1], (N + 1) * t.n_links, "torch.float32", [N + 1, t.n_links]]]]
    # back to one shared block: the block is released, then the template's values are set as set_params sets them
    with recording(e) as calls:
        e.reset_params()
    assert calls[0] == ["dsim_model_reserve_env_params", "model", 0]
    assert all(c[0] == "dsim_model_set_params" for c in calls[1:]) and len(calls) == 1 + len(fields)
    with recording(e) as calls:
        e.reset_params()
    assert all(c[0] == "dsim_model_set_params" for c in calls) and len(calls) == len(fields)


@pytest.mark.parametrize("off", [-1, 1])
def test_a_tensor_of_the_wrong_size_is_refused_before_any_call(off):
    t, e = _stub()
    sh = _shapes(t, N)
    a = {k: e.T(k, *sh[k]) for k in F}
    a[F[4]] = e.T(F[4], N, t.n_q + off)            # the fifth field is wrong: the four before it must not have been copied
    with recording(e) as calls:
        with pytest.raises(capi.DsimError, match="elements"):
            e.set_env_params([a[k] for k in F])
        assert calls == []
        flat = e.T(F[0], N * t.n_links + off)      # no environment dimension to read n from
        with pytest.raises(capi.DsimError):
            e.set_env_params([flat] + [None] * 5)
        assert calls == []


def test_fields_that_disagree_on_the_environments_are_refused_before_any_call():
    t, e = _stub()
    with recording(e) as calls:
        with pytest.raises(capi.DsimError, match="environment dimension"):
            e.set_env_params([e.T(F[0], N, t.n_links), e.T(F[1], N + 1, t.n_links)] + [None] * 4)
        with pytest.raises(capi.DsimError):
            e.set_env_params([None] * 6)
        with pytest.raises(capi.DsimError, match="six tensors"):
            e.set_env_params([e.T(F[0], N, t.n_links)])
        assert calls == []


@pytest.mark.parametrize("model", ["cartpole", "snu"])
def test_shared_set_params_records_what_it_recorded_before(model):
    t, e = _stub(model)
    sh = _shapes(t)
    a = {k: e.T(k, *sh[k]) for k in F}
    with recording(e) as calls:
        e.set_params([a[k] for k in F])
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_binding_calls.json")))[model]["set_params"]
    assert json.loads(json.dumps(calls)) == golden


def test_env_step_parameters_expand_the_template():
    t, e = _stub()
    p = e.env_step_parameters(N)
    assert isinstance(p, engine_module.EnvStepParameters) and isinstance(p, engine_module.StepParameters)
    sh = _shapes(t, N)
    for k, x, x0 in zip(F, p.tensors(), e.step_parameters().tensors()):
        assert tuple(x.shape) == sh[k] and x.is_contiguous() and x.dtype == torch.float32
        assert all(torch.equal(x[i], x0) for i in range(N))


@pytest.mark.parametrize("name", ["ant", "humanoid"])
def test_fold_per_environment(name):
    t, g, (act, mact) = P.case(name)
    dt, S, mm = float(g["dt"]), int(g["substeps"]), int(g["mm_freq"])
    _, _, ck = P.emu_par_forward(t, g["q_in"], g["qd_in"], act, mact, dt, S, mm)
    par = P.emu_par_backward(t, ck, act, mact, dt, S, mm, g["gq_out"], g["gqd_out"])
    e = stub_class(engine_module)(t)
    g_dof, g_con = torch.tensor(par["g_dof"]), torch.tensor(par["g_contact"])
    B = g_dof.shape[0]
    per = e.fold_param_grads(g_dof, g_con, per_env=True)
    tot = e.fold_param_grads(g_dof, g_con)
    ref = P.fold(t, name, par["g_dof"], None)
    for f, k in enumerate(("g_target_ke", "g_target_kd", "g_limit_ke", "g_limit_kd", "g_target")):
        assert tuple(per[f].shape) == (B, t.n_q if k == "g_target" else t.n_links), k
        if np.abs(ref[k]).max() > 0:
            err = relerr(per[f].numpy(), ref[k])
            print("%s %s per-environment fold err %.2e" % (name, k, err))
            assert err < 1e-5, (k, err)
        else:
            assert not per[f].any(), k
    assert tuple(per[5].shape) == (B, t.n_contacts, 4) and torch.equal(per[5], g_con)
    for f in range(6):
        assert tuple(tot[f].shape) == tuple(per[f].shape[1:])
        if float(tot[f].abs().max()) > 0:
            err = relerr(per[f].sum(0).numpy(), tot[f].numpy())
            print("%s field %d sum over environments err %.2e" % (name, f, err))
            assert err < 1e-5, (f, err)
    # `need` leaves fields out in both forms
    some = e.fold_param_grads(g_dof, g_con, need=(True, False, False, False, True, False), per_env=True)
    assert [x is not None for x in some] == [True, False, False, False, True, False]
    assert torch.equal(some[0], per[0]) and torch.equal(some[4], per[4])


def test_abi_version_is_unchanged():
    assert capi.EXPECTED_ABI == 110
    for fn in ("dsim_model_reserve_env_params", "dsim_model_env_params", "dsim_model_set_env_params"):
        assert fn in capi.ABI
