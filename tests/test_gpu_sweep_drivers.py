"""-m gpu: dsim_step_backward and dsim_env_step_backward on the same checkpoint (tests/sweep_drivers.py: why they must agree, the
inputs, the bounds).  One reverse sweep serves both launches; the models and switches below each take another branch of what
the two drivers leave to it: who requested the last substep's row, and where the last group's inverse comes from."""
import pytest
import torch

import sweep_drivers as SD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [
    ("ant", "full", {}),                                             # helper wave; the helper brings the last group's inverse
    ("ant", "full", dict(DSIM_HELPER="0", DSIM_PAIR="0")),           # one wave, inverse loaded on the spot
    ("humanoid", "full", {}),
    ("snu", "full", {}),                                             # four waves, rows by the body level, inverse in registers
    ("cartpole", "full", {}),
    ("ant", "full", dict(DSIM_FORCE_GENERIC="1")),                   # no early loads: the row is requested inside the sweep
    ("ant", "lean", {}),
    ("snu", "lean", {}),
]
_engines = {}


def _engine(env, ckpt_mode, kw):
    key = (env, ckpt_mode) + tuple(sorted(kw.items()))
    if key not in _engines:
        from diffrl_amd.engine import Engine
        with SD.switches(**kw):
            _engines[key] = Engine(SD.case(env)["t"], DEV, ckpt_mode=ckpt_mode)
    return _engines[key]


def _T(a):
    return torch.tensor(a, device=DEV).reshape(-1) if a is not None else None


@pytest.mark.parametrize("mm", SD.MMS)
@pytest.mark.parametrize("env,ckpt_mode,kw", MODES, ids=["-".join([m[0], m[1]] + ["%s=%s" % i for i in sorted(m[2].items())]) for m in MODES])
def test_env_adjoint_equals_step_adjoint_on_one_checkpoint(env, ckpt_mode, kw, mm):
    c = SD.case(env)
    eng = _engine(env, ckpt_mode, kw)
    assert (eng.variant == 0) == ("DSIM_FORCE_GENERIC" in kw)
    spec = type(c["spec"]).from_buffer_copy(c["spec"])
    scale = torch.tensor(c["scale"], device=DEV)
    spec.act_scale = scale.data_ptr()
    n = SD.N
    actions, act, mact = torch.tensor(c["actions"], device=DEV), _T(c["act"]), _T(c["mact"])
    qo, qdo, obs, rew, ck = eng.env_forward(spec, _T(c["q"]), _T(c["qd"]), actions, SD.M.DT, SD.M.S, mm, True)
    sq, sqd, _ = eng.forward(_T(c["q"]), _T(c["qd"]), act, mact, SD.M.DT, SD.M.S, mm, False)
    assert torch.equal(qo, sq) and torch.equal(qdo, sqd), "the step forward on the derived actuation is the fused forward"
    gq, gqd = _T(c["gq"]), _T(c["gqd"])
    step = eng.backward(ck, act, mact, SD.M.DT, SD.M.S, mm, gq, gqd)
    fused = eng.env_backward(spec, ck, actions, SD.M.DT, SD.M.S, mm, gq, gqd, torch.zeros_like(obs), torch.zeros_like(rew))
    torch.cuda.synchronize()
    eng.status()
    host = lambda x: x.cpu().numpy().reshape(n, -1) if x is not None else None  # noqa: E731
    SD.assert_drivers_agree(env, tuple(host(x) for x in step), tuple(host(x) for x in fused),
                            label="gpu %s mm=%d %s" % (ckpt_mode, mm, " ".join("%s=%s" % i for i in sorted(kw.items()))))
