"""Host harness: the step adjoint and the fused environment adjoint on the same checkpoint (tests/sweep_drivers.py: why they
must agree, the inputs, the bounds), with the generic layout on one wave and with each model's compile-time layout on the
wavefronts the library picks for it, full and lean checkpoints."""
import numpy as np
import pytest

import sweep_drivers as SD
from emu_lib import emu, emu_env_backward, emu_env_forward, mode, step_backward, step_forward, waves_of

# (model, static, lean)
MODES = [(env, static, False) for env in ("ant", "humanoid", "snu", "cartpole") for static in (False, True)]
MODES += [("ant", True, True), ("snu", True, True)]


@pytest.mark.parametrize("mm", SD.MMS)
@pytest.mark.parametrize("env,static,lean", MODES)
def test_env_adjoint_equals_step_adjoint_on_one_checkpoint(env, static, lean, mm):
    c = SD.case(env)
    t, S, DT = c["t"], SD.M.S, SD.M.DT
    waves = waves_of(t) if static else 1
    with mode(emu(), static, waves, lean):
        qo, qdo, obs, rew, ck = emu_env_forward(t, c["spec"], c["q"], c["qd"], c["actions"], DT, S, mm)
        fused = emu_env_backward(t, c["spec"], ck, c["actions"], DT, S, mm, c["gq"], c["gqd"], np.zeros_like(obs), np.zeros_like(rew))
    sq, sqd, _ = step_forward(t, c["q"], c["qd"], c["act"], c["mact"], DT, S, mm, static=static, waves=waves, lean=lean, want_ckpt=False)
    assert np.array_equal(qo, sq) and np.array_equal(qdo, sqd), "the step forward on the derived actuation is the fused forward"
    r = step_backward(t, ck, c["act"], c["mact"], DT, S, mm, c["gq"], c["gqd"], static=static, waves=waves, lean=lean)
    SD.assert_drivers_agree(env, (r["gq"], r["gqd"], r["gact"], r["gmact"]), fused,
                            label="host %s %d wave(s) %s mm=%d" % ("static" if static else "generic", waves, "lean" if lean else "full", mm))
