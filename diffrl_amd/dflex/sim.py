"""`SemiImplicitIntegrator`: the operator boundary of the reference (dflex/dflex/sim.py:2157-2221).

`forward(model, state, dt, substeps, mass_matrix_freq)` advances all environments by one control step
with ONE fused HIP launch (and registers ONE autograd node whose backward is one fused adjoint
launch), instead of ~100 kernel launches + ~280 tensor allocations per step in the reference
(SURVEY.md section 3.2)."""
import torch

from ..engine import EnvStepParameters, SimStep, SimStepEnvParams, SimStepParams
from . import config
from .model import Model, ModelBuilder, State  # noqa: F401  (re-exported like dflex.sim)


class SemiImplicitIntegrator:
    def __init__(self):
        pass

    def forward(self, model: Model, state_in: State, dt: float, substeps: int, mass_matrix_freq: int, params=None) -> State:
        """params (Model.step_parameters(), optional): the step runs under these gains, targets, limit springs and contact
        materials and is differentiable in them too -- the parameter tensors that require grad receive gradients summed over the
        environments (engine.SimStepParams).  The values are SET on the model (device-to-device, on the current stream) and stay
        set: every later launch on it, the fused env steps and the read-outs included, runs under what was set last, until
        model.engine().reset_params().  Without params: the path as it always was, under whatever the model holds.
        params = Model.step_parameters(per_env=True) (an engine.EnvStepParameters): row e of every tensor is environment e's
        value, and a tensor that requires grad receives in row e the gradient of environment e's outputs -- nothing is summed
        (engine.SimStepEnvParams).  The first such call reserves the model's per-environment block: make it before a graph
        capture (Engine.set_env_params)."""
        eng = model.engine()
        mact = model.muscle_activation if model.muscle_count else None
        out = State(act_like=model.joint_qd, model=model)
        if params is not None and not config.no_grad:
            if config.literal_quat_grad:
                raise RuntimeError("params: there is no literal-quaternion variant of the parameter adjoint (include/dsim.h)")
            node = SimStepEnvParams if isinstance(params, EnvStepParameters) else SimStepParams
            out.joint_q, out.joint_qd = node.apply(eng, float(dt), int(substeps), int(mass_matrix_freq), state_in.joint_q,
                                                   state_in.joint_qd, state_in.joint_act, mact, *params.tensors())
        elif config.no_grad:
            if params is not None:
                (eng.set_env_params if isinstance(params, EnvStepParameters) else eng.set_params)(params)
            with torch.no_grad():
                q, qd, _ = eng.forward(state_in.joint_q.contiguous(), state_in.joint_qd.contiguous(),
                                       state_in.joint_act.contiguous(), mact.contiguous() if mact is not None else None,
                                       float(dt), int(substeps), int(mass_matrix_freq), False)
            out.joint_q, out.joint_qd = q, qd
        else:
            out.joint_q, out.joint_qd = SimStep.apply(eng, float(dt), int(substeps), int(mass_matrix_freq),
                                                      state_in.joint_q, state_in.joint_qd, state_in.joint_act, mact)
        out._xf_q = eng.last_q_in if not config.no_grad else None   # None in no-grad mode (State.body_X_sc then derives from out.joint_q)
        if config.verify_fp and not (torch.isfinite(out.joint_q).all() and torch.isfinite(out.joint_qd).all()):
            raise FloatingPointError("non-finite state after SemiImplicitIntegrator.forward")
        return out

    def linearize(self, model: Model, state_in: State, dt: float, substeps: int, mass_matrix_freq: int):
        """The step and its Jacobian around state_in: (state_out, A, B) -- for a muscle model (state_out, A, B, B_muscle) -- with
        A [n_envs, K, K] = d (q', qd') / d (q, qd), B [n_envs, K, n_qd] = d (q', qd') / d joint_act and B_muscle [n_envs, K, M]
        = d (q', qd') / d muscle_activation, K = n_q + n_qd, rows (q' | qd'), columns of A (q | qd).  One forward launch that
        keeps its checkpoint and one Jacobian launch (Engine.step_jacobian); everything returned is detached.  The derivative
        is the one the adjoint defines (include/dsim.h, dsim_step_jacobian): the quaternion blocks of A's q columns are tangent."""
        eng = model.engine()
        mact = model.muscle_activation.detach().contiguous() if model.muscle_count else None
        act = state_in.joint_act.detach().contiguous()
        dt, substeps, mm = float(dt), int(substeps), int(mass_matrix_freq)
        with torch.no_grad():
            q, qd, ckpt = eng.forward(state_in.joint_q.detach().contiguous(), state_in.joint_qd.detach().contiguous(), act, mact,
                                      dt, substeps, mm, True, keep_q_in=True)
            A, B, Bm = eng.step_jacobian(ckpt, act, mact, dt, substeps, mm)
        out = State(act_like=model.joint_qd, model=model)
        out.joint_q, out.joint_qd = q.view(state_in.joint_q.shape), qd.view(state_in.joint_qd.shape)
        out._xf_q = eng.last_q_in
        return (out, A, B, Bm) if model.muscle_count else (out, A, B)
