"""Torch-facing wrapper of the HIP library: device memory + stream plumbing and the autograd node.

`SimStep` replaces `dflex.sim.SimulateFunc` (dflex/dflex/sim.py:2086-2154): one autograd node per
env.step(); forward = one fused kernel launch over all substeps, backward = one fused adjoint launch.

The C ABI takes bare pointers and cannot check sizes: every tensor handed to it goes through Engine._arg first.
"""
import collections
import ctypes as C
import math

import torch

from . import capi
from .template import ArticulationTemplate


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class StepParameters:
    """The model parameters the step is differentiable in, as device tensors shared by all environments: joint_target_ke,
    joint_target_kd, joint_limit_ke, joint_limit_kd [n_links], joint_target [n_q], contact_material [C, 4] (ke, kd, kf, mu per
    contact slot).  Engine.step_parameters() clones them from the template; set requires_grad on the ones to fit."""
    FIELDS = ("joint_target_ke", "joint_target_kd", "joint_limit_ke", "joint_limit_kd", "joint_target", "contact_material")

    def __init__(self, **tensors):
        for k in self.FIELDS:
            setattr(self, k, tensors[k])

    def tensors(self):
        """in the order of DSIM_PARAM_* (include/dsim.h)"""
        return tuple(getattr(self, k) for k in self.FIELDS)


class EnvStepParameters(StepParameters):
    """StepParameters with a value PER ENVIRONMENT: the same six fields with a leading environment dimension, joint_target_ke /
    joint_target_kd / joint_limit_ke / joint_limit_kd [N, n_links], joint_target [N, n_q], contact_material [N, C, 4].
    Engine.env_step_parameters(N) expands the template's values; Engine.set_env_params puts them on the model."""


# The differentiable read-outs of a state handed in: one row per pair of C functions, names as the parameters of include/dsim.h
# (the backward's cotangents and gradients are "g" + name; tests/test_engine_binding_cpu.py holds the rows against the header).
#   inputs:  (name, floats per environment, optional).  Sizes are products of n (environments), nq, nd, L (links), C (contacts) and
#            M (muscles).  An optional input may be None: "zeros" -- it counts as zeros and still has a gradient; "absent" -- it and
#            its gradient are not there.  An input the model has no room for (M = 0) is dropped: NULL in, no gradient.
#   outputs: (name, shape as returned[, the optional input without which it is not computed]).
Readout = collections.namedtuple("Readout", "name forward backward inputs outputs")
READOUTS = {r.name: r for r in (
    Readout("body_kinematics", "dsim_body_kinematics", "dsim_body_kinematics_backward",
            (("q", "nq", False), ("qd", "nd", "absent")),
            (("X_sc", ("n*L", 7)), ("X_sm", ("n*L", 7)), ("v_s", ("n*L", 6), "qd"))),
    Readout("joint_dynamics", "dsim_joint_dynamics", "dsim_joint_dynamics_backward",
            (("q", "nq", False), ("qd", "nd", False), ("act", "nd", "zeros"), ("muscle_act", "M", "zeros")),
            (("tau", ("n*nd",)), ("qdd", ("n*nd",)), ("f_s", ("n*L", 6)))),
    Readout("ground_contacts", "dsim_ground_contacts", "dsim_ground_contacts_backward",
            (("q", "nq", False), ("qd", "nd", False)),
            (("point", ("n*C", 3)), ("vel", ("n*C", 3)), ("force", ("n*C", 3)), ("link_wrench", ("n*L", 6)))),
    Readout("mass_matrix", "dsim_mass_matrix", "dsim_mass_matrix_backward",
            (("q", "nq", False),),
            (("H", ("n", "nd", "nd")), ("Hinv", ("n", "nd", "nd")), ("S", ("n*nd", 6)))),
)}


class Engine:
    """Owns the device copy of one articulation template on one GPU."""

    # Parameter epoch: a Python int that set_params, set_env_params, reserve_env_params and reset_params each bump.  EnvStepParams
    # records it in forward and refuses a backward under another one: the checkpoint would be consumed under other values than
    # its forward ran with.
    param_epoch = 0

    def __init__(self, template: ArticulationTemplate, device, ckpt_mode=None, specialise=None):
        """ckpt_mode: "full" (default; $DIFFRL_AMD_CKPT overrides) -- the forward launch streams every intermediate the
        adjoint reads to HBM -- or "lean" -- (q, qd) per substep only, the adjoint recomputes (include/dsim.h).
        specialise: what a model that matches none of the compiled layout tables gets (it would run the generic kernels, about
        half the speed).  True / $DSIM_AUTO_SPECIALISE=1: a kernel set of its own, compiled with hipcc on first use and cached
        next to the library (diffrl_amd.specialise.ensure_library: about a minute, once per model and source version; the
        constructor waits for it).  "background" (the default when None and $DSIM_AUTO_SPECIALISE is unset or "background"): the
        cached set if there is one; otherwise this Engine runs the generic kernels while a detached child process compiles the set, and
        the next Engine of the model picks it up.  False / $DSIM_AUTO_SPECIALISE=0: nothing is compiled or swapped at run time.
        A failed build, a missing hipcc or a library that turns out not to hold the set: a warning, the generic kernels stay."""
        self.template = template
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise capi.DsimError("diffrl_amd runs on MI355X only (device=%s); there is no CPU path" % device)
        self._lib = capi.lib()
        if self.device.index is None:   # "cuda" means the current device; tensors report an explicit index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._desc, self._keep = capi.make_desc(template)
        import os
        if specialise is None:
            v = os.environ.get("DSIM_AUTO_SPECIALISE", "background").lower()
            specialise = False if v in ("", "0", "off") else ("background" if v in ("background", "bg") else True)
            # (a developer override of the library -- A/B builds with a subset of the kernel sets -- is measured as it is: no
            # background swap behind its back)
            if specialise == "background" and os.environ.get("DSIM_LIB"):
                specialise = False
        h = self._create()
        if specialise and int(self._lib.dsim_model_variant(h)) == 0 and os.environ.get("DSIM_FORCE_GENERIC", "0") in ("", "0"):
            import warnings
            from . import specialise as sp
            if specialise == "background":
                path, _ = sp.ensure_library_background(template)   # None: compiling now (or no hipcc): generic kernels this time
            else:
                path = sp.ensure_library(template)   # None: hipcc missing or the build failed (warned about); the generic kernels stay
            # (the library already loaded reports variant 0 for this model: a path equal to it cannot help -- e.g. a product library
            # built with a DSIM_STATIC_VARIANTS subset, or a header regenerated without rebuilding)
            if path is not None and os.path.realpath(path) != os.path.realpath(getattr(self._lib, "_name", "") or ""):
                lib2 = capi.load(path)
                keep_lib, self._lib = self._lib, lib2
                try:
                    h2 = self._create()
                except capi.DsimError as ex:
                    h2, self._lib = None, keep_lib
                    warnings.warn("diffrl_amd: %s could not create this model (%s); it keeps the generic kernels" % (path, ex))
                if h2 is not None:
                    if int(lib2.dsim_model_variant(h2)) > 0:
                        keep_lib.dsim_model_destroy(h)
                        h = h2
                    else:   # keep the working generic handle, release the extra one
                        lib2.dsim_model_destroy(h2)
                        self._lib = keep_lib
                        warnings.warn("diffrl_amd: %s was built for this model but does not match it; it keeps the generic kernels"
                                      % path)
            elif path is not None:
                warnings.warn("diffrl_amd: the loaded library %s lists a kernel set for this model but was built without it; "
                              "it keeps the generic kernels" % path)
        self._h = h
        self.ckpt_mode = (ckpt_mode or os.environ.get("DIFFRL_AMD_CKPT", "full")).lower()
        if self.ckpt_mode not in ("full", "lean"):
            raise capi.DsimError("ckpt_mode must be 'full' or 'lean'")
        with torch.cuda.device(self.device):   # (re-evaluates the occupancy of the helper-wave kernels on the model's device)
            self._ck(self._lib.dsim_model_set_ckpt_mode(h, capi.CKPT_LEAN if self.ckpt_mode == "lean" else capi.CKPT_FULL))
        assert int(self._lib.dsim_model_device(h)) == self.device.index
        self.variant = int(self._lib.dsim_model_variant(h))  # 0 = generic kernels, > 0 = specialised for this model
        self.waves = int(self._lib.dsim_model_waves(h))      # wavefronts per environment of its kernels: 1 or 4
        self.n_q, self.n_qd, self.n_muscles = template.n_q, template.n_qd, template.n_muscles
        # joint_q ENTERING the last substep of the most recent forward() with gradients on ([n_envs, n_q], a copy: n_q floats per
        # environment -- never a reference to the checkpoint itself, which is hundreds of MB for the humanoid and must die with
        # its autograd node): what State.body_X_sc derives the reference's lagging transforms from (dflex/sim.py)
        self.last_q_in = None

    def _ck(self, rc):
        capi.check(rc, self._lib)

    def _call(self, fn, *args):
        """a launching call of the library on this model: its device current, the current stream as the last argument"""
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._ck(fn(*args, st))

    def _new(self, *shape):
        """uninitialised float32 on the model's device"""
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _create(self):
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            self._ck(self._lib.dsim_model_create(C.byref(self._desc), C.byref(h)))
        return h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.dsim_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def status(self):
        """Raises DsimError if a forward launch since the last report was handed a non-unit quaternion (include/dsim.h:
        the path is defined on unit quaternions only).  Host-side read of two mapped words; synchronise first for a
        definitive answer about launches still in flight."""
        self._ck(self._lib.dsim_model_status(self._h, None))

    # ---- what every launch checks ----------------------------------------------------------------------
    def _arg(self, t, numel, name, dtype=torch.float32):
        """the one test of a tensor whose pointer goes to the library: on the model's device, of that dtype, contiguous and of
        EXACTLY numel elements, whatever its shape (the kernels index it with the model's sizes and nothing else)"""
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dtype and t.is_contiguous()):
            raise capi.DsimError("%s must be a contiguous %s tensor on %s" % (name, dtype, self.device))
        if t.numel() != numel:
            raise capi.DsimError("%s has %d elements, not the %d of this model and call" % (name, t.numel(), numel))

    def _state(self, q, *others):
        """n_envs as joint_q (q) gives it; every (tensor, floats per environment, name) of `others` is held to it"""
        n = q.numel() // self.n_q if torch.is_tensor(q) else 0
        self._arg(q, n * self.n_q, "q")
        for t, width, name in others:
            self._arg(t, n * width, name)
        return n

    def _sizes(self, n=1):
        """-> the function that evaluates an entry of READOUTS, e.g. "n*L", "M" or 7, for this model and n environments"""
        t = self.template
        d = dict(n=n, nq=t.n_q, nd=t.n_qd, L=t.n_links, C=t.n_contacts, M=t.n_muscles)
        return lambda dim: dim if isinstance(dim, int) else math.prod(d[k] for k in dim.split("*"))

    # ---- read-outs of a state handed in (READOUTS) -----------------------------------------------------
    def body_transforms(self, q):
        """(X_sc, X_sm), each [n_envs * n_links, 7]: link frames and centre-of-mass frames in the world for the joint
        coordinates q -- the reference's State.body_X_sc / body_X_sm (dflex/dflex/model.py:338-392)."""
        q = q.detach().contiguous()
        n = self._state(q)
        L = self.template.n_links
        xsc = self._new(n * L, 7)
        xsm = self._new(n * L, 7)
        self._call(self._lib.dsim_body_transforms, self._h, n, _ptr(q), _ptr(xsc), _ptr(xsm))
        return xsc, xsm

    def _readout_inputs(self, r, inputs):
        """-> (n_envs, the inputs as they go to the library: checked, the ones the model has no room for dropped)"""
        if len(inputs) != len(r.inputs):
            raise capi.DsimError("%s takes %d inputs" % (r.forward, len(r.inputs)))
        width = self._sizes()
        kept = [t if width(w) else None for t, (_, w, _) in zip(inputs, r.inputs)]
        for t, (name, w, optional) in zip(kept, r.inputs):
            if t is None and width(w) and not optional:
                raise capi.DsimError("%s: %s is not optional" % (r.forward, name))
        n = self._state(kept[0], *[(t, width(w), name) for t, (name, w, _) in zip(kept[1:], r.inputs[1:]) if t is not None])
        return n, kept

    def readout_forward(self, r, *inputs):
        """r.forward on detached contiguous tensors -> one tensor per r.outputs (None: not computed without its input)"""
        n, inputs = self._readout_inputs(r, inputs)
        size = self._sizes(n)
        given = {name: t is not None for t, (name, _, _) in zip(inputs, r.inputs)}
        outs = tuple(self._new(*map(size, o[1])) if len(o) == 2 or given[o[2]] else None for o in r.outputs)
        self._call(getattr(self._lib, r.forward), self._h, n, *map(_ptr, inputs), *map(_ptr, outs))
        return outs

    def readout_backward(self, r, *args):
        """r.backward: args = the inputs, then one cotangent per r.outputs; any cotangent may be None (= zeros, no buffer)
        -> one flat gradient per r.inputs (None for an input that is absent or dropped)"""
        n, inputs = self._readout_inputs(r, args[:len(r.inputs)])
        cots = args[len(r.inputs):]
        if len(cots) != len(r.outputs):
            raise capi.DsimError("%s takes one cotangent (or None) for each of its %d outputs" % (r.backward, len(r.outputs)))
        size = self._sizes(n)
        for g, o in zip(cots, r.outputs):
            if g is not None:
                self._arg(g, math.prod(map(size, o[1])), "g" + o[0])
        grads = tuple(self._new(size("n*" + w)) if size(w) and not (t is None and optional == "absent") else None
                      for t, (_, w, optional) in zip(inputs, r.inputs))
        self._call(getattr(self._lib, r.backward), self._h, n, *map(_ptr, inputs), *map(_ptr, cots), *map(_ptr, grads))
        return grads

    def body_kinematics(self, q, qd=None):
        """(X_sc, X_sm, v_s | None): link frames, centre-of-mass frames ([n_envs * n_links, 7]) and -- if qd is given -- the
        world-frame spatial twists (w, v) of the links about the world origin ([n_envs * n_links, 6], the reference's
        State.body_v_s: the velocity of a point p of a link is v + w x p) of the joint state (q, qd) HANDED IN, differentiable in
        q and qd (ReadoutFunction below; one launch forward, one backward).  body_transforms is the detached read-back."""
        out = ReadoutFunction.apply(self, READOUTS["body_kinematics"], q, qd)
        return out if qd is not None else out + (None,)

    def body_kinematics_forward(self, q, qd=None):
        """dsim_body_kinematics on detached contiguous tensors"""
        return self.readout_forward(READOUTS["body_kinematics"], q, qd)

    def body_kinematics_backward(self, q, qd, gxsc, gxsm, gvs):
        """dsim_body_kinematics_backward: any cotangent may be None (= zeros, no buffer); -> (gq, gqd | None), flat"""
        return self.readout_backward(READOUTS["body_kinematics"], q, qd, gxsc, gxsm, gvs)

    def joint_dynamics(self, q, qd, act=None, muscle_act=None):
        """(tau [n_envs * n_qd], qdd [n_envs * n_qd], f_s [n_envs * n_links, 6]): the generalized force applied (PD target, joint
        limits and actuation included), the joint accelerations H(q)^-1 tau and every link's own world-frame spatial force
        (inertial force minus gravity plus its ground contacts and muscles) -- the reference's State.joint_tau / joint_qdd /
        body_f_s -- of the state and actuation HANDED IN, differentiable in all four inputs (ReadoutFunction below; one launch
        forward, one backward).  act / muscle_act default to zeros.  No step length enters: nothing is integrated."""
        return ReadoutFunction.apply(self, READOUTS["joint_dynamics"], q, qd, act, muscle_act)

    def joint_dynamics_forward(self, q, qd, act=None, muscle_act=None):
        """dsim_joint_dynamics on detached contiguous tensors"""
        return self.readout_forward(READOUTS["joint_dynamics"], q, qd, act, muscle_act)

    def joint_dynamics_backward(self, q, qd, act, muscle_act, gtau, gqdd, gfs):
        """dsim_joint_dynamics_backward: any cotangent may be None (= zeros, no buffer); -> (gq, gqd, gact, gmuscle_act | None), flat"""
        return self.readout_backward(READOUTS["joint_dynamics"], q, qd, act, muscle_act, gtau, gqdd, gfs)

    def ground_contacts(self, q, qd):
        """(point [n_envs * C, 3], vel [n_envs * C, 3], force [n_envs * C, 3], link_wrench [n_envs * n_links, 6]): per ground
        contact, in model order, the point tested against the ground (point[:, 1] is the signed depth, negative = penetrating),
        its velocity and the normal-plus-friction force on it (exactly zero where the depth is >= 0), and per link the sum of
        (point x force, force) over its contacts -- the contact part of the reference's State.body_f_s -- of the state HANDED IN,
        differentiable in q and qd (ReadoutFunction below; one launch forward, one backward)."""
        return ReadoutFunction.apply(self, READOUTS["ground_contacts"], q, qd)

    def ground_contacts_forward(self, q, qd):
        """dsim_ground_contacts on detached contiguous tensors"""
        return self.readout_forward(READOUTS["ground_contacts"], q, qd)

    def ground_contacts_backward(self, q, qd, gpoint, gvel, gforce, glw):
        """dsim_ground_contacts_backward: any cotangent may be None (= zeros, no buffer); -> (gq, gqd), flat"""
        return self.readout_backward(READOUTS["ground_contacts"], q, qd, gpoint, gvel, gforce, glw)

    def mass_matrix(self, q):
        """(H [n_envs, n_qd, n_qd], Hinv [n_envs, n_qd, n_qd], S [n_envs * n_qd, 6]): the joint-space inertia J^T M J + diag(armature)
        that a refresh substep of q inverts (the reference's model.H is without the armature), its Gauss-Jordan inverse with the
        bits the step and joint_dynamics use, and the world-frame motion axis of every dof (State.joint_S_s) -- of the q HANDED IN,
        differentiable in it (ReadoutFunction below; one launch forward, one backward, which asks only for what has a cotangent)."""
        return ReadoutFunction.apply(self, READOUTS["mass_matrix"], q)

    def mass_matrix_forward(self, q):
        """dsim_mass_matrix on a detached contiguous tensor"""
        return self.readout_forward(READOUTS["mass_matrix"], q)

    def mass_matrix_backward(self, q, gH, gHinv, gS):
        """dsim_mass_matrix_backward: any cotangent may be None (= zeros, no buffer); -> gq, flat"""
        return self.readout_backward(READOUTS["mass_matrix"], q, gH, gHinv, gS)[0]

    # ---- the step --------------------------------------------------------------------------------------
    def last_substep_q(self, ckpt, substeps):
        """joint_q ENTERING the last substep of the step that wrote `ckpt` (the head of that substep's checkpoint row): what the
        reference's eval_rigid_fk saw when it filled the returned State's body_X_sc (sim.py:2316-2601)."""
        row = int(self._lib.dsim_ckpt_floats_mm(self._h, 2, 1 << 30)) - int(self._lib.dsim_ckpt_floats_mm(self._h, 1, 1 << 30))
        return ckpt[:, (substeps - 1) * row:(substeps - 1) * row + self.n_q].contiguous()

    def _alloc_ckpt(self, n, substeps, mm_freq):
        """[n][dsim_ckpt_floats_mm]: per substep the saved forward block (starts with q, qd), then the H^-1 per group"""
        words = int(self._lib.dsim_ckpt_floats_mm(self._h, substeps, mm_freq))
        return self._new(n, words)

    def forward(self, q, qd, act, mact, dt, substeps, mm_freq, need_ckpt, keep_q_in=False):
        """keep_q_in: also copy joint_q entering the last substep out of the checkpoint (-> self.last_q_in; one small copy kernel,
        asked for by the operator boundary only: SimStep / SemiImplicitIntegrator.forward)"""
        M = self.n_muscles
        mact = mact if M else None
        n = self._state(q, (qd, self.n_qd, "qd"), (act, self.n_qd, "act"), *([(mact, M, "muscle_act")] if M else []))
        q_out = torch.empty_like(q)
        qd_out = torch.empty_like(qd)
        ckpt = None
        if need_ckpt:
            ckpt = self._alloc_ckpt(n, substeps, mm_freq)
        self.last_q_in = None
        self._call(self._lib.dsim_step_forward, self._h, n, _ptr(q), _ptr(qd), _ptr(act), _ptr(mact),
                   C.c_float(dt), substeps, mm_freq, _ptr(q_out), _ptr(qd_out), _ptr(ckpt))
        if ckpt is not None and keep_q_in:
            self.last_q_in = self.last_substep_q(ckpt, substeps)
        return q_out, qd_out, ckpt

    def _check_ckpt(self, ckpt, substeps, mm_freq):
        """-> n_envs of the checkpoint.  It must be consumed with the geometry (substeps, mass-matrix frequency, checkpoint mode)
        it was written with: the row stride differs otherwise and the adjoint launch would read other rows' words"""
        words = int(self._lib.dsim_ckpt_floats_mm(self._h, substeps, mm_freq))
        if not torch.is_tensor(ckpt) or ckpt.dim() != 2 or ckpt.shape[1] != words:
            raise capi.DsimError("checkpoint of shape %s does not match this model / step geometry (%d floats per environment "
                                 "in '%s' mode)" % (tuple(getattr(ckpt, "shape", ())), words, self.ckpt_mode))
        self._arg(ckpt, ckpt.shape[0] * words, "checkpoint")   # (a strided view, e.g. ckpt[::2], has the right shape and the wrong row stride)
        return ckpt.shape[0]

    def _actuation(self, ckpt, act, mact, substeps, mm_freq):
        """The prologue of every step adjoint, first half: the checkpoint and the actuation it is consumed with
        -> (n_envs, muscle_act | None: a model without muscles ignores it)"""
        n, M = self._check_ckpt(ckpt, substeps, mm_freq), self.n_muscles
        self._arg(act, n * self.n_qd, "act")
        if not M:
            return n, None
        if mact is None:
            raise capi.DsimError("model has muscles but muscle_act is None")
        self._arg(mact, n * M, "muscle_act")
        return n, mact

    def _cotangents(self, n, gq_out, gqd_out, sets=None):
        """Second half: the cotangents, made contiguous, and the gradient buffers in their leading shape
        -> (K, gq_out, gqd_out, (gq, gqd, gact, gmuscle_act | None)).
        sets None: one cotangent pair per environment, K = 1, flat buffers.  Otherwise K pairs in each of `sets` sets -- n_envs,
        or 1 when all environments share them --, K as gq_out's size gives it, buffers [n_envs, K, .]."""
        gq_out, gqd_out = (g.contiguous() if torch.is_tensor(g) else g for g in (gq_out, gqd_out))
        K = 1
        if sets is not None:
            K = gq_out.numel() // (sets * self.n_q) if torch.is_tensor(gq_out) else 0
            if K < 1:
                raise capi.DsimError("gq_out / gqd_out must hold the same number K >= 1 of cotangent rows in each of %d sets" % sets)
        self._arg(gq_out, (sets or n) * K * self.n_q, "gq_out")
        self._arg(gqd_out, (sets or n) * K * self.n_qd, "gqd_out")
        new = (lambda w: self._new(n * w)) if sets is None else (lambda w: self._new(n, K, w))
        return K, gq_out, gqd_out, (new(self.n_q), new(self.n_qd), new(self.n_qd), new(self.n_muscles) if self.n_muscles else None)

    def backward(self, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, literal=False):
        """literal: dsim_step_backward_literal -- the quaternion blocks of the returned gq carry the component along the quaternion
        that the reference's literal adjoint has (one more small launch; default: the wrench form, no such component)"""
        n, mact = self._actuation(ckpt, act, mact, substeps, mm_freq)
        _, gq_out, gqd_out, grads = self._cotangents(n, gq_out, gqd_out)
        fn, scratch = self._lib.dsim_step_backward, ()
        if literal:
            fn, scratch = self._lib.dsim_step_backward_literal, (self._new(n, int(self._lib.dsim_literal_scratch_floats(self._h))),)
        self._call(fn, self._h, n, _ptr(ckpt), _ptr(act), _ptr(mact), C.c_float(dt), substeps, mm_freq, _ptr(gq_out),
                   _ptr(gqd_out), *map(_ptr, grads + scratch))
        return grads

    def backward_multi(self, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, shared=False):
        """dsim_step_backward_multi: K cotangent pairs per environment against one checkpoint, one launch of n_envs * K
        workgroups.  gq_out [K, n_q] / gqd_out [K, n_qd] with shared=True (one set for every environment), [n_envs, K, n_q] /
        [n_envs, K, n_qd] otherwise -> (gq_in [n_envs, K, n_q], gqd_in [n_envs, K, n_qd], gact [n_envs, K, n_qd],
        gmuscle_act [n_envs, K, M] | None); row (e, k) is what backward() returns for environment e and pair k, bit for bit."""
        n, mact = self._actuation(ckpt, act, mact, substeps, mm_freq)
        K, gq_out, gqd_out, grads = self._cotangents(n, gq_out, gqd_out, 1 if shared else n)
        self._call(self._lib.dsim_step_backward_multi, self._h, n, K, 1 if shared else 0, _ptr(ckpt), _ptr(act), _ptr(mact),
                   C.c_float(dt), substeps, mm_freq, _ptr(gq_out), _ptr(gqd_out), *map(_ptr, grads))
        return grads

    def step_jacobian(self, ckpt, act, mact, dt, substeps, mm_freq):
        """dsim_step_jacobian: the Jacobian of the step that wrote `ckpt`, one launch -> (J_state [n_envs, K, K], J_act
        [n_envs, K, n_qd], J_muscle [n_envs, K, M] | None) with K = n_q + n_qd: row k is the gradient of output coordinate k
        of (q_out | qd_out), the columns of J_state are (q_in | qd_in).  The derivative is the adjoint's (include/dsim.h); the
        quaternion blocks of the q_in columns are tangent."""
        n, mact = self._actuation(ckpt, act, mact, substeps, mm_freq)
        K, M = self.n_q + self.n_qd, self.n_muscles
        J = self._new(n, K, K)
        Ja = self._new(n, K, self.n_qd)
        Jm = self._new(n, K, M) if M else None
        self._call(self._lib.dsim_step_jacobian, self._h, n, _ptr(ckpt), _ptr(act), _ptr(mact), C.c_float(dt),
                   substeps, mm_freq, _ptr(J), _ptr(Ja), _ptr(Jm))
        return J, Ja, Jm

    # ---- model parameters of the step ------------------------------------------------------------------
    def step_parameters(self):
        """StepParameters cloned from the template (fresh host-to-device copies: take them once, outside a graph capture)"""
        t = self.template
        dev = lambda a, *shape: torch.as_tensor(a, dtype=torch.float32).reshape(*shape).to(self.device)  # noqa: E731
        return StepParameters(joint_target_ke=dev(t.joint_target_ke, -1), joint_target_kd=dev(t.joint_target_kd, -1),
                              joint_limit_ke=dev(t.joint_limit_ke, -1), joint_limit_kd=dev(t.joint_limit_kd, -1),
                              joint_target=dev(t.joint_target, -1), contact_material=dev(t.contact_material, -1, 4))

    def env_step_parameters(self, n_envs):
        """EnvStepParameters for n_envs environments: the template's values in every row, contiguous tensors of their own (fresh
        host-to-device copies: take them once, outside a graph capture)"""
        p = self.step_parameters()
        return EnvStepParameters(**{k: x.unsqueeze(0).repeat(int(n_envs), *([1] * x.dim())).contiguous()
                                    for k, x in zip(StepParameters.FIELDS, p.tensors())})

    def _param_sizes(self):
        """floats per environment of the six fields, in their order"""
        t = self.template
        return (t.n_links,) * 4 + (t.n_q, 4 * t.n_contacts)

    def env_params(self):
        """dsim_model_env_params: the environments the model holds parameter rows for, 0 while all share one block"""
        return int(self._lib.dsim_model_env_params(self._h))

    def reserve_env_params(self, n_envs):
        """dsim_model_reserve_env_params: a constant block for each of n_envs environments, every row filled with the values all
        environments share at that moment; 0: back to one shared block.  It allocates or frees device memory: not capturable
        (refused during a graph capture).  The Engine remembers the count (its model is its own), so that set_env_params asks
        for a reservation only when the number of environments changes."""
        self._call(self._lib.dsim_model_reserve_env_params, self._h, int(n_envs))
        self._env_rows = int(n_envs)
        self.param_epoch += 1

    def set_env_params(self, p):
        """dsim_model_set_env_params for every field of p (an EnvStepParameters, or its six tensors in that order; an entry may
        be None = left as it is): row e of a tensor becomes environment e's value.  All tensors are checked before the first
        copy and must agree on the number n of environments.  One launch per field on the current stream, capturable, no host
        synchronisation -- EXCEPT the first call with a new n, which reserves the model's per-environment block
        (dsim_model_reserve_env_params: it allocates, fills every row from the values all environments share at that moment,
        and is refused during a graph capture): make that call before capturing.  From then on every launch on this model runs
        environment e under row e, a launch of fewer environments under the first rows, and a launch of more than n is an
        error; set_params still sets a field for ALL environments; reset_params() goes back to one shared block."""
        ts = p.tensors() if isinstance(p, StepParameters) else tuple(p)
        sizes = self._param_sizes()
        if len(ts) != 6:
            raise capi.DsimError("set_env_params takes the six tensors of an EnvStepParameters")
        ns = {x.shape[0] for x in ts if torch.is_tensor(x) and x.dim() >= 2}
        if len(ns) != 1 or any(x is not None and not (torch.is_tensor(x) and x.dim() >= 2) for x in ts):
            raise capi.DsimError("set_env_params: every tensor given needs a leading environment dimension, the same for all "
                                 "(found %s)" % sorted(ns))
        n = ns.pop()
        if n < 1:
            raise capi.DsimError("set_env_params: no environments")
        for x, size, name in zip(ts, sizes, StepParameters.FIELDS):   # (all of them before the first copy: all are set or none)
            if x is not None:
                self._arg(x, n * size, name)
        if getattr(self, "_env_rows", 0) != n:
            self.reserve_env_params(n)
        self.param_epoch += 1
        for field, (x, size) in enumerate(zip(ts, sizes)):
            if x is not None and size:
                self._call(self._lib.dsim_model_set_env_params, self._h, field, n, _ptr(x))

    def set_params(self, p):
        """dsim_model_set_params for every field of p (a StepParameters, or its six tensors in that order; an entry may be None =
        left as it is): device-to-device copies on the current stream, capturable, no host synchronisation.  Every later launch
        on this model ordered after them -- step, fused env step, read-outs -- runs under these values, for ALL environments; the
        model keeps what was last set until reset_params()."""
        ts = p.tensors() if isinstance(p, StepParameters) else tuple(p)
        t = self.template
        sizes = (t.n_links,) * 4 + (t.n_q, 4 * t.n_contacts)
        if len(ts) != 6:
            raise capi.DsimError("set_params takes the six tensors of a StepParameters")
        for x, size, name in zip(ts, sizes, StepParameters.FIELDS):   # (all of them before the first copy: all are set or none)
            if x is not None:
                self._arg(x, size, name)
        self.param_epoch += 1
        for field, (x, size) in enumerate(zip(ts, sizes)):
            if x is not None and size:
                self._call(self._lib.dsim_model_set_params, self._h, field, _ptr(x))

    def reset_params(self):
        """back to the template's values, shared by all environments (a per-environment block is released: not capturable then)"""
        if getattr(self, "_params0", None) is None:
            self._params0 = self.step_parameters()
        if getattr(self, "_env_rows", 0):
            self.reserve_env_params(0)
        self.set_params(self._params0)   # (bumps the parameter epoch)

    def _fold_index(self):
        """(link of every dof [nd], the hinge / slider dofs [k], their coordinates [k]) on the device"""
        if getattr(self, "_fold", None) is None:
            t = self.template
            link, dofs, coords = [], [], []
            for i in range(t.n_links):
                d0, d1 = int(t.joint_qd_start[i]), int(t.joint_qd_start[i + 1])
                link += [i] * (d1 - d0)
                if int(t.joint_type[i]) in (0, 1):   # prismatic, revolute: the dof's coordinate carries the target
                    dofs.append(d0)
                    coords.append(int(t.joint_q_start[i]))
            mk = lambda a: torch.as_tensor(a, dtype=torch.int64).to(self.device)  # noqa: E731
            self._fold = (mk(link), mk(dofs), mk(coords))
        return self._fold

    def fold_param_grads(self, g_dof, g_contact, need=(True,) * 6, per_env=False):
        """what backward_params returns per environment and dof / contact slot -> the gradients of the six StepParameters tensors
        (in their order; None where not needed): summed over the environments, dofs folded into their links (a ball joint's three
        dofs share one gain) and, for joint_target, into the coordinate of their hinge / slider.
        per_env: the environment dimension is kept -- [N, n_links], [N, n_q], [N, C, 4], the gradients of an EnvStepParameters."""
        gp = [None] * 6
        if per_env:
            if any(need[:5]):
                link, dofs, coords = self._fold_index()
                N = g_dof.shape[0]
                for field, row in ((0, 0), (1, 1), (2, 3), (3, 4)):
                    if need[field]:
                        gp[field] = torch.zeros(N, self.template.n_links, device=g_dof.device).index_add_(1, link, g_dof[:, row])
                if need[4]:
                    gp[4] = torch.zeros(N, self.n_q, device=g_dof.device).index_add_(1, coords, g_dof[:, 2][:, dofs])
            if need[5]:
                gp[5] = g_contact
            return gp
        if any(need[:5]):
            link, dofs, coords = self._fold_index()
            d = g_dof.sum(dim=0)   # [5, nd]: target_ke, target_kd, target, limit_ke, limit_kd
            for field, row in ((0, 0), (1, 1), (2, 3), (3, 4)):
                if need[field]:
                    gp[field] = torch.zeros(self.template.n_links, device=d.device).index_add_(0, link, d[row])
            if need[4]:
                gp[4] = torch.zeros(self.n_q, device=d.device).index_add_(0, coords, d[2][dofs])
        if need[5]:
            gp[5] = g_contact.sum(dim=0)
        return gp

    def backward_params(self, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, want_dof=True, want_contact=True):
        """dsim_step_backward_params -> (gq, gqd, gact, gmuscle_act | None, g_dof [n_envs, 5, n_qd] | None, g_contact
        [n_envs, C, 4] | None): the state gradients of backward(), bit for bit, and per environment the gradient terms of every
        dof for (target_ke, target_kd, target, limit_ke, limit_kd) and of every contact slot for (ke, kd, kf, mu), summed over
        the substeps.  The checkpoint is consumed under the parameter values its forward ran with."""
        n, mact = self._actuation(ckpt, act, mact, substeps, mm_freq)
        _, gq_out, gqd_out, grads = self._cotangents(n, gq_out, gqd_out)
        Cn = self.template.n_contacts
        g_dof = self._new(n, 5, self.n_qd) if want_dof else None
        g_con = (self._new(n, Cn, 4) if Cn else torch.zeros(n, 0, 4, device=self.device)) if want_contact else None
        self._call(self._lib.dsim_step_backward_params, self._h, n, _ptr(ckpt), _ptr(act), _ptr(mact), C.c_float(dt),
                   substeps, mm_freq, _ptr(gq_out), _ptr(gqd_out), *map(_ptr, grads + (g_dof, g_con)))
        return grads + (g_dof, g_con)

    # ---- fused environment surface ------------------------------------------------------------------
    def env_forward(self, spec, q, qd, actions, dt, substeps, mm_freq, need_ckpt, episode=None):
        """-> (q_out, qd_out, obs, rew, ckpt[, obs_before_reset, done] when `episode` (an EpisodeIO) is given)"""
        n = self._state(q, (qd, self.n_qd, "qd"), (actions, spec.n_act, "actions"))
        q_out, qd_out = torch.empty_like(q), torch.empty_like(qd)
        obs = self._new(n, spec.n_obs)
        rew = self._new(n)
        ckpt = self._alloc_ckpt(n, substeps, mm_freq) if need_ckpt else None
        ep, extra = None, ()
        if episode is not None:
            ep, extra = episode.bind(self, n, spec.n_obs)
        self._call(self._lib.dsim_env_step_forward, self._h, C.byref(spec), n, _ptr(q), _ptr(qd), _ptr(actions), C.c_float(dt),
                   substeps, mm_freq, _ptr(q_out), _ptr(qd_out), _ptr(obs), _ptr(rew), _ptr(ckpt),
                   C.byref(ep) if ep is not None else None)
        return (q_out, qd_out, obs, rew, ckpt) + extra

    def env_backward(self, spec, ckpt, actions, dt, substeps, mm_freq, gq_out, gqd_out, gobs, grew, gobs_before=None):
        """any cotangent may be None (= zeros: no fill kernels are launched for unused outputs)"""
        n = self._check_ckpt(ckpt, substeps, mm_freq)
        self._arg(actions, n * spec.n_act, "actions")
        for g, width, name in ((gq_out, self.n_q, "gq_out"), (gqd_out, self.n_qd, "gqd_out"), (gobs, spec.n_obs, "gobs"),
                               (grew, 1, "grew"), (gobs_before, spec.n_obs, "gobs_before_reset")):
            if g is not None:
                self._arg(g, n * width, name)
        gq = self._new(n * self.n_q)
        gqd = self._new(n * self.n_qd)
        ga = self._new(n, spec.n_act)
        self._call(self._lib.dsim_env_step_backward, self._h, C.byref(spec), n, _ptr(ckpt), _ptr(actions), C.c_float(dt),
                   substeps, mm_freq, _ptr(gq_out), _ptr(gqd_out), _ptr(gobs), _ptr(grew), _ptr(gobs_before), _ptr(gq), _ptr(gqd),
                   _ptr(ga))
        return gq, gqd, ga

    def env_backward_params(self, spec, ckpt, actions, dt, substeps, mm_freq, gq_out, gqd_out, gobs, grew, gobs_before=None,
                            want_dof=True, want_contact=True):
        """dsim_env_step_backward_params -> (gq, gqd, ga, g_dof [n_envs, 5, n_qd] | None, g_contact [n_envs, C, 4] | None): the
        gradients of env_backward, bit for bit, and per environment the parameter terms backward_params returns, summed over the
        substeps of this step.  Any cotangent may be None (= zeros).  The checkpoint is consumed under the parameter values its
        forward ran with; one launch, plain launch mode."""
        n = self._check_ckpt(ckpt, substeps, mm_freq)
        self._arg(actions, n * spec.n_act, "actions")
        for g, width, name in ((gq_out, self.n_q, "gq_out"), (gqd_out, self.n_qd, "gqd_out"), (gobs, spec.n_obs, "gobs"),
                               (grew, 1, "grew"), (gobs_before, spec.n_obs, "gobs_before_reset")):
            if g is not None:
                self._arg(g, n * width, name)
        Cn = self.template.n_contacts
        gq = self._new(n * self.n_q)
        gqd = self._new(n * self.n_qd)
        ga = self._new(n, spec.n_act)
        g_dof = self._new(n, 5, self.n_qd) if want_dof else None
        g_con = (self._new(n, Cn, 4) if Cn else torch.zeros(n, 0, 4, device=self.device)) if want_contact else None
        for g, numel, name in ((gq, n * self.n_q, "gq_in"), (gqd, n * self.n_qd, "gqd_in"), (ga, n * spec.n_act, "gactions"),
                               (g_dof, n * 5 * self.n_qd, "g_dof"), (g_con, n * Cn * 4, "g_contact")):
            if g is not None:
                self._arg(g, numel, name)
        self._call(self._lib.dsim_env_step_backward_params, self._h, C.byref(spec), n, _ptr(ckpt), _ptr(actions), C.c_float(dt),
                   substeps, mm_freq, _ptr(gq_out), _ptr(gqd_out), _ptr(gobs), _ptr(grew), _ptr(gobs_before), _ptr(gq), _ptr(gqd),
                   _ptr(ga), _ptr(g_dof), _ptr(g_con))
        return gq, gqd, ga, g_dof, g_con

    def env_observe(self, spec, q, qd, stored_actions):
        n = self._state(q, (qd, self.n_qd, "qd"), (stored_actions, spec.n_act, "stored_actions"))
        obs = self._new(n, spec.n_obs)
        rew = self._new(n)
        self._call(self._lib.dsim_env_observe, self._h, C.byref(spec), n, _ptr(q), _ptr(qd), _ptr(stored_actions), _ptr(obs),
                   _ptr(rew))
        return obs, rew


class EpisodeIO:
    """Device buffers of the in-kernel episode bookkeeping (`dsim_episode`, include/dsim.h): progress_buf, the pool of
    start states finished environments restart from, and the termination rules."""

    def __init__(self, progress, reset_q, reset_qd, reset_count, episode_length, height_terminate, check_invalid,
                 want_obs_before, noise_q=None, noise_qd=None, noise_angle=0.0, seed=0):
        self.progress, self.reset_q, self.reset_qd, self.reset_count = progress, reset_q, reset_qd, reset_count
        self.episode_length, self.height_terminate, self.check_invalid = episode_length, height_terminate, check_invalid
        self.want_obs_before = want_obs_before
        # in-kernel stochastic restart: per-coordinate noise amplitudes [n_q] / [n_qd] (device, float32) or None
        self.noise_q, self.noise_qd, self.noise_angle, self.seed = noise_q, noise_qd, float(noise_angle), int(seed)

    def bind(self, engine, n, n_obs):
        engine._arg(self.progress, n, "episode.progress", torch.int64)
        engine._arg(self.reset_count, n, "episode.reset_count", torch.int32)
        k = self.reset_q.shape[0] if torch.is_tensor(self.reset_q) and self.reset_q.dim() else 0   # [pool][n_envs][n_q]
        engine._arg(self.reset_q, k * n * engine.n_q, "episode.reset_q")
        engine._arg(self.reset_qd, k * n * engine.n_qd, "episode.reset_qd")
        for t, cols, name in ((self.noise_q, engine.n_q, "episode.noise_q"), (self.noise_qd, engine.n_qd, "episode.noise_qd")):
            if t is not None:
                engine._arg(t, cols, name)
        done = torch.empty(n, dtype=torch.int64, device=engine.device)
        obs_before = engine._new(n, n_obs) if self.want_obs_before else None
        ep = capi.Episode()
        ep.progress, ep.done = self.progress.data_ptr(), done.data_ptr()
        ep.obs_before_reset = obs_before.data_ptr() if obs_before is not None else None
        ep.reset_q, ep.reset_qd, ep.reset_count = self.reset_q.data_ptr(), self.reset_qd.data_ptr(), self.reset_count.data_ptr()
        ep.reset_pool, ep.episode_length = int(k), int(self.episode_length)
        ep.height_terminate, ep.check_invalid = int(bool(self.height_terminate)), int(bool(self.check_invalid))
        ep.noise_q = self.noise_q.data_ptr() if self.noise_q is not None else None
        ep.noise_qd = self.noise_qd.data_ptr() if self.noise_qd is not None else None
        ep.noise_angle, ep.seed = self.noise_angle, self.seed & 0xFFFFFFFFFFFFFFFF
        return ep, (obs_before, done)


class SimStep(torch.autograd.Function):
    """(joint_q, joint_qd, joint_act, muscle_activation) -> (joint_q', joint_qd') for one env.step().  SimStepParams appends
    the six parameter tensors to the inputs (`params`); the rest of the input handling is the same code."""

    @staticmethod
    def forward(ctx, engine, dt, substeps, mm_freq, q, qd, act, mact, *params):
        q, qd, act = q.contiguous(), qd.contiguous(), act.contiguous()
        mact = mact.contiguous() if mact is not None else None
        need = any(t is not None and t.requires_grad for t in (q, qd, act, mact) + params)
        q_out, qd_out, ckpt = engine.forward(q.detach(), qd.detach(), act.detach(),
                                             mact.detach() if mact is not None else None, dt, substeps, mm_freq, need,
                                             keep_q_in=True)
        ctx.engine, ctx.dt, ctx.substeps, ctx.mm_freq = engine, dt, substeps, mm_freq
        ctx.has_mact = mact is not None
        ctx.shapes = (q.shape, qd.shape, act.shape, mact.shape if mact is not None else None)
        if need:
            ctx.save_for_backward(ckpt, act.detach(), mact.detach() if mact is not None else act.new_empty(0), *params)
        return q_out.view(q.shape), qd_out.view(qd.shape)

    @staticmethod
    def saved(ctx, gq_out, gqd_out):
        """-> (ckpt, act, muscle_act | None, gq_out, gqd_out) of a backward: a missing cotangent is zeros"""
        ckpt, act, mact = ctx.saved_tensors[:3]
        if gq_out is None:
            gq_out = torch.zeros(ctx.shapes[0], dtype=torch.float32, device=ckpt.device)
        if gqd_out is None:
            gqd_out = torch.zeros(ctx.shapes[1], dtype=torch.float32, device=ckpt.device)
        return ckpt, act, mact if ctx.has_mact else None, gq_out, gqd_out

    @staticmethod
    def grads(ctx, gq, gqd, gact, gm, *gparams):
        """the gradients in the order and shapes of forward's inputs"""
        return (None, None, None, None, gq.view(ctx.shapes[0]), gqd.view(ctx.shapes[1]), gact.view(ctx.shapes[2]),
                gm.view(ctx.shapes[3]) if ctx.has_mact else None, *gparams)

    @staticmethod
    def backward(ctx, gq_out, gqd_out):
        from .dflex import config
        ckpt, act, mact, gq_out, gqd_out = SimStep.saved(ctx, gq_out, gqd_out)
        return SimStep.grads(ctx, *ctx.engine.backward(ckpt, act, mact, ctx.dt, ctx.substeps, ctx.mm_freq, gq_out, gqd_out,
                                                       literal=config.literal_quat_grad))


class SimStepParams(torch.autograd.Function):
    """SimStep with the model parameters as inputs: (joint_q, joint_qd, joint_act, muscle_activation, six parameter tensors) ->
    (joint_q', joint_qd').  forward sets the parameters on the model, then steps; backward sets the SAVED tensors again (another
    forward with other values may have run in between: the checkpoint is consumed under the values it was written with),
    launches dsim_step_backward_params, folds dofs into links (joint_target: into coordinates) and sums over the environments.
    All of it on the current stream, so a captured rollout whose leaves are parameter tensors sees in-place updates at the next
    replay.  The model keeps what was set last -- after a backward, the values of that backward's forward."""

    @staticmethod
    def forward(ctx, engine, dt, substeps, mm_freq, q, qd, act, mact, *params):
        params = tuple(p.contiguous() for p in params)
        engine.set_params(params)
        return SimStep.forward(ctx, engine, dt, substeps, mm_freq, q, qd, act, mact, *params)

    @staticmethod
    def backward(ctx, gq_out, gqd_out):
        ckpt, act, mact, gq_out, gqd_out = SimStep.saved(ctx, gq_out, gqd_out)
        params = ctx.saved_tensors[3:]
        e = ctx.engine
        need = ctx.needs_input_grad[8:]
        e.set_params(params)
        gq, gqd, gact, gm, g_dof, g_con = e.backward_params(ckpt, act, mact, ctx.dt, ctx.substeps, ctx.mm_freq, gq_out, gqd_out,
                                                            want_dof=any(need[:5]) or not need[5], want_contact=need[5])
        gp = [g.view(p.shape) if g is not None else None for g, p in zip(e.fold_param_grads(g_dof, g_con, need), params)]
        return SimStep.grads(ctx, gq, gqd, gact, gm, *gp)


class SimStepEnvParams(torch.autograd.Function):
    """SimStepParams with a value per environment: the six tensors of an EnvStepParameters as inputs.  forward sets them on the
    model (Engine.set_env_params), then steps; backward sets the SAVED tensors again, launches dsim_step_backward_params and folds
    dofs into links (joint_target: into coordinates) WITHOUT summing over the environments: every row receives the gradient of
    its own environment's outputs, in the tensor's own shape -- N parameter hypotheses differentiated by one launch."""

    @staticmethod
    def forward(ctx, engine, dt, substeps, mm_freq, q, qd, act, mact, *params):
        params = tuple(p.contiguous() for p in params)
        engine.set_env_params(params)
        return SimStep.forward(ctx, engine, dt, substeps, mm_freq, q, qd, act, mact, *params)

    @staticmethod
    def backward(ctx, gq_out, gqd_out):
        ckpt, act, mact, gq_out, gqd_out = SimStep.saved(ctx, gq_out, gqd_out)
        params = ctx.saved_tensors[3:]
        e = ctx.engine
        need = ctx.needs_input_grad[8:]
        e.set_env_params(params)
        gq, gqd, gact, gm, g_dof, g_con = e.backward_params(ckpt, act, mact, ctx.dt, ctx.substeps, ctx.mm_freq, gq_out, gqd_out,
                                                            want_dof=any(need[:5]) or not need[5], want_contact=need[5])
        gp = [g.view(p.shape) if g is not None else None
              for g, p in zip(e.fold_param_grads(g_dof, g_con, need, per_env=True), params)]
        return SimStep.grads(ctx, gq, gqd, gact, gm, *gp)


class EnvStep(torch.autograd.Function):
    """Fused env.step(): (joint_q, joint_qd, actions) -> (joint_q', joint_qd', obs, rew); ONE launch each way.
    With an EpisodeIO the launch also does the episode bookkeeping and the outputs gain (obs_before_reset, done)."""

    @staticmethod
    def forward(ctx, engine, spec, episode, dt, substeps, mm_freq, q, qd, actions):
        q, qd, actions = q.contiguous(), qd.contiguous(), actions.contiguous()
        need = q.requires_grad or qd.requires_grad or actions.requires_grad
        out = engine.env_forward(spec, q.detach(), qd.detach(), actions.detach(), dt, substeps, mm_freq, need, episode)
        q_out, qd_out, obs, rew, ckpt = out[:5]
        ctx.engine, ctx.spec, ctx.dt, ctx.substeps, ctx.mm_freq = engine, spec, dt, substeps, mm_freq
        ctx.shapes = (q.shape, qd.shape, actions.shape)
        ctx.set_materialize_grads(False)
        if need:
            ctx.save_for_backward(ckpt, actions.detach())
        res = (q_out.view(q.shape), qd_out.view(qd.shape), obs, rew)
        if episode is not None:
            obs_before, done = out[5], out[6]
            ctx.mark_non_differentiable(done)
            res = res + ((obs_before if obs_before is not None else obs.new_empty(0)), done)
        return res

    @staticmethod
    def backward(ctx, gq_out, gqd_out, gobs, grew, gobs_before=None, gdone=None):
        ckpt, actions = ctx.saved_tensors
        c = lambda g: g.contiguous() if g is not None else None  # noqa: E731
        if gobs_before is not None and gobs_before.numel() == 0:
            gobs_before = None
        gq, gqd, ga = ctx.engine.env_backward(ctx.spec, ckpt, actions, ctx.dt, ctx.substeps, ctx.mm_freq, c(gq_out),
                                              c(gqd_out), c(gobs), c(grew), c(gobs_before))
        return None, None, None, None, None, None, gq.view(ctx.shapes[0]), gqd.view(ctx.shapes[1]), ga.view(ctx.shapes[2])


class EnvStepParams(torch.autograd.Function):
    """EnvStep with the six tensors of a StepParameters (per_env False) or an EnvStepParameters (per_env True) as inputs:
    (joint_q, joint_qd, actions, six parameter tensors) -> EnvStep's outputs, and a gradient for every parameter tensor that
    requires one.  forward does NOT set the values on the model (that would be six copies per step of a rollout): the caller has
    set them (DFlexEnv.set_step_parameters) and forward records the Engine's parameter epoch.  backward raises DsimError if the
    epoch moved -- the checkpoint would be consumed under other values than its forward ran with --, launches
    dsim_env_step_backward_params with only the outputs needed and folds them (Engine.fold_param_grads): summed over the
    environments for shared parameters, row e for environment e otherwise.  Autograd sums the steps of a rollout."""

    @staticmethod
    def forward(ctx, engine, spec, episode, dt, substeps, mm_freq, per_env, q, qd, actions, *params):
        if len(params) != 6:
            raise capi.DsimError("EnvStepParams takes the six tensors of a StepParameters / EnvStepParameters")
        ctx.epoch, ctx.per_env = engine.param_epoch, bool(per_env)
        ctx.param_shapes = tuple(p.shape for p in params)
        q, qd, actions = q.contiguous(), qd.contiguous(), actions.contiguous()
        out = engine.env_forward(spec, q.detach(), qd.detach(), actions.detach(), dt, substeps, mm_freq, True, episode)
        q_out, qd_out, obs, rew, ckpt = out[:5]
        ctx.engine, ctx.spec, ctx.dt, ctx.substeps, ctx.mm_freq = engine, spec, dt, substeps, mm_freq
        ctx.shapes = (q.shape, qd.shape, actions.shape)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ckpt, actions.detach())
        res = (q_out.view(q.shape), qd_out.view(qd.shape), obs, rew)
        if episode is not None:
            obs_before, done = out[5], out[6]
            ctx.mark_non_differentiable(done)
            res = res + ((obs_before if obs_before is not None else obs.new_empty(0)), done)
        return res

    @staticmethod
    def backward(ctx, gq_out, gqd_out, gobs, grew, gobs_before=None, gdone=None):
        e = ctx.engine
        if e.param_epoch != ctx.epoch:
            raise capi.DsimError("the model's parameters were set again between this env.step() and its backward (parameter epoch "
                                 "%d -> %d): the checkpoint would be consumed under other values than its forward ran with"
                                 % (ctx.epoch, e.param_epoch))
        ckpt, actions = ctx.saved_tensors
        c = lambda g: g.contiguous() if g is not None else None  # noqa: E731
        if gobs_before is not None and gobs_before.numel() == 0:
            gobs_before = None
        need = ctx.needs_input_grad[10:]
        gq, gqd, ga, g_dof, g_con = e.env_backward_params(ctx.spec, ckpt, actions, ctx.dt, ctx.substeps, ctx.mm_freq, c(gq_out),
                                                          c(gqd_out), c(gobs), c(grew), c(gobs_before), want_dof=any(need[:5]),
                                                          want_contact=need[5])
        gp = [g.view(s) if g is not None else None
              for g, s in zip(e.fold_param_grads(g_dof, g_con, need, per_env=ctx.per_env), ctx.param_shapes)]
        return (None,) * 7 + (gq.view(ctx.shapes[0]), gqd.view(ctx.shapes[1]), ga.view(ctx.shapes[2]), *gp)


class ReadoutFunction(torch.autograd.Function):
    """(a row r of READOUTS, its inputs) -> the outputs that are computed: a read-out of the state handed in with its adjoint
    (r.forward / r.backward, e.g. dsim_joint_dynamics / dsim_joint_dynamics_backward); the backward launch re-runs the forward
    pass on the saved inputs.  The quaternion blocks of the returned joint_q gradient have no component along the quaternion,
    as SimStep's."""

    @staticmethod
    def forward(ctx, engine, r, *inputs):
        # (an input the model has no room for -- muscle_act without muscles -- is absent from here on: no gradient either)
        width = engine._sizes()
        det = [t.detach().contiguous() if t is not None and width(w) else None for t, (_, w, _) in zip(inputs, r.inputs)]
        outs = engine.readout_forward(r, *det)
        ctx.engine, ctx.r = engine, r
        ctx.shapes = [t.shape if d is not None else None for t, d in zip(inputs, det)]
        ctx.set_materialize_grads(False)   # an output the loss does not read costs no cotangent buffer
        ctx.save_for_backward(*[d if d is not None else det[0].new_empty(0) for d in det])
        return tuple(o for o in outs if o is not None)

    @staticmethod
    def backward(ctx, *cots):
        if all(g is None for g in cots):
            return (None,) * (2 + len(ctx.shapes))
        inputs = [t if s is not None else None for t, s in zip(ctx.saved_tensors, ctx.shapes)]
        # (an output that was not computed has no cotangent; neither has one without elements: contacts of a model without any)
        cots = [g.contiguous() if g is not None and g.numel() else None for g in cots] + [None] * (len(ctx.r.outputs) - len(cots))
        # Through the public <name>_backward, not readout_backward(r, ...): that method is the seam a caller observes the adjoint
        # launch at -- the GPU tests of the four read-outs wrap it on the instance to see which cotangents autograd hands over --
        # as it was with the four autograd classes.  (mass_matrix_backward returns its one gradient bare.)
        grads = getattr(ctx.engine, ctx.r.name + "_backward")(*inputs, *cots)
        grads = grads if isinstance(grads, tuple) else (grads,)
        return (None, None) + tuple(g.view(s) if s is not None else None for g, s in zip(grads, ctx.shapes))
