"""Test infrastructure of the model-parameter gradients of the step (dsim_model_set_params / dsim_step_backward_params):

* the step of the lane-serial host harness with a parameter block and with the parameter gradients (dsim_emu_step_forward /
  dsim_emu_step_backward of tests/emu/dsim_emu.cpp through emu_lib.step_forward / step_backward; tests/emu_lib.py loads the harness);
* the folds from what the kernels return -- per dof [N][5][nd], per contact slot [N][C][4] -- to what the reference records per
  environment: per link, per coordinate (target) and per SHAPE (contact_material of <env>_model.npz is the shape of each slot);
* the bounds the two test tiers share.
"""
import numpy as np

from emu_lib import ENVS, ROOT  # noqa: F401
from emu_lib import PARAM_FIELDS as FIELDS
from emu_lib import step_backward, step_forward
from oracle_lib import golden, template_from_golden

DOF_ROWS = ("target_ke", "target_kd", "target", "limit_ke", "limit_kd")                     # rows of g_dof
PARAM_TENSORS = ("g_target_ke", "g_target_kd", "g_target", "g_limit_ke", "g_limit_kd", "g_shape_materials")
# forward outputs and state gradients: the bounds of the step tests (tests/test_emu_phases.py, tests/test_gpu_parity.py)
STATE_BOUND, GRAD_BOUND = 1e-4, 1e-3
HINGE = (0, 1)


def emu_par_forward(t, q, qd, act, mact, dt, substeps, mm_freq, params=None, static=False, waves=1, lean=False):
    """-> (q_out, qd_out, ckpt); buffers start as NaN"""
    return step_forward(t, q, qd, act, mact, dt, substeps, mm_freq, params=params, static=static, waves=waves, lean=lean)


def emu_par_backward(t, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, params=None, static=False, waves=1, lean=False,
                     want=(True, True), want_act=True):
    """want = (g_dof, g_contact); both False: the plain step adjoint.  -> dict(gq, gqd, gact, gmact, g_dof, g_contact); an output
    not wanted is passed as NULL and returned as None; the buffers start as NaN: what comes back was written."""
    return step_backward(t, ckpt, act, mact, dt, substeps, mm_freq, gq_out, gqd_out, params=params, static=static, waves=waves,
                         lean=lean, want=want, want_act=want_act)


# ---- folds -------------------------------------------------------------------------------------------------------------
def dof_maps(t):
    """(link of every dof [nd], coordinate of every hinge / slider dof or -1 [nd])"""
    link, coord = np.zeros(t.n_qd, np.int64), np.full(t.n_qd, -1, np.int64)
    for i in range(t.n_links):
        d0, d1 = int(t.joint_qd_start[i]), int(t.joint_qd_start[i + 1])
        link[d0:d1] = i
        if int(t.joint_type[i]) in HINGE:
            coord[d0] = int(t.joint_q_start[i])
    return link, coord


def fold(t, name, g_dof, g_contact):
    """per environment, in the reference's shapes: g_target_ke / kd, g_limit_ke / kd [N, L], g_target [N, n_q],
    g_shape_materials [N, shapes, 4] (None without contacts); float64 sums"""
    link, coord = dof_maps(t)
    out = {}
    if g_dof is not None:
        g = np.asarray(g_dof, np.float64)
        N = g.shape[0]
        for r, k in enumerate(DOF_ROWS):
            if k == "target":
                a = np.zeros((N, t.n_q))
                np.add.at(a, (slice(None), coord[coord >= 0]), g[:, r, coord >= 0])
            else:
                a = np.zeros((N, t.n_links))
                np.add.at(a, (slice(None), link), g[:, r, :])
            out["g_" + k] = a
    if g_contact is not None and t.n_contacts:
        m = golden(name + "_model")
        shape = np.asarray(m["contact_material"], np.int64)
        gc = np.asarray(g_contact, np.float64)
        a = np.zeros((gc.shape[0], m["shape_materials"].shape[0], 4))
        np.add.at(a, (slice(None), shape), gc)
        out["g_shape_materials"] = a
    return out


def param_bound(noise):
    """10 x the tensor's recorded +-1 ulp noise of the reference, floor 1e-4, ceiling 1e-3 (no recorded tensor's 10 x noise is above
    the ceiling: the largest is SNUHumanoid's shape_materials, 8.1e-4)"""
    return float(np.clip(10.0 * float(noise), 1e-4, 1e-3))


def case(name):
    """(template, fixture, actuation as (act, mact))"""
    t, g = template_from_golden(name), golden(name + "_par")
    N = g["q_in"].shape[0]
    if t.n_muscles > 0:
        return t, g, (np.zeros((N, t.n_qd), np.float32), g["muscle_act_in"])
    return t, g, (g["act_in"], None)


def perturbed_params(t, seed=5):
    """every field scaled by seeded factors in [0.8, 1.25] (targets moved by +-0.1), as float32"""
    rs = np.random.RandomState(seed)
    s = lambda a: (np.asarray(a, np.float32) * rs.uniform(0.8, 1.25, np.shape(a))).astype(np.float32)  # noqa: E731
    return dict(target_ke=s(t.joint_target_ke), target_kd=s(t.joint_target_kd), limit_ke=s(t.joint_limit_ke), limit_kd=s(t.joint_limit_kd),
                target=(t.joint_target + rs.uniform(-0.1, 0.1, t.n_q)).astype(np.float32), contact_material=s(t.contact_material))


def with_params(t, p):
    """a template with these values in place of its own"""
    import copy
    t2 = copy.deepcopy(t)
    for k, attr in (("target_ke", "joint_target_ke"), ("target_kd", "joint_target_kd"), ("limit_ke", "joint_limit_ke"),
                    ("limit_kd", "joint_limit_kd"), ("target", "joint_target"), ("contact_material", "contact_material")):
        setattr(t2, attr, np.ascontiguousarray(p[k], np.float32))
    return t2
