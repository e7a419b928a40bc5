"""Test infrastructure of the differentiable mass matrix read-out (dsim_mass_matrix / dsim_mass_matrix_backward):

* the entry points of the lane-serial host harness for this phase code (tests/emu/dsim_emu_mass.cpp; tests/emu_lib.py loads the
  harness), for the shipped layouts and for the two user models of tests/golden/user_*.npz;
* a float32 numpy restatement of the pivot-free Gauss-Jordan elimination (classical form, written from the formulas alone): the
  yardstick of the residual |Hinv H - I| that an fp32 inverse of THIS matrix can be expected to reach;
* the bounds and the link / dof incidence mask the two test tiers share.
"""
import ctypes as C

import numpy as np

from diffrl_amd.capi import make_desc
from emu_lib import ENVS, ROOT  # noqa: F401
from emu_lib import emu, emu_user, f32, mode, ptr

SETS = ("H", "Hinv", "S", "all")
FWD_BOUND = 1e-5      # S and H in the tensor's max-norm: the bound of the first-substep S_s and I_s (tests/ckpt_fields.py)
SYM_BOUND = 1e-6      # max |H - H^T| / max |H|
RADIAL = 1e-6
RESIDUAL_FACTOR, RESIDUAL_FLOOR = 10.0, 1e-6
FD_STEP, FD_BOUND = 1e-2, 1e-3


def emu_mass_forward(t, q, static=False, waves=1, user=False, want=(True, True, True)):
    """-> (H [N, nd, nd], Hinv [N, nd, nd], S [N, nd, 6]); an output not wanted is passed as NULL and returned as None.  The
    buffers start as NaN: what comes back was written."""
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q = f32(q)
    N, nd = q.shape[0], t.n_qd
    outs = [np.full((N, nd, nd), np.nan, np.float32) if want[0] else None, np.full((N, nd, nd), np.nan, np.float32) if want[1] else None,
            np.full((N, nd, 6), np.nan, np.float32) if want[2] else None]
    with mode(lib, static, waves):
        rc = lib.dsim_emu_mass_matrix(C.byref(desc), C.c_int(N), ptr(q), *[ptr(o) for o in outs])
    assert rc == 0, rc
    return tuple(outs)


def emu_mass_backward(t, q, gH, gHinv, gS, static=False, waves=1, user=False):
    lib = emu_user() if user else emu()
    desc, keep = make_desc(t)
    q, gH, gHinv, gS = f32(q), f32(gH), f32(gHinv), f32(gS)
    gq = np.full((q.shape[0], t.n_q), np.nan, np.float32)
    with mode(lib, static, waves):
        rc = lib.dsim_emu_mass_matrix_backward(C.byref(desc), C.c_int(q.shape[0]), ptr(q), ptr(gH), ptr(gHinv), ptr(gS), ptr(gq))
    assert rc == 0, rc
    return gq


# ---- the yardstick of the inverse ---------------------------------------------------------------------------------------
def gauss_jordan_f32(H):
    """In-place Gauss-Jordan inverse without pivoting, every operation rounded to float32.  Per pivot k: the pivot row is divided by
    the pivot (its own column holding 1 / pivot), and every other row i loses its multiple H[i][k] of the new pivot row (its column
    k holding -H[i][k] / pivot)."""
    A = np.array(H, np.float32)
    n = A.shape[0]
    for k in range(n):
        piv = A[k, k]
        A[k, k] = np.float32(1.0)
        A[k] = A[k] / piv
        for i in range(n):
            if i != k:
                m = A[i, k]
                A[i, k] = np.float32(0.0)
                A[i] = A[i] - m * A[k]
    return A


def residual(Hinv, H):
    """max |Hinv H - I| per batch, a float64 product of two fp32 tensors"""
    P = np.asarray(Hinv, np.float64) @ np.asarray(H, np.float64)
    return float(np.abs(P - np.eye(P.shape[-1])).max())


def residual_bound(H_ref):
    """(bound, yardstick): 10 x the residual of the float32 restatement on the reference's matrices, floor 1e-6.  The factor covers
    the hardware reciprocal and the kernel's own rounding of H."""
    y = max(residual(gauss_jordan_f32(h), h) for h in np.asarray(H_ref, np.float32))
    return max(RESIDUAL_FACTOR * y, RESIDUAL_FLOOR), y


# ---- fixtures and bounds -------------------------------------------------------------------------------------------------
def reference_H(t, step):
    """sub_H of the step fixture (the reference's model.H) + diag(joint_armature): what the kernels invert"""
    nd = t.n_qd
    H = np.asarray(step["sub_H"], np.float64).reshape(-1, nd, nd)
    return H + np.diag(np.asarray(t.joint_armature, np.float64))


def reference_S(t, step):
    return np.asarray(step["sub_S_s"], np.float64).reshape(-1, t.n_qd, 6)


def cotangents(m, tag, rows=slice(None)):
    B = m["c_H"].shape[0]
    cS = m["c_S"].reshape(B, -1, 6)
    return tuple(c[rows] if tag in (k, "all") else None for c, k in ((m["c_H"], "H"), (m["c_Hinv"], "Hinv"), (cS, "S")))


def grad_bound(noise_rows):
    """10 x the set's recorded +-1 ulp noise of the reference, floor 1e-4, ceiling 1e-3"""
    return float(np.clip(10.0 * np.max(noise_rows), 1e-4, 1e-3))


def link_dof_mask(t):
    """[L, nd] bool: dof d belongs to link i or one of its ancestors"""
    L, nd = t.n_links, t.n_qd
    start = [int(s) for s in t.joint_qd_start]   # L + 1 entries
    m = np.zeros((L, nd), bool)
    for i in range(L):
        p = int(t.joint_parent[i])
        if p >= 0:
            m[i] = m[p]
        m[i, start[i]:start[i + 1]] = True
    return m


def dot_bound(Hinv, tau):
    """elementwise worst case of an fp32 dot product of nd terms in any order, + the rounding of the result's storage"""
    nd = Hinv.shape[-1]
    return (nd + 2) * 2.0 ** -24 * np.einsum("bij,bj->bi", np.abs(np.asarray(Hinv, np.float64)), np.abs(np.asarray(tau, np.float64)))
