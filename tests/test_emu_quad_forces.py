"""CPU tier: the Ant step pair of the host harness (tests/emu: the lane-serial build of the kernel phase code, which has no
register blocks and therefore reloads the body-level constants of the quad kinematics in every substep -- the path the
two-environment kernels and every read-out keep) on the cases of tests/test_gpu_quad_forces.py: N = 1 and 3 recorded start states
(feet in contact, so the per-body contact sums are not zero) with two hinges pushed past their limits, S = 4, mass-matrix refresh
every 1, 2 and 4 substeps, specialised layout with full and lean checkpoints.

 * against the scalar oracle: state 1e-4, gradients 1e-3 (tests/test_gpu_joint_regs.py);
 * against tests/golden/quad_forces_emu_parent.npz, what the parent commit's libdsim_emu.so gave on the same cases: bit for bit on
   every output and on every word of the checkpoint that the forward launch defines (f_tot, qdd and the rest of the saved block,
   every group's inverse).  Keeping the constants in registers only moves loads; nothing may change a bit.

python tests/test_emu_quad_forces.py --record [out.npz] writes that file from the harness DSIM_EMU_LIB names (run at the parent)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (run as a script: the package's directory)

from oracle_lib import golden, oracle_backward, project_tangent, relerr, template_from_golden  # noqa: E402

NS = [1, 3]
S4 = 4
FIRST = 7
MMS = [1, 2, 4]
KEYS = ("q", "qd", "gq", "gqd", "gact")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_forces_emu_parent.npz")
_oracle = {}
_parent = {}


def case(t, n):
    """n start states of the recorded step whose feet touch the ground (its environments 7, 8, 9: the first five are airborne,
    test_contact_sums_are_not_zero), one hinge below its lower limit and one above its upper limit in each"""
    g = golden("ant_step")
    sl = slice(FIRST, FIRST + n)
    q = g["q_in"][sl].copy()
    jt, qs = np.asarray(t.joint_type), np.asarray(t.joint_q_start)
    hinges = [int(qs[i]) for i in range(t.n_links) if int(jt[i]) in (0, 1)]
    lo, hi = np.asarray(t.joint_limit_lower, np.float32), np.asarray(t.joint_limit_upper, np.float32)
    for e in range(n):
        a, b = hinges[(2 * e) % len(hinges)], hinges[(2 * e + 3) % len(hinges)]
        q[e, a] = lo[a] - np.float32(0.2)
        q[e, b] = hi[b] + np.float32(0.2)
    return dict(q=q, qd=g["qd_in"][sl], act=g["act_in"][sl], gq=g["gq_out"][sl], gqd=g["gqd_out"][sl], dt=float(g["dt"]))


def ckpt_words(t, ck, S, mm):
    """the words of a full checkpoint that the forward launch defines (tests/test_gpu_joint_regs.py: _ckpt_words)"""
    from emu_lib import layout
    off, _ = layout(t)
    nd, nq = t.n_qd, t.n_q
    L, row = t.n_links, off["qdd"] + nd - off["q"]
    stride, hw, groups = (row + 3) & ~3, (nd * nd + 3) & ~3, (S + mm - 1) // mm
    assert ck.shape[1] >= S * stride + groups * hw
    fields = [("q", 0, nq), ("qd", 0, nd), ("xsc", 0, 7 * L), ("S", 36, 6 * nd), ("v", 0, 6 * L), ("a", 0, 6 * L), ("i10", 0, 10 * L),
              ("ftot", 0, 6 * L), ("qdd", 0, nd)]
    parts = [ck[:, s * stride + off[f] - off["q"] + lo:s * stride + off[f] - off["q"] + hi] for s in range(S) for f, lo, hi in fields]
    parts += [ck[:, S * stride + g * hw:S * stride + g * hw + nd * nd] for g in range(groups)]
    return np.concatenate(parts, axis=1)


def _emu_run(t, c, S, mm, lean):
    import emu_lib
    qo, qdo, ck = emu_lib.step_forward(t, c["q"], c["qd"], c["act"], None, c["dt"], S, mm, static=True, lean=lean)
    r = emu_lib.step_backward(t, ck, c["act"], None, c["dt"], S, mm, c["gq"], c["gqd"], static=True, lean=lean)
    out = dict(q=qo, qd=qdo, gq=r["gq"], gqd=r["gqd"], gact=r["gact"])
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    if not lean:
        out["ckpt"] = ckpt_words(t, ck, S, mm)
        assert np.isfinite(out["ckpt"]).all()
    return out


def _tag(n, mm, lean):
    return "n%d_mm%d_%s" % (n, mm, "lean" if lean else "full")


@pytest.fixture(scope="module")
def t():
    return template_from_golden("ant")


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("mm", MMS)
@pytest.mark.parametrize("n", NS)
def test_harness_vs_oracle_and_parent_bits(t, n, mm, lean):
    c = case(t, n)
    r = _emu_run(t, c, S4, mm, lean)
    key = (n, mm)
    if key not in _oracle:
        _oracle[key] = oracle_backward(t, c["q"], c["qd"], c["act"], None, c["dt"], S4, mm, c["gq"], c["gqd"])
    o = _oracle[key]
    e = dict(q=relerr(r["q"], o["q_out"]), qd=relerr(r["qd"], o["qd_out"]),
             gq=relerr(project_tangent(t, c["q"], r["gq"]), project_tangent(t, c["q"], o["gq"])),
             gqd=relerr(r["gqd"], o["gqd"]), gact=relerr(r["gact"], o["gact"]))
    print("%s oracle: " % _tag(n, mm, lean) + "  ".join("%s %.2e" % kv for kv in e.items()))
    assert e["q"] < 1e-4 and e["qd"] < 1e-4, e
    assert e["gq"] < 1e-3 and e["gqd"] < 1e-3 and e["gact"] < 1e-3, e
    if not _parent:
        _parent.update(np.load(GOLDEN))
    for k in r:
        assert np.array_equal(r[k], _parent["%s_%s" % (_tag(n, mm, lean), k)]), k


def test_contact_sums_are_not_zero(t):
    """the cases must exercise the contact wrenches (an all-airborne state would hide a wrong contact sum): the contact wrench rows of
    a substep from every start state are not all zero"""
    c = case(t, 3)
    import emu_lib
    for e in range(3):
        img, off, dims = emu_lib.substep_image(t, c["q"][e], c["qd"][e], c["act"][e], None, c["dt"] / 16)
        cw = img[off["cw"]:off["cw"] + 6 * t.n_contacts]
        assert np.abs(cw).max() > 0, e


if __name__ == "__main__":
    assert len(sys.argv) >= 2 and sys.argv[1] == "--record"
    tt = template_from_golden("ant")
    rec = {}
    for n_ in NS:
        for mm_ in MMS:
            for lean_ in (False, True):
                for k_, v_ in _emu_run(tt, case(tt, n_), S4, mm_, lean_).items():
                    rec["%s_%s" % (_tag(n_, mm_, lean_), k_)] = v_
    out_path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez_compressed(out_path, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out_path, len(rec), os.path.getsize(out_path)))
