"""CPU: the differentiable ground-contact read-out (dsim_core.hpp: dsim_ground_contact_forward / dsim_ground_contact_backward)
on the lane-serial host build of the phase code (tests/emu/dsim_emu_con.cpp, compiled by tests/con_lib.py), generic and
specialised layouts, one and four wavefronts per environment.

References: tests/golden/<env>_con.npz (tools/gen_contact_golden.py): `force` and `link_wrench` and their gradients are the
reference simulator's own eval_rigid_contacts_art on its own frames and twists; `point` and `vel`, which the reference has no
tensor of, are the float64 statement of tests/con_lib.py on the reference's recorded frames, their gradients that statement's
adjoint chained with kin_lib.fk_adjoint.  The statement itself is held to the reference's tensors here, and its adjoint to
central differences of its forward.

Bounds (the project's, tests/test_joint_dynamics_cpu.py): forward 1e-4 in each tensor's max-norm, or 10 x the reference's recorded
+-1 ulp noise of the tensor where that is larger; adjoint, every cotangent set in its own max-norm, 10 x the reference's recorded
+-1 ulp noise of that set and tensor, floor 1e-5, ceiling 1e-3; joint_q gradients after project_tangent, own radial part
<= 1e-6 of max |gq|.  A contact the fixture marks `edge` (|point.y| < 1e-4: fp32 rounding may flip its active set; at most 1 % of
a model's contacts, in at most one state) is left out of the force comparison, its state out of the link_wrench and gradient
rows.  The user models have no recording: their reference is the float64 statement, their noise that statement's own deviation
under the same +-1 ulp moves of the fp32 inputs."""
import itertools
import os
import re

import numpy as np
import pytest

import con_lib as K
import kin_lib
from diffrl_amd import capi
from diffrl_amd.template import ArticulationTemplate
from oracle_lib import golden, project_tangent, relerr, template_from_golden

VARIANTS = [(False, 1, "generic-1w"), (False, 4, "generic-4w"), (True, 1, "specialised-1w"), (True, 4, "specialised-4w")]
SETS = ("point", "vel", "force", "lw", "all")
FWD = (("point", "point"), ("vel", "vel"), ("force", "force"), ("lw", "link_wrench"))
RADIAL = 1e-6
_cache = {}


def _case(name):
    if name not in _cache:
        _cache[name] = (template_from_golden(name), golden(name + "_con"))
    return _cache[name]


def cotangents(g, tag):
    return tuple(g["c_" + k] if tag in (k, "all") else None for k in ("point", "vel", "force", "lw"))


def fwd_bound(g, key, prefix="noise_"):
    return max(1e-4, 10.0 * float(g[prefix + key].max()))


def grad_bound(noise_rows):
    return float(np.clip(10.0 * noise_rows.max(), 1e-5, 1e-3))


def kept_states(edge):
    """states without an edge contact; the fixture holds at most one with one"""
    keep = ~edge.any(axis=1)
    assert (~keep).sum() <= 1 and edge.sum() <= 0.01 * edge.size
    return keep


def rows_err(a, b, rows):
    a, b = np.asarray(a, np.float64)[rows], np.asarray(b, np.float64)[rows]
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def check_forward(g, out, edge, what, prefix=""):
    keep = kept_states(edge)
    names = dict(point=prefix + "point", vel=prefix + "vel", force=prefix + "force", lw=prefix + ("lw" if prefix else "link_wrench"))
    nz = "comp_noise_" if prefix else "noise_"
    for (k, nk), a in zip(FWD, out):
        ref = g[names[k]]
        if k == "force":
            e = float(np.abs(np.asarray(a, np.float64) - ref)[~edge].max() / np.abs(ref).max())
        elif k == "lw":
            e = rows_err(a, ref, keep)
        else:
            e = relerr(a, ref)
        bound = fwd_bound(g, k if prefix else nk, nz)
        print("%s forward %-5s err %.2e bound %.1e" % (what, k, e, bound))
        assert e < bound, (k, e, bound)
    # exactly zero where the point does not penetrate
    assert not out[2][out[0][:, :, 1] >= 0].any()


@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", K.ENVS)
def test_forward_matches_the_fixture(name, static, waves, label):
    t, g = _case(name)
    out = K.emu_con_forward(t, g["q_in"], g["qd_in"], static, waves)
    assert all(np.isfinite(o).all() for o in out)   # every word written (the buffers start as NaN)
    check_forward(g, out, g["edge"].astype(bool), "%s %s" % (name, label))
    # link_wrench is the gather in contact order of (point x force, force)
    lw = K.gather_link_wrench(t, out[0], out[2])
    assert np.abs(lw - out[3]).max() <= 1e-6 * np.abs(out[3]).max()


@pytest.mark.parametrize("static,waves,label", VARIANTS)
@pytest.mark.parametrize("name", K.ENVS)
def test_adjoint_matches_the_reference(name, static, waves, label):
    t, g = _case(name)
    q, qd = g["q_in"], g["qd_in"]
    keep = kept_states(g["edge"].astype(bool))
    for tag in SETS:
        gq, gqd = K.emu_con_backward(t, q, qd, *cotangents(g, tag), static=static, waves=waves)
        assert np.isfinite(gq).all() and np.isfinite(gqd).all()
        rows = keep if tag in ("force", "lw", "all") else np.ones_like(keep)
        for k, got, ref in (("gq", project_tangent(t, q, gq), project_tangent(t, q, g["gq_" + tag])), ("gqd", gqd, g["gqd_" + tag])):
            noise = g["noise_%s_%s" % (k, tag)][rows]
            e, bound = rows_err(got, ref, rows), grad_bound(noise)
            print("%s %s cotangent %-5s %-3s err %.2e  reference noise %.2e  bound %.1e" % (name, label, tag, k, e, noise.max(), bound))
            assert e < bound, (tag, k, e, bound)
        rad = kin_lib.radial_part(t, q, gq)
        assert rad <= RADIAL, (tag, rad)


@pytest.mark.parametrize("name", K.ENVS)
def test_every_null_pattern(name):
    """an output that is not asked for changes no other output; a NULL cotangent is a zero cotangent -- bit for bit"""
    t, g = _case(name)
    q, qd = g["q_in"][:3], g["qd_in"][:3]
    waves = kin_lib.waves_of(t)
    for static in (False, True):
        full = K.emu_con_forward(t, q, qd, static, waves)
        for want in itertools.product((False, True), repeat=4):
            if not any(want):
                continue
            out = K.emu_con_forward(t, q, qd, static, waves, want=want)
            for w, a, b in zip(want, out, full):
                assert (a is None) if not w else np.array_equal(a, b), want
        cs = [g["c_" + k][:3] for k in ("point", "vel", "force", "lw")]
        for have in itertools.product((False, True), repeat=4):
            a = K.emu_con_backward(t, q, qd, *[c if h else None for c, h in zip(cs, have)], static=static, waves=waves)
            b = K.emu_con_backward(t, q, qd, *[c if h else np.zeros_like(c) for c, h in zip(cs, have)], static=static, waves=waves)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), have
            if not any(have):
                assert not a[0].any() and not a[1].any()


@pytest.mark.parametrize("name", K.ENVS)
def test_inactive_contacts_contribute_nothing_through_force_and_wrench(name):
    t, g = _case(name)
    q, qd = g["q_in"], g["qd_in"]
    free = ~(g["point"][:, :, 1] < 0).any(axis=1) & ~g["edge"].astype(bool).any(axis=1)   # states without a penetrating contact
    assert free.any()
    gq, gqd = K.emu_con_backward(t, q, qd, None, None, g["c_force"], g["c_lw"], waves=kin_lib.waves_of(t))
    assert not gq[free].any() and not gqd[free].any()


@pytest.mark.parametrize("name", K.ENVS)
def test_composite_forward_matches_the_reference(name):
    """the read-out of the state a whole env-step of the reference ends in"""
    t, g = _case(name)
    out = K.emu_con_forward(t, g["comp_q"], g["comp_qd"], True, kin_lib.waves_of(t))
    check_forward(g, out, g["comp_edge"].astype(bool), name + " composite", prefix="comp_")


@pytest.mark.parametrize("name", K.ENVS)
def test_statement_matches_the_reference(name):
    """the float64 statement against the reference's own tensors and gradients, with the bounds of the kernels"""
    t, g = _case(name)
    q, qd = g["q_in"].astype(np.float64), g["qd_in"].astype(np.float64)
    edge = g["edge"].astype(bool)
    check_forward(g, K.forward_batch(t, q, qd), edge, name + " statement")
    keep = kept_states(edge)
    for tag in ("force", "lw", "all"):
        gq, gqd = K.adjoint_batch(t, q, qd, *cotangents(g, tag))
        for k, got, ref in (("gq", gq, project_tangent(t, q, g["gq_" + tag])), ("gqd", gqd, g["gqd_" + tag])):
            e, bound = rows_err(got, ref, keep), grad_bound(g["noise_%s_%s" % (k, tag)][keep])
            print("%s statement cotangent %-5s %-3s err %.2e bound %.1e" % (name, tag, k, e, bound))
            assert e < bound, (tag, k, e, bound)


@pytest.mark.parametrize("name", K.ENVS)
def test_statement_adjoint_equals_central_differences(name):
    """on the states whose contacts are at least 1e-3 from every switch, along a random tangent direction, to 1e-6"""
    t, g = _case(name)
    q, qd = g["q_in"].astype(np.float64), g["qd_in"].astype(np.float64)
    rs = np.random.RandomState(3)
    done, h = 0, 1e-6
    for b in range(len(q)):
        if K.switch_margin(t, q[b], qd[b]) < 1e-3:
            continue
        cs = [np.asarray(c[b], np.float64) for c in cotangents(g, "all")]
        gq, gqd = K.adjoint(t, q[b], qd[b], *cs)
        dq, dqd = project_tangent(t, q[b], rs.normal(size=t.n_q)).reshape(-1), rs.normal(size=t.n_qd)
        loss = lambda s: sum((o * c).sum() for o, c in zip(K.forward(t, q[b] + s * dq, qd[b] + s * dqd)[:4], cs))  # noqa: E731
        fd, an = (loss(h) - loss(-h)) / (2 * h), gq @ dq + gqd @ dqd
        assert abs(fd - an) <= 1e-6 * abs(fd), (b, fd, an)
        done += 1
    assert done >= 2, done   # (SNUHumanoid: 88 contacts, two of its six states keep every one of them 1e-3 from a switch)


def _user_case(path):
    from test_edge_cases_cpu import _tree_states
    t = ArticulationTemplate.load(path)
    q, qd, _ = _tree_states(t, np.random.default_rng(17), 6)
    return t, q.astype(np.float32), qd.astype(np.float32)


@pytest.mark.parametrize("static,label", [(False, "generic"), (True, "specialised")])
@pytest.mark.parametrize("tag,path", kin_lib.USER_MODELS)
def test_user_models_match_the_float64_statement(tag, path, static, label):
    """free, hinge, prismatic and ball joints, CSR-list subtrees (user_tree) and a 17-link row tree (user_rowtree)"""
    t, q, qd = _user_case(path)
    B, Cn, L = len(q), t.n_contacts, t.n_links
    assert Cn > 0
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    ref = K.forward_batch(t, q64, qd64)
    edge = np.abs(ref[0][:, :, 1]) < K.EDGE
    keep = kept_states(edge)
    cov = K.coverage(t, q64, qd64)
    assert min(cov.values()) > 0, cov
    out = K.emu_con_forward(t, q, qd, static, 1, user=True)
    for (k, _), a, r in zip(FWD, out, ref):
        e = (np.abs(a - r)[~edge].max() / np.abs(r).max()) if k == "force" else rows_err(a, r, keep if k == "lw" else slice(None))
        print(tag, label, "forward", k, "%.2e" % e)
        assert e < 1e-4, (k, e)
    rs = np.random.RandomState(11)
    cs = [rs.normal(size=s).astype(np.float32) for s in ((B, Cn, 3), (B, Cn, 3), (B, Cn, 3), (B, L, 6))]
    for sel in SETS:
        c = tuple(x if sel in (k, "all") else None for x, k in zip(cs, ("point", "vel", "force", "lw")))
        rq, rqd = K.adjoint_batch(t, q64, qd64, *c)
        runs = []
        for k in range(8):   # the statement's own deviation under +-1 ulp moves of the fp32 inputs
            r2 = np.random.RandomState(100 + k)
            q1 = np.nextafter(q, q + r2.choice([-1.0, 1.0], size=q.shape).astype(np.float32)).astype(np.float64)
            qd1 = np.nextafter(qd, qd + r2.choice([-1.0, 1.0], size=qd.shape).astype(np.float32)).astype(np.float64)
            runs.append(K.adjoint_batch(t, q1, qd1, *c))
        gq, gqd = K.emu_con_backward(t, q, qd, *c, static=static, waves=1, user=True)
        for k, got, r, j in (("gq", project_tangent(t, q, gq), rq, 0), ("gqd", gqd, rqd, 1)):
            dev = np.max([np.abs(project_tangent(t, q, x[j]) - r if j == 0 else x[j] - r).max(axis=1) for x in runs], axis=0)
            noise = dev / (np.abs(r).max() + 1e-30)
            e, bound = rows_err(got, r, keep), grad_bound(noise[keep])
            print("%s %s cotangent %-5s %-3s err %.2e  statement noise %.2e  bound %.1e" % (tag, label, sel, k, e, noise[keep].max(), bound))
            assert e < bound, (sel, k, e, bound)
        assert kin_lib.radial_part(t, q, gq) <= RADIAL


def test_cartpole_has_no_contacts():
    t = template_from_golden("cartpole")
    g = golden("cartpole_step")
    q, qd = g["q_in"], g["qd_in"]
    assert t.n_contacts == 0
    for static in (False, True):
        point, vel, force, lw = K.emu_con_forward(t, q, qd, static, 1)
        assert point.shape == (len(q), 0, 3) and not lw.any()
        gq, gqd = K.emu_con_backward(t, q, qd, None, None, None, np.ones_like(lw), static=static, waves=1)
        assert not gq.any() and not gqd.any()


def test_the_two_functions_are_exported_and_the_abi_number_stays():
    hdr = open(os.path.join(K.ROOT, "include", "dsim.h")).read()
    for fn in ("dsim_ground_contacts", "dsim_ground_contacts_backward"):
        assert fn in capi.EXPORTS and re.search(r"\bint %s\(" % fn, hdr)
    assert len(capi.ABI["dsim_ground_contacts"][1]) == 9 and len(capi.ABI["dsim_ground_contacts_backward"][1]) == 11
    assert capi.EXPECTED_ABI == 110
