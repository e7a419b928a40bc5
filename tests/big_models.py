"""Large random articulations for the envelope tests of both tiers (tests/test_model_envelope_cpu.py on the host harness,
tests/test_gpu_model_envelope.py on the kernels): models of 22 to 64 links at the limits dsim_model_create admits (64 links,
64 dofs, 96 coordinates, 160 KiB of LDS; include/dsim.h "Admitted models").  Test infrastructure only.

big_tree() is the builder, MODELS the set A-F of the tests (built once per process through model()), each with the property that
puts it on the code path it is there for; check_property() asserts that property from the layout, so a change of the builder
cannot move a model off its path unnoticed."""
import functools

import numpy as np

from diffrl_amd import dflex as df

NL = 64                       # lanes of a wavefront (dsim_core.hpp: DSIM_NL)
LIMITS = dict(L=64, nd=64, nq=96, lds_bytes=160 * 1024, literal_L=24, literal_nd=28)
_NQ = {df.JOINT_PRISMATIC: 1, df.JOINT_REVOLUTE: 1, df.JOINT_BALL: 4, df.JOINT_FIXED: 0, df.JOINT_FREE: 7}
_ND = {df.JOINT_PRISMATIC: 1, df.JOINT_REVOLUTE: 1, df.JOINT_BALL: 3, df.JOINT_FIXED: 0, df.JOINT_FREE: 6}


def big_tree(seed, n_links, floating, kinds=(df.JOINT_REVOLUTE,), branch=3, shapes=1, armature=0.05, muscles=0, exact_kinds=None,
             shape_kinds=("sphere",), max_nd=64, max_nq=96):
    """Random articulation of n_links links, deterministic by seed.  The parent of link i is drawn from the three links around
    (i - 1) // branch, so the depth stays logarithmic and H well conditioned; the numbering is breadth-first (subtrees are not
    index ranges: the CSR-list code paths run, as with test_edge_cases_cpu._random_tree).  Root: a free joint (floating) or a hinge.
    kinds: the joint kinds the other links draw from -- a draw that would leave fewer than one dof / coordinate of the budget
    (max_nd, max_nq) per remaining link becomes a hinge; exact_kinds: the kinds of links 1 .. n_links - 1 as given instead.
    shapes: shapes per link (int, or a (low, high) range drawn per link) of shape_kinds ("sphere": one contact, "capsule": two,
    "box": eight).  muscles: line-of-action muscles of 3 to 5 way-points on random links.  -> (template, parents)"""
    rng = np.random.default_rng(seed)
    b = df.sim.ModelBuilder()
    b.add_articulation()
    parents = [-1]
    for i in range(1, n_links):
        c = (i - 1) // branch
        parents.append(int(rng.integers(max(0, c - 1), min(i - 1, c + 1) + 1)))
    nq = nd = 0
    for i in range(n_links):
        if i == 0:
            kind = df.JOINT_FREE if floating else df.JOINT_REVOLUTE
        elif exact_kinds is not None:
            kind = exact_kinds[i - 1]
        else:
            kind = kinds[int(rng.integers(0, len(kinds)))]
            left = n_links - 1 - i
            if nd + _ND[kind] + left > max_nd or nq + _NQ[kind] + left > max_nq:
                kind = df.JOINT_REVOLUTE
        nq, nd = nq + _NQ[kind], nd + _ND[kind]
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        rot = rng.normal(size=4)
        rot /= np.linalg.norm(rot)
        pos = (0.0, 0.0, 0.0) if i == 0 else tuple(rng.uniform(-0.25, 0.25, 3))
        link = b.add_link(parents[i], df.transform(pos, tuple(rot)), tuple(axis), kind, stiffness=float(rng.uniform(0, 2)),
                          damping=float(rng.uniform(0.05, 0.5)), limit_lower=-0.8, limit_upper=0.8, armature=armature)
        ns = shapes if isinstance(shapes, int) else int(rng.integers(shapes[0], shapes[1] + 1))
        for _ in range(ns):
            sk = shape_kinds[int(rng.integers(0, len(shape_kinds)))]
            kw = dict(ke=1e4, kd=1e3, kf=1e3, mu=float(rng.uniform(0.3, 1.0)))
            if sk == "sphere":
                b.add_shape_sphere(link, pos=tuple(rng.uniform(-0.1, 0.1, 3)), radius=0.08, **kw)
            elif sk == "capsule":
                b.add_shape_capsule(link, pos=tuple(rng.uniform(-0.1, 0.1, 3)), radius=0.05, half_width=0.12, **kw)
            else:
                b.add_shape_box(link, pos=tuple(rng.uniform(-0.05, 0.05, 3)), hx=0.08, hy=0.05, hz=0.06, **kw)
    for _ in range(muscles):
        k = int(rng.integers(3, 6))
        links = [int(x) for x in rng.integers(0, n_links, k)]
        b.add_muscle(links, [tuple(rng.uniform(-0.1, 0.1, 3)) for _ in range(k)], 1.0, 0.1, 0.1, 0.2, 0.0)
    if floating:
        b.joint_q[0:3] = [0.0, 0.3, 0.0]
    m = b.finalize("cpu")
    m.ground = True
    m.gravity = (0.0, -9.81, 0.0)
    m.collide()
    return m.template(), parents


_R, _P, _B, _X = df.JOINT_REVOLUTE, df.JOINT_PRISMATIC, df.JOINT_BALL, df.JOINT_FIXED
# model E: 24 links, 6 + 2 * 3 + 16 = 28 dofs (two ball joints, sixteen hinges, five rigidly attached links)
_E_KINDS = [_B, _R, _R, _X, _R, _R, _B, _R, _X, _R, _R, _R, _X, _R, _R, _R, _X, _R, _R, _R, _X, _R, _R]

MODELS = {
    # L = nd = 64 on a fixed root, C = 64: both hard limits at once, every `L < NL` / `nd < NL` decision at its boundary
    "A": dict(seed=1, n_links=64, floating=False, kinds=(_R, _P), branch=3, shapes=1),
    # contacts next to the links on one wave no longer fit: L + C > 64 with C <= 64 (one wave), dofs beyond lane 32
    "B": dict(seed=2, n_links=40, floating=True, kinds=(_R, _P), branch=3, shapes=1),
    # 21 ball joints under a hinge: nd = 64 with 22 links, nq = 85
    "C": dict(seed=3, n_links=22, floating=False, kinds=(_B,), branch=3, shapes=1),
    # more than 64 contacts and no muscles: the four-wave generic kernels.  (Seed 4 with armature 0.05 had cond(H) = 5e3 and its qdd
    # read-out at 1.0e-4 of the oracle's, the bound itself: the model was changed, not the bound.)
    "D": dict(seed=14, n_links=36, floating=True, kinds=(_R, _P, _B, _R), branch=3, shapes=(2, 3), max_nd=60, armature=0.1),
    # the literal adjoint exactly at its limit of 24 links / 28 dofs
    "E": dict(seed=5, n_links=24, floating=True, exact_kinds=_E_KINDS, branch=3, shapes=1),
    # B with 40 muscles
    "F": dict(seed=2, n_links=40, floating=True, kinds=(_R, _P), branch=3, shapes=1, muscles=40),
    # E with one more rigidly attached link: beyond the literal adjoint's limit, inside every other
    "E25": dict(seed=5, n_links=25, floating=True, exact_kinds=_E_KINDS + [_X], branch=3, shapes=1),
}
BASE = ("A", "B", "C", "D", "E", "F")
SCHEDULES = ((4, 2), (3, 3))


@functools.lru_cache(maxsize=None)
def model(name):
    """(template, parents) of MODELS[name], built once per process"""
    return big_tree(**MODELS[name])


def dims_of(t):
    from diffrl_amd import specialise
    off, d = specialise.layout(t)
    return off, d


def expected_waves(d):
    """dsim_hip.hip: pick_waves for the generic kernels without the DSIM_WAVES override"""
    return 4 if (d["NS"] > NL or d["C"] > NL) else 1


def check_property(name, t):
    """the property that makes MODELS[name] cover its path (the comments at MODELS), from the layout and the template"""
    off, d = dims_of(t)
    L, nd, nq, C, NS = d["L"], d["nd"], d["nq"], d["C"], d["NS"]
    ty = [int(x) for x in t.joint_type]
    assert off["total_words"] * 4 <= LIMITS["lds_bytes"]
    assert d["flags"] & 1 == 0, "breadth-first numbering: the CSR-list paths"
    if name == "A":
        assert (L, nd, C) == (64, 64, 64) and ty[0] == _R and set(ty) == {_R, _P} and NS == 0 and expected_waves(d) == 1
    elif name == "B":
        assert ty[0] == df.JOINT_FREE and 33 <= L <= 63 and nd > 32 and 64 - L < C <= 64 and NS == 0 and expected_waves(d) == 1
    elif name == "C":
        assert L == 22 and nd == 64 and nq == 85 and ty[0] == _R and all(x == _B for x in ty[1:]) and expected_waves(d) == 1
    elif name == "D":
        assert ty[0] == df.JOINT_FREE and 33 <= L <= 40 and {_R, _P, _B} <= set(ty) and C > 64 and NS == 0
        assert nd > 32 and expected_waves(d) == 4
    elif name == "E":
        assert (L, nd) == (LIMITS["literal_L"], LIMITS["literal_nd"]) and ty[0] == df.JOINT_FREE and _B in ty
    elif name == "E25":
        assert L == LIMITS["literal_L"] + 1 and nd <= LIMITS["literal_nd"]
    elif name == "F":
        tb = model("B")[0]
        assert L == tb.n_links and nd == tb.n_qd and (np.asarray(t.joint_parent) == np.asarray(tb.joint_parent)).all()
        assert t.n_muscles == 40 and 0 < NS and L > 32
    return off, d


# seeds of states(): one constant per model, so that a model added later leaves the states -- and the recorded figures -- of these alone
STATE_SEEDS = {"A": 1000, "B": 1001, "C": 1002, "D": 1003, "E": 1004, "E25": 1005, "F": 1006}


def states(name, n):
    """(q, qd, act, mact | None, gq_out, gqd_out) of n environments of MODELS[name], deterministic"""
    from test_edge_cases_cpu import _tree_states
    t = model(name)[0]
    rng = np.random.default_rng(STATE_SEEDS[name])
    q, qd, act = _tree_states(t, rng, n)
    mact = rng.uniform(0.0, 10.0, (n, t.n_muscles)).astype(np.float32) if t.n_muscles else None
    gq, gqd = rng.normal(0, 1, q.shape).astype(np.float32), rng.normal(0, 1, qd.shape).astype(np.float32)
    return q, qd, act, mact, gq, gqd


@functools.lru_cache(maxsize=None)
def oracle_case(name, n, S, mm):
    """(inputs, oracle_backward's result) of n environments of one schedule: computed once per process, shared, never modified"""
    from oracle_lib import oracle_backward
    t = model(name)[0]
    x = states(name, n)
    q, qd, act, mact, gq, gqd = x
    return x, oracle_backward(t, q, qd, act, mact, S / 960.0, S, mm, gq, gqd)


def step_errors(t, q, out, o):
    """max-norm relative errors of (q_out, qd_out, gq, gqd, gact, gmact | None) against oracle_backward's result -> (state, gradients)"""
    from oracle_lib import project_tangent, relerr
    qo, qdo, gq, gqd, gact, gmact = out
    state = dict(q=relerr(qo, o["q_out"]), qd=relerr(qdo, o["qd_out"]))
    grad = dict(gq=relerr(project_tangent(t, q, gq), project_tangent(t, q, o["gq"])), gqd=relerr(gqd, o["gqd"]), gact=relerr(gact, o["gact"]))
    if t.n_muscles:
        grad["gmact"] = relerr(gmact, o["gmact"])
    return state, grad


@functools.lru_cache(maxsize=None)
def mass_reference(name, n):
    """(q, H [n, nd, nd], S [n, nd, 6]) in float64: H = J^T M J + diag(armature) with the scalar oracle's world-frame axes S_s and
    spatial inertias I_s of the first substep -- row d of J_i is S_s[d] where dof d belongs to link i or one of its ancestors"""
    import mass_lib
    from oracle_lib import oracle_forward
    t = model(name)[0]
    q, qd, act, mact = states(name, n)[:4]
    dbg = oracle_forward(t, q, np.zeros_like(qd), np.zeros_like(act), None if mact is None else np.zeros_like(mact), 1.0 / 960.0, 1, 1,
                         debug=True)[2]
    S, I = dbg["S_s"].astype(np.float64), dbg["I_s"].astype(np.float64)
    mask = mass_lib.link_dof_mask(t).astype(np.float64)
    J = np.einsum("id,bdk->bidk", mask, S)
    H = np.einsum("bidk,bikl,bigl->bdg", J, I, J) + np.diag(np.asarray(t.joint_armature, np.float64))
    return q, H, S


@functools.lru_cache(maxsize=None)
def lds_limit_pair():
    """(template just below, template just above) the 160 KiB LDS limit: model A with muscles added until total_words * 4 crosses it
    (bisection over the muscle count: the image grows with every muscle)"""
    from diffrl_amd import specialise
    words = lambda m: specialise.layout(big_tree(**dict(MODELS["A"], muscles=m))[0])[0]["total_words"]  # noqa: E731
    lo, hi = 0, 64
    while words(hi) * 4 <= LIMITS["lds_bytes"]:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if words(mid) * 4 <= LIMITS["lds_bytes"] else (lo, mid)
    return big_tree(**dict(MODELS["A"], muscles=lo))[0], big_tree(**dict(MODELS["A"], muscles=hi))[0]
