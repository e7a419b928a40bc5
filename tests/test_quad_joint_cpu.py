"""The operations dsim_math_quad.hpp adds for the free root's integrator and its adjoint, and the two blocks themselves
(dq_root_integrate, dq_root_integrate_adj), on the host: the component-per-lane (quad) backend and the one-link-per-lane
(scalar) backend agree bit for bit, and both agree with the dsim_math.hpp forms the kernels used before.

tests/quad/quad_joint_check.cpp is compiled here with the flags of tests/test_quad_adjoint_cpu.py; its quads run lane-serially
through the harness executor's shfl.  Inputs are random unit quaternions and twists; case 0 of every round is the degenerate
one (|r + dr h|^2 underflows: il == 0), which must give the identity rotation / a zero rotation cotangent in both backends.
The same program is built a second time with the address and undefined-behaviour sanitizers and run on its own (fewer rounds)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "quad", "quad_joint_check.cpp")
OPS = ["qdot", "qmul_adj_a", "qmul_v", "qmul_v_int", "qnorm2_int", "scale_axpy_sel", "ld_st", "root_integrate", "root_integrate_adj"]
ROUNDS = 250   # 16 random cases each: 4000 per operation
# the bound of tests/test_quad_adjoint_cpu.py for the same comparison: both forms evaluate the same expression of a dozen or two
# terms with differently ordered fp32 roundings (2^-24 each), relative to the magnitude of those terms
REL_TOL = 1e-6
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-DDSIM_STATIC_VARIANTS(X)="]


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    return cxx


def _collect(exe, rounds, seeds):
    out = {}
    for seed in seeds:
        for line in subprocess.check_output([exe, str(rounds), str(seed)], text=True).splitlines():
            name, n, bits, err = line.split()
            o = out.setdefault(name, [0, 0, 0.0])
            o[0] += int(n)
            o[1] += int(bits)
            o[2] = max(o[2], float(err)) if float(err) == float(err) else float("nan")
    return out


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """the plain and the sanitized build, compiled side by side"""
    d = tmp_path_factory.mktemp("quad_joint")
    exe, san = str(d / "quad_joint_check"), str(d / "quad_joint_check_san")
    jobs = [subprocess.Popen([_cxx()] + FLAGS + ["-o", exe, SRC]),
            subprocess.Popen([_cxx()] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san, SRC])]
    assert [j.wait() for j in jobs] == [0, 0]
    return exe, san


@pytest.fixture(scope="module")
def results(builds):
    return _collect(builds[0], ROUNDS // 2, (1, 2))


def test_every_operation_is_covered(results):
    assert sorted(results) == sorted(OPS + ["degenerate_bad"])
    assert all(results[k][0] >= 4 * 16 * (ROUNDS // 2) * 2 for k in OPS)


@pytest.mark.parametrize("op", OPS)
def test_quad_backend_matches_scalar_backend_bit_for_bit(results, op):
    n, bits, _ = results[op]
    print("%s: %d values, %d differ" % (op, n, bits))
    assert bits == 0


@pytest.mark.parametrize("op", OPS)
def test_quad_joint_math_matches_dsim_math(results, op):
    n, _, err = results[op]
    print("%s: %d values, max error / magnitude of the terms %.3e" % (op, n, err))
    assert err <= REL_TOL


def test_degenerate_rotation_gives_identity_and_zero_cotangent(results):
    """il == 0: the identity quaternion out of the integrator, g_rt = 0 out of integrate^T, in both backends (the count of
    degenerate cases that gave anything else)"""
    assert results["degenerate_bad"][0] == 0


def test_sanitized_build_runs_clean(builds):
    out = _collect(builds[1], 8, (3,))
    assert sorted(out) == sorted(OPS + ["degenerate_bad"])
    assert out["degenerate_bad"][0] == 0
    for op in OPS:
        assert out[op][1] == 0 and out[op][2] <= REL_TOL, (op, out[op])
