"""The operations dsim_math_quad.hpp adds for the adjoint's body level, on the host: the component-per-lane (quad) backend and the
one-link-per-lane (scalar) backend agree bit for bit, and both agree with the dsim_math.hpp / dsim_core.hpp functions they replace.

tests/quad/quad_adjoint_check.cpp is compiled here with the flags of tests/test_quad_math_cpu.py (the host harness's plus
-ffp-contract=off); its quads run lane-serially through the harness executor's shfl.  The same program is built a second time
with the address and undefined-behaviour sanitizers and run on its own (fewer rounds): it must exit cleanly with the same verdicts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "quad", "quad_adjoint_check.cpp")
OPS = ["ld_i10_mul", "scross_t", "scross_dual_t", "fcross_t", "sdot", "qmul_v", "sv_axpy", "bilinear_adj", "pose_wrench"]
ROUNDS = 250   # 16 random cases each: 4000 per operation
# the bound of tests/test_quad_math_cpu.py for the same comparison: both forms evaluate the same expression of a dozen or two
# terms with differently ordered fp32 roundings (2^-24 each), relative to the magnitude of those terms
REL_TOL = 1e-6
# (the harness source behind the executor is included whole; its per-model kernel instantiations are not needed here and are
# left out -- with them the sanitized build alone takes a quarter of an hour)
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
    """the plain and the sanitized build, compiled side by side (the harness behind the executor is a large translation unit)"""
    d = tmp_path_factory.mktemp("quad_adj")
    exe, san = str(d / "quad_adjoint_check"), str(d / "quad_adjoint_check_san")
    jobs = [subprocess.Popen([_cxx()] + FLAGS + ["-o", exe, SRC]),
            subprocess.Popen([_cxx()] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san, SRC])]
    assert [j.wait() for j in jobs] == [0, 0]
    return exe, san


@pytest.fixture(scope="module")
def results(builds):
    return _collect(builds[0], ROUNDS // 2, (1, 2))


def test_every_operation_is_covered(results):
    assert sorted(results) == sorted(OPS)
    assert all(results[k][0] >= 3 * 16 * (ROUNDS // 2) * 2 for k in OPS)


@pytest.mark.parametrize("op", OPS)
def test_quad_backend_matches_scalar_backend_bit_for_bit(results, op):
    n, bits, _ = results[op]
    print("%s: %d values, %d differ" % (op, n, bits))
    assert bits == 0


@pytest.mark.parametrize("op", OPS)
def test_quad_adjoint_math_matches_dsim_math(results, op):
    n, _, err = results[op]
    print("%s: %d values, max error / magnitude of the terms %.3e" % (op, n, err))
    assert err <= REL_TOL


def test_sanitized_build_runs_clean(builds):
    out = _collect(builds[1], 8, (3,))
    assert sorted(out) == sorted(OPS)
    for op in OPS:
        assert out[op][1] == 0 and out[op][2] <= REL_TOL, (op, out[op])
