"""dsim_math_quad.hpp on the host: the component-per-lane (quad) backend and the one-link-per-lane (scalar) backend of every
operation agree bit for bit, and both agree with the dsim_math.hpp functions they replace.

tests/quad/quad_math_check.cpp is compiled here with the flags of the host harness (tests/emu) plus -ffp-contract=off (the
header's own contraction pragma is clang's); its quads run lane-serially through the harness executor's shfl."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "quad", "quad_math_check.cpp")
OPS = ["add", "scale", "axpy", "cross", "dot3", "qmul", "rotate", "rot_cols", "sym_mul", "inertia_mul", "world_inertia", "scross"]
ROUNDS = 250   # 16 random cases each: 4000 per operation
# Both forms evaluate the same expression of at most ~10 terms with differently ordered fp32 roundings (2^-24 each), so they
# differ by a few 1e-7 of the magnitude of those terms; 1e-6 is the bound the change was specified with.
REL_TOL = 1e-6


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("quad") / "quad_math_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe, SRC])
    out = {}
    for seed in (1, 2):
        for line in subprocess.check_output([exe, str(ROUNDS // 2), str(seed)], text=True).splitlines():
            name, n, bits, err = line.split()
            o = out.setdefault(name, [0, 0, 0.0])
            o[0] += int(n)
            o[1] += int(bits)
            o[2] = max(o[2], float(err)) if float(err) == float(err) else float("nan")
    return out


def test_every_operation_is_covered(results):
    assert sorted(results) == sorted(OPS)
    assert all(results[k][0] >= 3 * 16 * (ROUNDS // 2) * 2 for k in OPS)


@pytest.mark.parametrize("op", OPS)
def test_quad_backend_matches_scalar_backend_bit_for_bit(results, op):
    n, bits, _ = results[op]
    print("%s: %d values, %d differ" % (op, n, bits))
    assert bits == 0


@pytest.mark.parametrize("op", OPS)
def test_quad_math_matches_dsim_math(results, op):
    n, _, err = results[op]
    print("%s: %d values, max error / magnitude of the terms %.3e" % (op, n, err))
    assert err <= REL_TOL
