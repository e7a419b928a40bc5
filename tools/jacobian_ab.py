"""One dsim_step_jacobian launch against n_q + n_qd sequential dsim_step_backward launches of the same build (Ant: 29), the only
way to a step Jacobian before ABI 110:
    python tools/jacobian_ab.py [n_envs ...]          (default: 16 1024; appends to profiles/step_jacobian_ab.txt with --record)
HIP events around each variant, median of 20 runs after 5 warm-ups.  Both variants read the same checkpoint and write device
buffers allocated once; the loop's one-hot cotangents are prepared outside the timed region."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from diffrl_amd.engine import Engine  # noqa: E402
from oracle_lib import golden, template_from_golden  # noqa: E402

RUNS, WARMUP = 20, 5


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main(argv):
    record = "--record" in argv
    sizes = [int(x) for x in argv if x.isdigit()] or [16, 1024]
    dev = torch.device("cuda:0")
    t, g = template_from_golden("ant"), golden("ant_step")
    eng = Engine(t, dev)
    S, mm, dt = int(g["substeps"]), int(g["mm_freq"]), float(g["dt"])
    nq, nd = t.n_q, t.n_qd
    K = nq + nd
    lines = []
    for n in sizes:
        rows = np.arange(n) % g["q_in"].shape[0]
        T = lambda a: torch.tensor(np.ascontiguousarray(a[rows], np.float32), device=dev).reshape(-1)   # noqa: E731
        q, qd, act = T(g["q_in"]), T(g["qd_in"]), T(g["act_in"])
        _, _, ck = eng.forward(q, qd, act, None, dt, S, mm, True)
        eye = torch.eye(K, device=dev)
        seeds = [(eye[k, :nq].repeat(n).contiguous(), eye[k, nq:].repeat(n).contiguous()) for k in range(K)]

        def loop():
            return [eng.backward(ck, act, None, dt, S, mm, sq, sqd) for sq, sqd in seeds]

        def one():
            return eng.step_jacobian(ck, act, None, dt, S, mm)

        Js = one()[0]
        ref = loop()
        assert all(torch.equal(Js[:, k, :nq].reshape(-1), ref[k][0]) and torch.equal(Js[:, k, nq:].reshape(-1), ref[k][1]) for k in range(K))
        t_loop, t_one = timed(loop), timed(one)
        lines.append("Ant N=%d (variant %d, substeps %d, mm_freq %d): %d x dsim_step_backward %.3f ms, 1 x dsim_step_jacobian %.3f ms, "
                     "ratio loop / single %.2f" % (n, eng.variant, S, mm, K, t_loop, t_one, t_loop / t_one))
        print(lines[-1], flush=True)
    if record:
        with open(os.path.join(ROOT, "profiles", "step_jacobian_ab.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
