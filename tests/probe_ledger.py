"""One policy for "probed" gradient tolerances, and a LOUD record of every time it is used.

Stated tolerance of every gradient comparison: 1e-3 max-norm relative.  A comparison above it may
pass only if the REFERENCE-order gradient is itself that sensitive at these inputs -- contacts switch on / off, friction
switches regime and joint limits engage at thresholds, so gradients are piecewise and a state that differs in the 7th digit
can sit on the other side of a threshold -- which the caller shows by recomputing the gradient with the scalar oracle
(reference operation order) from inputs perturbed by 1e-7 .. 1e-5 ("the probe").  This module makes that escape hatch
bounded and visible:

  * the accepted error is  max(1e-3, FACTOR x sensitivity)  and never more than a hard CEILING per level
    (one env-step: 5e-3; H = 32 rollouts / episodes, whose gradients multiply through 512-1536 substeps: 1e-2 -- round 6;
    the largest error of a probed environment is 9.7e-3 -- a Humanoid 1024 x 32 environment whose reference-order sensitivity is
    9.7e-3 too, tests/test_reference_episodes.py --, 5.7e-3 on round 5's sparser sample; the ceiling was 2e-2 in round 5 and 5e-2 before);
  * every test that may use the probe states a BUDGET -- how many of its cases may need it (today's measured counts);
    one more than that fails the test, so a real adjoint regression cannot hide behind "sensitive environment";
  * every use is recorded: a UserWarning (pytest prints its warnings summary even with -q), a line in
    gpurun_out/probe_ledger.jsonl, and a "probed tolerances" section at the end of the run (tests/conftest.py).
"""
import json
import os
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER_PATH = os.environ.get("DSIM_PROBE_LEDGER") or os.path.join(ROOT, "gpurun_out", "probe_ledger.jsonl")
STATED = 1e-3
FACTOR = 3.0
CEILING = {"step": 5e-3, "rollout": 1e-2}
SAMPLED = {}       # test id -> (cases compared, what) for the "probed fraction" line of the summary (note_sampled)
STATED_FORM = {}   # test id -> (what, whole-tensor max-norm relative error, cosine, cases): BASELINE.md section 4's own figures, un-probed
ENTRIES = []       # this session's records, printed by conftest.pytest_terminal_summary
_USED = {}         # test id -> probed cases so far


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]


def accept(level, measured, sensitivity, budget, what="", factor=FACTOR):
    """Tolerance for ONE case whose measured error is `measured` (>= 1e-3) and whose reference-order sensitivity the caller
    has probed; records the use and enforces the test's budget of probed cases.  Returns the tolerance to assert against."""
    tid = _test_id()
    tol = min(max(STATED, factor * float(sensitivity)), CEILING[level])
    n = _USED[tid] = _USED.get(tid, 0) + 1
    rec = dict(test=tid, level=level, what=str(what), error=float(measured), sensitivity=float(sensitivity), tolerance=tol,
               used=n, budget=int(budget))
    ENTRIES.append(rec)
    try:
        os.makedirs(os.path.dirname(LEDGER_PATH), exist_ok=True)
        with open(LEDGER_PATH, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    warnings.warn("PROBED TOLERANCE %s %s: error %.2e > 1e-3 accepted up to %.2e (reference-order sensitivity %.2e), case %d of a "
                  "budget of %d" % (tid, what, measured, tol, sensitivity, n, budget), UserWarning, stacklevel=2)
    assert n <= budget, ("%s: %d cases needed a probed tolerance, the budget is %d -- either an adjoint regression or a new "
                         "sensitive case that must be looked at (gpurun_out/probe_ledger.jsonl)" % (tid, n, budget))
    return tol


def note_sampled(n, what=""):
    """a test that compares n cases (environments) against the stated tolerance says so: the summary prints the probed fraction"""
    SAMPLED[_test_id()] = (int(n), str(what))


def note_stated(what, whole_tensor_err, cosine, n):
    """the stated tolerance's own form for one recording -- max-norm relative error over the whole gradient tensor and the cosine,
    no probe involved -- for the summary at the end of the run"""
    STATED_FORM[_test_id()] = (str(what), float(whole_tensor_err), float(cosine), int(n))
    try:
        os.makedirs(os.path.dirname(LEDGER_PATH), exist_ok=True)
        with open(LEDGER_PATH, "a") as f:
            f.write(json.dumps(dict(test=_test_id(), level="stated-form", what=str(what), whole_tensor_relerr=float(whole_tensor_err),
                                    cosine=float(cosine), cases=int(n))) + "\n")
    except OSError:
        pass


def reset():
    _USED.clear()
    SAMPLED.clear()
    STATED_FORM.clear()
    del ENTRIES[:]
