"""The candidate rule of the persistent form's capacity query (csrc/residency_rule.hpp) against staged self-test outcomes, without a
GPU: a host-only C++ harness (tests/residency/rule_harness.cpp) compiled with AddressSanitizer + UBSan and run in a child process.
The fallback path -- the largest candidate grid fails the co-residency self-test -- is reachable here only: no GPU test makes a
self-test fail on purpose.  Expected values: the rule as it stood in the per-instance launcher, with blocks = 2 (the estimate),
api = 1 (the runtime's answer) and 256 CUs."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case -> (capacity, grids the self-test was run at, in order, `blocks` afterwards)
EXPECT = {
    "pass_450": (512, [450], 2),
    "want_300_after_450": (512, [], 2),          # a grid <= the validated one needs no self-test
    "fail_450_pass_256": (256, [450, 256], 1),
    "fail_always_450": (0, [450, 256], 2),       # the third candidate (one per CU) is not smaller than the second: skipped
    "fail_200": (0, [200], 2),                   # the same grid is not retried for a smaller candidate
    "cap100_pass": (100, [100], 2),              # HIPETS_MAX_WORKGROUPS=100: `blocks` is not updated from a capped answer
    "cap100_fail": (0, [100], 2),
}


def test_candidate_rule_against_staged_self_tests():
    import __graft_entry__ as ge

    exe = ge.build_residency_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr  # clean under ASan and UBSan
    got, pays = {}, None
    for line in out.stdout.splitlines():
        name, *fields = line.split()
        kv = dict(f.split("=") for f in fields)
        if name == "pays":
            pays = {k: int(v) for k, v in kv.items()}
        else:
            got[name] = (int(kv["capacity"]), [int(g) for g in kv["calls"].split(",") if g], int(kv["blocks"]))
    assert got == EXPECT
    # turns when one workgroup per CU is resident, one launch per step when two are and the batch still exceeds that
    assert pays == dict(one_per_cu_fits=1, turns=1, two_per_cu=1, beyond_two_per_cu=0)
