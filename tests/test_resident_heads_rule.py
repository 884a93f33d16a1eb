"""Which DEVICE rollouts run the resident-heads instance (kspec.hpp KSpec::RES): the selection rule (csrc/residency_rule.hpp
resident_heads_wanted / resident_heads_kept -- what launch.hpp pick_rollout_instance and rollout.hip apply) as compiled, without a GPU:
a host-only harness (tests/residency/resident_heads_harness.cpp) built with AddressSanitizer + UBSan and run in a child process.
The instance keeps a wave's op heads of ONE member for the whole launch, so it is right only for the straight persistent form of the
R = 3 instances: the turn-based form (pop 1080 at R = 3: 450 logical workgroups on 256 CUs), other R, per-step launches and models
of another depth must not get it."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case -> (asked for, kept after the capacity query)
EXPECT = {
    "smallest_R3_pop12": (1, 1),
    "one_per_cu_R3_pop480": (1, 1),
    "headline_R3_pop500": (1, 1),
    "R4_one_per_cu": (0, 0),  # (no R = 4 instance: it spilt to scratch memory)
    "turns_R3_pop1080": (0, 0),
    "R1_pop360": (0, 0),
    "R1_small": (0, 0),
    "R2_small": (0, 0),
    "three_layer_model": (0, 0),
    "six_layer_model": (0, 0),
    "horizon_1": (0, 0),
    "exactly_256": (1, 1),
    "257": (0, 0),
    "capped_below_logical": (1, 0),
    "self_test_failed": (1, 0),
}


def test_resident_heads_selection_rule():
    import __graft_entry__ as ge

    exe = ge.build_resident_heads_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr.strip(), out.stderr  # clean under ASan and UBSan
    got = {}
    for line in out.stdout.splitlines():
        name, *fields = line.split()
        kv = dict(f.split("=") for f in fields)
        got[name] = (int(kv["wanted"]), int(kv["kept"]))
    assert got == EXPECT


def test_resident_instances_in_the_build_report():
    """Every fused R = 3 shape has its resident twin in the shipped library (the last KSpec argument is 1), none of them uses scratch
    memory, and their AccVGPR count stays within the file (pitfall: the allocator's own AccVGPR spill space shares it)."""
    import json

    import __graft_entry__ as ge

    ge.build_library()  # (nothing to do where the library is current)
    kernels = json.load(open(ge.BUILDINFO))["kernels"]
    res = {k: v for k, v in kernels.items() if "rollout_kernel" in k and k.split("EEEEEvNS")[0].endswith("Li1ELi1")}
    by_r = {r: [k for k in res if f"rollout_kernelILi{r}E" in k] for r in (1, 2, 3, 4)}
    assert len(by_r[3]) == 5 and not by_r[4] and not by_r[1] and not by_r[2], {r: len(v) for r, v in by_r.items()}
    for k, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["AGPRs"] <= 256 and v["Occupancy [waves/SIMD]"] == 1, (k, v)
