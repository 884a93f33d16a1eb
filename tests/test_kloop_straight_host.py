"""No whole-accumulator copies in the k loops of the fused fp32 rollout instances with one wave per SIMD (R = 3, 4), read off the build
report (libhipets.buildinfo.json: __graft_entry__.count_accumulator_moves counts, per rollout kernel, the v_mov_b64 and the runs of
>= 8 consecutive v_mov_b64 / v_mov_b32 between two MFMAs).

Where C++ control flow met around the asm MFMAs of csrc/gemm_f32.hpp -- the arms of the last chunk's switch over its 1..4 real k-steps,
the arms of the input layer's rolled loop -- the register allocator copied every accumulator of the wave: 18-22 v_mov_b64 in a row
between two MFMAs, and a pipe drain in front of each.  The k-steps of the last chunk now skip themselves inside their asm statement and
the input layer forks once into whole bodies (gemm_f32.hpp "conditional k-steps", kForked).  What is left, and the limits below:

                                         before (v_mov_b64 / runs)     now                 limit
  R = 3 resident-heads twins (5)         871 .. 1055 / 34 .. 42        122 .. 165 / 0      200 / 2
  R = 3 plain instances, DEVICE (5)      631 ..  813 / 26 .. 35        237 .. 301 / 6, 7   330 / 8
  R = 3 plain instances, FAST (5)        588 ..  735 / 26 .. 36        198 .. 223 / 6, 7   330 / 8
  R = 4 instances (DEVICE, FAST)         611, 529    / 18              247, 165   / 5      330 / 8

The runs left in the plain instances are no copies: every op body starts its 9-13 accumulators from the 3-4 bias quads of its column
tiles, ~20 v_mov_b64 in front of the body's first MFMA -- one run per op and one more for the input layer's second body (the twins
read their initial values from AccVGPRs: no v_mov at all).  Head-room: 10-20 % on the counts for another compiler's choices elsewhere in
the kernel, one or two runs (a sixth op body would be one); a single arm with its copies back adds ~20 v_mov_b64 and a run PER ARM and
op, i.e. hundreds -- at R = 3 every limit is below half of the smallest count before, and below two thirds of it at R = 4."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LIMITS = {"twin": (200, 2), "plain": (330, 8)}
# the counts of the two cfg2 kernels (HALFCHEETAH reward, three output tiles, DEVICE) before this change
BEFORE = {"twin": (963, 34), "plain": (701, 26)}


def lean_fp32_kernels():
    """{(R, KSpec arguments): report} of the fused fp32 instances with one wave per SIMD: KSpec<ACT, HIDC, OUTC, NORM, OBSP, REW, TERM, KMODE,
    PREC, FUSE, RES> with PREC 0 (fp32) and FUSE 1, R >= 3"""
    ge.build_library()
    out = {}
    for name, rep in json.load(open(ge.BUILDINFO))["kernels"].items():
        m = re.search(r"rollout_kernelILi(\d)ENS_5KSpecI((?:Lin?\d+E)+)EEE", name)
        if not m:
            continue
        args = tuple(int(a.replace("n", "-")) for a in re.findall(r"Li(n?\d+)E", m.group(2)))
        if int(m.group(1)) >= 3 and len(args) == 11 and args[8] == 0 and args[9] == 1:
            out[(int(m.group(1)), args)] = rep
    return out


def test_the_build_report_counts_moves_of_every_rollout_kernel():
    ge.build_library()
    kernels = json.load(open(ge.BUILDINFO))["kernels"]
    rollout = {k: v for k, v in kernels.items() if "rollout_kernel" in k}
    assert len(rollout) >= 20
    for name, rep in rollout.items():
        assert {"v_mov_b64", "mov_runs", "codeLenInByte"} <= set(rep), name


def test_lean_fp32_instances_hold_no_whole_accumulator_copies():
    ks = lean_fp32_kernels()
    assert sorted(R for R, _ in ks) == [3] * 15 + [4] * 2  # five shapes x (twin, DEVICE, FAST) at R = 3; one shape x (DEVICE, FAST) at R = 4
    assert sum(args[10] for _, args in ks) == 5
    for (R, args), rep in ks.items():
        movs, runs = LIMITS["twin" if args[10] else "plain"]
        print("KLOOP_MOVES", R, args, rep["v_mov_b64"], rep["mov_runs"], rep["codeLenInByte"])
        assert rep["v_mov_b64"] <= movs and rep["mov_runs"] <= runs, (R, args, rep)


def test_the_limits_refuse_the_counts_before():
    for kind, (movs, runs) in BEFORE.items():
        assert movs > 2 * LIMITS[kind][0] and runs > 2 * LIMITS[kind][1]


def test_counter_on_a_snippet(tmp_path):
    """count_accumulator_moves: a run counts between two MFMAs only, shorter runs and runs in front of the first MFMA do not"""
    mfma = "\tv_mfma_f32_16x16x4_f32 v[0:3], v8, v9, v[0:3]\n"
    mov = "\tv_mov_b64_e32 v[10:11], v[0:1]\n"
    body = mov * 9 + mfma + mov * 8 + mfma + mov * 7 + "\ts_nop 1\n" + mov * 7 + mfma + mov * 4 + "\tv_mov_b32_e32 v1, v2\n" * 4 + "\ts_nop 0\n" + mfma
    p = tmp_path / "k.s"
    p.write_text("_Z14rollout_kernelIfEvv:   ; @_Z14rollout_kernelIfEvv\n" + body + "\ts_endpgm\n; codeLenInByte = 512\nother:   ; @other\n" + mov * 9)
    assert ge.count_accumulator_moves(str(p)) == {"_Z14rollout_kernelIfEvv": {"v_mov_b64": 35, "mov_runs": 2, "codeLenInByte": 512}}
