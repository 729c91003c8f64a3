"""The step's schedule, launch by launch (emulator): which kernels, memsets, copies, event records and stream waits a submit
issues, with what grid / workgroup / LDS size, on which stream and in which order.  The emulator runs every launch at once,
so a kernel that moved to the wrong stream or a wait that was dropped changes no result and no parity test sees it; the
fake runtime's trace (tests/hostsim/sim.cpp, FASTP_SIM_TRACE) does.  Each case creates its engine in a fresh child process
(streams and events are labelled by their order of creation in the process), submits one small batch and compares the trace
from fastp_gpu_create's return onward with tests/golden/launch_trace/<case>.txt, line for line.

A golden changes only on purpose, in a change that means to change the schedule: record it again
(`python tests/test_launch_trace.py --record`) and say in that change what moved and why.  A refactor of the host code
leaves every golden as it is."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "launch_trace")
EXOTIC_UNITS = (3, 17, 40)
TILE = {"FASTP_GPU_LANE": "0"}                              # the split plan's tile kernel
FUSED = {"FASTP_GPU_LANE": "0", "FASTP_GPU_SPLIT": "0"}     # Stats inside the one kernel

# case -> (option family of test_launch_geometry.FAMILIES (+ "_overrep": the overrepresentation analysis on),
#          environment switches, what else differs from "one submit of 64 units of 100 bases")
CASES = {
    "pe_default": ("pe_default", {}, {}),                                        # lane plan, claim fused, Duplicate's tail on the tail stream
    "se_default": ("se_default", {}, {}),
    "pe_default_tile": ("pe_default", TILE, {}),
    "pe_default_fused": ("pe_default", FUSED, {}),
    "pe_default_unaligned": ("pe_default", {}, {"unaligned": True}),             # rows off 16 bytes: the tile kernel instead of the lane kernel
    "pe_claim_own_kernel": ("pe_default", {"FASTP_GPU_CLAIM_FUSED": "0"}, {}),
    "pe_c_dedup3": ("pe_c_dedup3", {}, {}),                                      # --dedup folded
    "pe_c_dedup3_prepass": ("pe_c_dedup3", {"FASTP_GPU_DEDUP_FOLD": "0"}, {}),   # the hash pre-pass
    "pe_c_dedup3_L203": ("pe_c_dedup3", {}, {"L": 203}),                         # fused plan with --dedup
    "pe_c": ("pe_c", {}, {}),                                                    # correction list, link and corr-stats kernels
    "pe_cut_front": ("pe_cut_front", {}, {}),                                    # front-stats kernel
    "pe_merge": ("pe_merge", {}, {}),
    "pe_merge_unaligned": ("pe_merge", {}, {"unaligned": True}),                 # rows copied to aligned arrays
    "pe_overrep": ("pe_default_overrep", {}, {}),                                # early, on the tail stream
    "pe_overrep_fused": ("pe_default_overrep", FUSED, {}),                       # at the end of the step
    "pe_overrep_deferred": ("pe_default_overrep", {}, {"drive": "deferred"}),    # FASTP_GPU_BATCH_DEFER_OVERREP, then fastp_gpu_overrep_device
    "pe_exotic_lane": ("pe_default", {}, {"exotic": True}),                      # the text kernel beside the lane kernel
    "pe_exotic_tile": ("pe_default", TILE, {"exotic": True}),                    # on the tail stream behind the tile kernel
    "pe_exotic_fused": ("pe_default", FUSED, {"exotic": True}),                  # inline
    "pe_exact_all": ("pe_default", {"FASTP_GPU_EXACT": "1"}, {}),
    "pe_exotic_dedup": ("pe_c_dedup3", {}, {"exotic": True}),
    "pe_exotic_overrep": ("pe_default_overrep", {}, {"exotic": True}),
    "pe_sharded": ("pe_default", {}, {"drive": "sharded"}),                      # pass 1, then pass 2
    "pe_sharded_dedup": ("pe_c_dedup3", {}, {"drive": "sharded"}),
    "pe_sharded_exotic_dedup": ("pe_c_dedup3", {}, {"drive": "sharded", "exotic": True}),
    # (tiles of 8 pairs, one per workgroup: 192 units per launch on the emulator's three CUs - two launches)
    "pe_several_launches": ("pe_default", {"FASTP_GPU_MAX_TILES_PER_BLOCK": "1", "FASTP_GPU_TILE": "8"}, {"n": 300}),
    "pe_empty_batch": ("pe_default", {}, {"n": 0}),
}


def _unalign(tens, b, paired):
    """the batch's rows 4 bytes off a 16-byte boundary"""
    import torch
    for name in ("seq1", "qual1") + (("seq2", "qual2") if paired else ()):
        t = torch.zeros(tens[name].numel() + 32, dtype=torch.uint8)
        off = 4 + (-t.data_ptr()) % 16
        t[off:off + tens[name].numel()] = tens[name]
        tens[name + "_off"] = t
        setattr(b, name, t.data_ptr() + off)


def run_case(case, out_path, lib_path=None):
    """(child process) the case's engine and one batch; the trace starts when fastp_gpu_create has returned"""
    import torch

    import cases
    import engines
    import shard_util
    import synth
    import test_launch_geometry as geo
    from fastp_amd import abi, engine
    fam, _, how = CASES[case]
    L, n, drive = how.get("L", 100), how.get("n", 64), how.get("drive", "submit")
    overrep = fam.endswith("_overrep")
    fam = fam[:-len("_overrep")] if overrep else fam
    paired = geo.FAMILIES[fam][0]
    p = geo.params_for(fam, L, 512)
    d = synth.synth_pairs(max(n, 1), L=L, seed=11, paired=paired, dup_frac=0.3)
    if overrep:
        p = cases.finalize_params("pe_overrep", p, d["seq1"], d["len1"], d.get("seq2"), d.get("len2"))
    if how.get("exotic"):
        for u in EXOTIC_UNITS:
            d["seq1"][u, 1] = ord("R")
    eng = engine.GpuEngine(p, lib_path=lib_path or engines.build_sim())
    batches, results, keep = shard_util.device_batches(eng, d, 0, n, 1, torch.device("cpu"))
    b, r = batches[0], results[0]
    if how.get("unaligned"):
        _unalign(keep[0][0], b, paired)
    os.environ["FASTP_SIM_TRACE"] = out_path
    if drive == "sharded":
        scan = torch.zeros(max(16, eng.dup_scan_bytes(n)), dtype=torch.uint8)
        eng.submit_pass1_device(b, scan.data_ptr(), r)
        eng.submit_pass2_device(b, scan.data_ptr(), r)
    elif drive == "deferred":
        b.flags |= abi.BATCH_DEFER_OVERREP
        eng.submit_device(b, r)
        eng.overrep_device(b, r)
    else:
        eng.submit_device(b, r)
    eng.synchronize()
    del os.environ["FASTP_SIM_TRACE"]
    eng.close()


def trace_of(case, out_path, lib_path=None):
    env = dict(os.environ)
    for k in [k for k in env if k.startswith(("FASTP_GPU_", "FASTP_SIM_"))]:
        del env[k]
    env.update(CASES[case][1])
    open(out_path, "w").close()
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, out_path] + ([lib_path] if lib_path else []),
                   env=env, check=True, timeout=300)
    with open(out_path) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("case", list(CASES))
def test_sim_launch_trace_equals_golden(case, tmp_path):
    import engines
    engines.build_sim()
    with open(os.path.join(GOLDEN_DIR, case + ".txt")) as f:
        golden = f.read().splitlines()
    got = trace_of(case, str(tmp_path / "trace.txt"))
    assert got, "the emulator wrote no trace"
    first = next((i for i, (a, b) in enumerate(zip(got, golden)) if a != b), min(len(got), len(golden)))
    assert got == golden, (f"{case}: the schedule differs from the golden at line {first + 1} ({len(got)} lines, golden {len(golden)}):\n"
                           f"  now    {got[first] if first < len(got) else '(end)'}\n"
                           f"  golden {golden[first] if first < len(golden) else '(end)'}")


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        run_case(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None)
    elif sys.argv[1] == "--record":   # [library [case ...]]: the emulator library to record from (default: this tree's)
        os.makedirs(GOLDEN_DIR, exist_ok=True)
        for c in sys.argv[3:] or CASES:
            n = len(trace_of(c, os.path.join(GOLDEN_DIR, c + ".txt"), sys.argv[2] if len(sys.argv) > 2 else None))
            print(f"{c}: {n} lines")
