"""Launch geometry at its thresholds (emulator): fastp_gpu_create picks the plan, every kernel's LDS layout, the lane kernel's
SWM / ext instantiation and the Stats kernel's form from max_len, cycles (2 x max_len with --merge), insert_size_max, the dup
accuracy level, the options and the device's LDS per workgroup.  The emulator (tests/hostsim) refuses a launch, or a
hipFuncSetAttribute, above the emulated sharedMemPerBlock (160 KiB; FASTP_SIM_LDS_BYTES sets less), the way the runtime does,
so a layout that does not fit fails here instead of on the card.  The parity cases at the thresholds have GPU twins below
(test_gpu_thresholds_equal_oracle); the sweep and the sizing checks need no GPU (a refusal at create launches nothing)."""
import re

import numpy as np
import pytest

import engines
import oraclelib
import synth
from fastp_amd import abi, engine

LDS_BYTES = 160 * 1024      # the MI355X's LDS per workgroup (hipDeviceProp_t::sharedMemPerBlock)
FASTA = [b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGGGTGCCAAGG"]


def _dedup(level):
    return lambda p: (setattr(p, "correction", 1), setattr(p, "dedup", 1), setattr(p, "dup_accuracy_level", level))


# option families: (paired, how the params are set, the longest reads it has the lane plan for, Stats in one pass); levels 3 - 5
# keep four bloom buffers whose hash primes need a fourth byte plane above 202 bases, level 6 has eight buffers
LANE_MAX = 256
FAMILIES = {
    "pe_default": (True, lambda p: None, LANE_MAX, True),
    "se_default": (False, lambda p: None, LANE_MAX, True),
    "pe_c": (True, lambda p: setattr(p, "correction", 1), LANE_MAX, False),
    **{f"pe_c_dedup{lv}": (True, _dedup(lv), {1: LANE_MAX, 2: LANE_MAX, 6: 0}.get(lv, 202), False) for lv in range(1, 7)},
    "pe_merge": (True, lambda p: (setattr(p, "merge", 1), setattr(p, "correction", 1)), LANE_MAX, False),
    "pe_cut_front": (True, lambda p: (setattr(p, "cut_front", 1), setattr(p, "cut_right", 1)), LANE_MAX, False),
    "pe_trim_front": (True, lambda p: (setattr(p, "trim_front1", 3), setattr(p, "trim_front2", 5)), LANE_MAX, False),
    "pe_umi": (True, lambda p: (setattr(p, "umi_len1", 8), setattr(p, "length_required", 15)), LANE_MAX, False),
    "pe_fasta": (True, lambda p: abi.set_adapter_fasta(p, FASTA), LANE_MAX, True),
    "pe_polyx_cplx": (True, lambda p: (setattr(p, "poly_x", 1), setattr(p, "complexity_filter", 1)), LANE_MAX, True),
    "pe_overlapped_out": (True, lambda p: setattr(p, "overlapped_out", 1), 0, True),
    "pe_gap": (True, lambda p: setattr(p, "allow_gap_overlap_trimming", 1), 0, True),
}

# both sides of every seq-stride step (32 bases), SWM 10 -> 16 (160 / 161), Stats form 5's column blocks (176 / 177), the lane
# plan's limit (256 / 257), long reads up to FASTP_GPU_MAX_READ_LEN
LENGTHS = [32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 176, 177, 192, 193, 224, 225, 256, 257, 400, 511, 512]
ISIZES = [0, 1, 511, 512, 1000, 2379, 4095, 4096] + [int(x) for x in np.random.default_rng(7).integers(2, 4095, size=4)]
# the lane layouts that asked for more LDS than the device has before l.ctr / l.sink were reserved ahead of the wavefronts
FORMER_OVERFLOW = [("pe_c_dedup3", L, 1000) for L in (141, 142, 143, 144)] + [("pe_c_dedup3", L, 2379) for L in (150, 151, 152)]


def _grid():
    """every family x every length, each at one insert_size_max of ISIZES (a seeded rotation), plus FORMER_OVERFLOW"""
    rng = np.random.default_rng(2024)
    pts = []
    for fam in FAMILIES:
        lens = LENGTHS + [202, 203] if fam == "pe_c_dedup3" else LENGTHS[::3] if fam.startswith("pe_c_dedup") else LENGTHS
        for L in lens:
            pts.append((fam, L, ISIZES[int(rng.integers(0, len(ISIZES)))]))
    return pts + [p for p in FORMER_OVERFLOW if p not in pts]


GRID = _grid()

# What create refuses on the grid (family -> the lengths; every insert_size_max the grid drew for them).  A change that makes
# create refuse more (or less) fails here: update the table only on purpose.
REFUSED = {
    "pe_merge": {400, 511, 512},      # (800 - 1024 cycles: no tile size fits the LDS budget)
    "pe_c_dedup3": {400, 511, 512},   # (long reads, the tile's insert-size bins and four bloom buffers: likewise)
    "pe_c_dedup4": {400},
}


def params_for(fam, L, isize):
    paired, setup, _, _ = FAMILIES[fam]
    p = abi.default_params(paired, L)
    setup(p)
    p.insert_size_max = isize
    return p


def expected_plan(fam, L):
    """the rule of fastp_gpu_create (fastp_gpu.hip, lane_plan_supported): the lane plan for reads of up to 256 bases where the
    option family has a lane form (and its duplicate hash has three byte planes); otherwise the split plan when Stats take the
    reads as they are (nothing moves or edits a kept base), else the fused plan"""
    _, _, lane_max, one_pass = FAMILIES[fam]
    if L <= lane_max:
        return "lane"
    return "split" if one_pass else "fused"


def edge_data(n, L, isize, paired, seed):
    """reads of exactly L and L - 1 bases mixed with short ones; inserts around and beyond insert_size_max (the top bin of the
    insert-size histogram: pairs that do not overlap, overlaps longer than the maximum) and beyond 2L"""
    mean = float(min(max(isize, 20), 2 * L))
    d = synth.synth_pairs(n, L=L, seed=seed, paired=paired, insert_mean=mean, insert_sd=0.6 * mean + 10, insert_min=5,
                          insert_max=max(800, 3 * L), ragged_frac=0.2, dup_frac=0.1)
    rng = np.random.default_rng(seed + 1)
    for m in ("1", "2") if paired else ("1",):
        short = rng.random(n) < 0.3
        cut = short & (d["len" + m] == L)
        d["len" + m][cut] = L - 1
        d["seq" + m][cut, L - 1] = 0
        d["qual" + m][cut, L - 1] = 0
    return d


def _args(d, paired):
    return (d["seq1"], d["qual1"], d["len1"]) + ((d["seq2"], d["qual2"], d["len2"]) if paired else ())


def compare_with_oracle(mk_engine, params, d, paired, what):
    o = oraclelib.Oracle(params)
    g = mk_engine(params)
    try:
        ro, rg = o.process(*_args(d, paired)), g.process(*_args(d, paired))
        co, cg = o.counters(), g.counters()
        plan = g.plan()
    finally:
        o.close()
        g.close()
    for k, rec in enumerate(("r1", "r2", "pair")):
        if ro[k] is not None:
            bad = np.nonzero(ro[k] != rg[k])[0]
            assert len(bad) == 0, f"{what}: {rec} differs at {bad[:5]}: oracle {ro[k][bad[:3]]} device {rg[k][bad[:3]]}"
    assert np.array_equal(np.sort(ro[3], order=["read", "pos"]), np.sort(rg[3], order=["read", "pos"])), f"{what}: corrections differ"
    bad = np.nonzero(co != cg)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} counters differ, first at {bad[:6]}"
    return plan


# ---- a. geometry sweep ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_sim_geometry_sweep(fam):
    """every grid point of the family: create succeeds (and a batch equals the oracle on the plan the rule predicts) or is
    refused cleanly with E_INVALID / E_TOO_LONG and a message - never a launch over the device's LDS"""
    refused, problems = set(), []
    for (f, L, isize) in GRID:
        if f != fam:
            continue
        paired = FAMILIES[fam][0]
        p = params_for(fam, L, isize)
        try:
            g = engines.sim_engine(p)
        except engine.EngineError as e:
            if e.code not in (abi.E_INVALID, abi.E_TOO_LONG) or not str(e).split(":", 1)[-1].strip():
                problems.append(f"L={L} isize={isize}: create failed with {e.code}: {e}")
            refused.add(L)
            continue
        g.close()
        d = edge_data(64, L, isize, paired, seed=L * 7 + isize)
        try:
            plan = compare_with_oracle(engines.sim_engine, p, d, paired, f"{fam} L={L} isize={isize}")
        except (AssertionError, engine.EngineError) as e:
            problems.append(f"L={L} isize={isize}: {e}")
            continue
        if plan != expected_plan(fam, L):
            problems.append(f"L={L} isize={isize}: plan {plan}, the rule says {expected_plan(fam, L)}")
    assert not problems, f"{fam}:\n  " + "\n  ".join(problems)
    assert refused == REFUSED.get(fam, set()), f"{fam}: create refuses lengths {sorted(refused)}, pinned {sorted(REFUSED.get(fam, set()))}"


# ---- b. parity on both sides of each threshold ------------------------------------------------------------------------------
THRESHOLDS = [
    ("pe_default", 160, 512), ("pe_default", 161, 512),          # lane SWM 10 -> 16
    ("pe_c", 160, 300), ("pe_c", 161, 300),
    ("pe_cut_front", 160, 512), ("pe_cut_front", 161, 512),
    ("se_default", 176, 512), ("se_default", 177, 512),          # Stats form 5: one column block -> several
    ("pe_default", 176, 200), ("pe_default", 177, 200),
    ("pe_c_dedup3", 202, 512), ("pe_c_dedup3", 203, 512),        # four bloom buffers: three byte planes -> four (lane -> fused)
    ("pe_default", 256, 512), ("pe_default", 257, 512),          # lane -> tile
    ("pe_umi", 256, 1), ("pe_umi", 257, 1),
    ("pe_merge", 64, 512), ("pe_merge", 65, 512),                # --merge: 2L crosses a stride (128 / 130 cycles)
    ("pe_merge", 80, 120), ("pe_merge", 81, 120),                # (160 / 162 cycles)
    ("pe_default", 150, 0), ("pe_default", 150, 4096),           # the insert-size histogram at its ends
] + FORMER_OVERFLOW
THRESHOLD_IDS = [f"{f}-{L}-{i}" for (f, L, i) in THRESHOLDS]


def check_threshold(mk_engine, fam, L, isize, n):
    paired = FAMILIES[fam][0]
    p = params_for(fam, L, isize)
    d = edge_data(n, L, isize, paired, seed=1000 + L + isize)
    plan = compare_with_oracle(mk_engine, p, d, paired, f"{fam} L={L} isize={isize}")
    assert plan == expected_plan(fam, L)


@pytest.mark.parametrize("fam,L,isize", THRESHOLDS, ids=THRESHOLD_IDS)
def test_sim_thresholds_equal_oracle(fam, L, isize):
    check_threshold(engines.sim_engine, fam, L, isize, 300)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_thresholds_equal_oracle")
@pytest.mark.parametrize("fam,L,isize", THRESHOLDS, ids=THRESHOLD_IDS)
def test_gpu_thresholds_equal_oracle(fam, L, isize):
    check_threshold(engines.gpu_engine, fam, L, isize, 3000)


# ---- c. sizing -------------------------------------------------------------------------------------------------------------
_LANE_LINE = re.compile(r"lane kernel \d+ x (\d+) threads .*LDS (\d+) bytes per workgroup")
_PLAN_LINE = re.compile(r"(lane|split|fused) plan, .*?LDS (\d+) bytes, .*stats kernel form (\d+), .*LDS (\d+) bytes")


@pytest.mark.parametrize("fam,L,isize", FORMER_OVERFLOW, ids=[f"{f}-{L}-{i}" for (f, L, i) in FORMER_OVERFLOW])
def test_sim_former_overflow_lane_lds_fits(fam, L, isize, monkeypatch, capfd):
    """the lane kernel's LDS request of the cases that used to ask for 163,888 bytes, as the geometry line prints it"""
    monkeypatch.setenv("FASTP_GPU_VERBOSE", "1")
    capfd.readouterr()
    g = engines.sim_engine(params_for(fam, L, isize))
    g.close()
    m = _LANE_LINE.search(capfd.readouterr().err)
    assert m, "no lane kernel geometry line"
    assert int(m.group(2)) <= LDS_BYTES, m.group(0)
    assert int(m.group(1)) >= 640, m.group(0)   # (one wavefront less than the layout that did not fit, not fewer)


@pytest.mark.parametrize("fam,L", [("pe_default", 150), ("se_default", 150), ("pe_cut_front", 150), ("pe_c", 150),
                                   ("pe_merge", 100), ("pe_c_dedup3", 142), ("pe_gap", 150), ("pe_default", 300)])
def test_sim_small_lds_device_equals_oracle_or_refuses(fam, L, monkeypatch, capfd):
    """a card with 64 KiB of LDS per workgroup: create sizes every layout for it (outputs equal the oracle), or refuses cleanly"""
    monkeypatch.setenv("FASTP_SIM_LDS_BYTES", str(64 * 1024))
    monkeypatch.setenv("FASTP_GPU_VERBOSE", "1")
    paired = FAMILIES[fam][0]
    p = params_for(fam, L, 512)
    try:
        engines.sim_engine(p).close()
    except engine.EngineError as e:
        assert e.code == abi.E_INVALID and "bytes of LDS" in str(e), str(e)
        return
    err = capfd.readouterr().err
    for m in _PLAN_LINE.finditer(err):
        assert int(m.group(2)) <= 64 * 1024 and int(m.group(4)) <= 64 * 1024, m.group(0)
    for m in _LANE_LINE.finditer(err):
        assert int(m.group(2)) <= 64 * 1024, m.group(0)
    compare_with_oracle(engines.sim_engine, p, edge_data(200, L, 512, paired, seed=L), paired, f"{fam} L={L} at 64 KiB")


@pytest.mark.parametrize("split", ["0", "1"])
def test_sim_lds_budget_above_the_device_is_clamped(split, monkeypatch, capfd):
    """FASTP_GPU_LDS_KB larger than the device's LDS never reaches a launch: the tile layout is sized to what the card has"""
    monkeypatch.setenv("FASTP_GPU_LDS_KB", "512")
    monkeypatch.setenv("FASTP_GPU_SPLIT", split)
    monkeypatch.setenv("FASTP_GPU_LANE", "0")
    monkeypatch.setenv("FASTP_GPU_VERBOSE", "1")
    p = params_for("pe_default", 150, 512)
    capfd.readouterr()
    engines.sim_engine(p).close()
    m = _PLAN_LINE.search(capfd.readouterr().err)
    assert m and int(m.group(2)) <= LDS_BYTES, m and m.group(0)
    compare_with_oracle(engines.sim_engine, p, edge_data(200, 150, 512, True, seed=3), True, f"FASTP_GPU_LDS_KB=512 split={split}")


def test_sim_launch_over_the_lds_limit_fails_with_a_message(monkeypatch):
    """the emulator's limit itself: a tile size asked for that cannot fit 16 KiB fails as an error of the engine, not an abort"""
    monkeypatch.setenv("FASTP_SIM_LDS_BYTES", str(16 * 1024))
    with pytest.raises(engine.EngineError) as ei:
        engines.sim_engine(params_for("pe_default", 150, 512))
    assert ei.value.code in (abi.E_INVALID, abi.E_HIP) and "LDS" in str(ei.value), str(ei.value)
