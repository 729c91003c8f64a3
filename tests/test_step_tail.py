"""The end of a step on the device: the Stats fold of a launch with more than one slab group is the wide fold
(fq_reduce_wide_kernel), and Duplicate's finish kernel runs as the largest workgroup that fits the registers the
context's Stats kernel leaves per SIMD (512 in granules of 8; a 256-lane workgroup is a wave per SIMD), so that it runs
beside that kernel - 1024 lanes where nothing fits.  Whole steps against the oracle, and the choice itself as a condition
on the build (fastp_gpu_debug_kernel_regs, fastp_gpu_debug_stats_fold)."""
import numpy as np
import pytest

import engines
import oraclelib
import synth
from fastp_amd import abi

pytestmark = pytest.mark.gpu

FRONT_TRIM = {"trim_front1": 5, "trim_front2": 5}   # form 5's 128-VGPR instantiation: nothing fits beside it


def _params(opts=None):
    p = abi.default_params(True, 150)
    p.cut_right = 1
    for k, v in (opts or {}).items():
        setattr(p, k, v)
    return p


def _args(d):
    return (d["seq1"], d["qual1"], d["len1"], d["seq2"], d["qual2"], d["len2"])


def _step(p, d):
    g, o = engines.gpu_engine(p), oraclelib.Oracle(p)
    try:
        rg, ro = g.process(*_args(d)), o.process(*_args(d))
        cg, co = g.counters(), o.counters()
        info = g.debug_stats_fold()
        lay = g.layout
    finally:
        g.close()
        o.close()
    return rg, ro, cg, co, info, lay


def _ceil8(r):
    return (r + 7) // 8 * 8


def _expected_finish_threads(regs):
    """the largest of 1024 / 512 / 256 lanes whose waves fit beside the Stats kernel's four per SIMD; 1024 if none does"""
    left = 512 - 4 * _ceil8(regs["stats"]["vgprs"])
    for t in (1024, 512, 256):
        if (t // 256) * _ceil8(regs["fq_dup_finish_kernel"]["vgprs"]) <= left:
            return t
    return 1024


def test_a_launch_with_many_stats_slabs_takes_the_wide_fold():
    """16,384 + 37 pairs of 100 bases: more than 64 Stats workgroups, a last one that is not full"""
    p = _params()
    d = synth.synth_pairs(16384 + 37, L=100, seed=707, insert_mean=140.0, insert_sd=40.0)
    rg, ro, cg, co, info, _ = _step(p, d)
    assert info["last_stats_fold"] == "wide", info
    for k, what in enumerate(("read1 results", "read2 results", "pair results")):
        assert rg[k].tobytes() == ro[k].tobytes(), f"{what} differ from the oracle"
    bad = np.nonzero(cg != co)[0]
    assert len(bad) == 0, f"{len(bad)} counters differ, first at {bad[:8]}: oracle {co[bad[:8]]} gpu {cg[bad[:8]]}"


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("ctx_name", ["default", "front_trim"])
def test_duplicate_heavy_batches_equal_the_oracle(ctx_name, n):
    """every pair three times, shuffled; n at the workgroup edges of both finish sizes (the default context's and the
    front-trim context's 1024)"""
    p = _params(FRONT_TRIM if ctx_name == "front_trim" else None)
    d = synth.synth_pairs((n + 2) // 3, L=100, seed=900 + n, insert_mean=140.0, insert_sd=40.0, dup_frac=0.0)
    order = np.random.default_rng(n).permutation(np.tile(np.arange((n + 2) // 3), 3)[:n])
    d = {k: np.ascontiguousarray(v[order]) for k, v in d.items()}
    rg, ro, cg, co, _, lay = _step(p, d)
    dups = int((ro[0]["flags"] & abi.RF_DUP != 0).sum())
    assert dups >= n // 2, dups
    for k, what in enumerate(("read1 results", "read2 results", "pair results")):
        assert rg[k].tobytes() == ro[k].tobytes(), f"{ctx_name}, n = {n}: {what} differ from the oracle"
    assert cg[lay.dup_total] == co[lay.dup_total] == n
    assert cg[lay.dup_count] == co[lay.dup_count] == dups
    assert np.array_equal(cg, co)


def test_default_options_run_finish_as_256_lanes():
    """beside the default options' Stats kernel (four waves per SIMD) one wave of finish per SIMD fits and two do not -
    a condition on the build, not a measurement"""
    g = engines.gpu_engine(_params())
    try:
        regs, info = g.debug_kernel_regs(), g.debug_stats_fold()
    finally:
        g.close()
    stats, fin = regs["stats"]["vgprs"], regs["fq_dup_finish_kernel"]["vgprs"]
    assert stats > 0 and fin > 0
    assert 4 * _ceil8(stats) + _ceil8(fin) <= 512 < 4 * _ceil8(stats) + 2 * _ceil8(fin), f"finish {fin} VGPRs beside 4 x {stats}"
    assert info["finish_threads"] == _expected_finish_threads(regs) == 256, info


def test_a_single_end_context_keeps_finish_at_1024_lanes():
    """single-end: the Stats kernel ends before Duplicate's chain does, finish runs alone on the chip and the large
    workgroup is the faster one there - whatever fits, 1024 stays; a duplicate-heavy batch through it equals the oracle"""
    p = abi.default_params(False, 150)
    p.cut_right = 1
    p.adapter_seq_r1 = None
    g = engines.gpu_engine(p)
    try:
        regs, info = g.debug_kernel_regs(), g.debug_stats_fold()
    finally:
        g.close()
    assert regs["stats"]["vgprs"] > 0
    assert info["finish_threads"] == 1024, (info, _expected_finish_threads(regs))
    n = 1025
    d = synth.synth_pairs((n + 2) // 3, L=100, seed=77, insert_mean=140.0, insert_sd=40.0, dup_frac=0.0, paired=False)
    order = np.random.default_rng(n).permutation(np.tile(np.arange((n + 2) // 3), 3)[:n])
    d = {k: np.ascontiguousarray(v[order]) for k, v in d.items()}
    o = oraclelib.Oracle(p)
    g = engines.gpu_engine(p)
    try:
        rg, ro = g.process(d["seq1"], d["qual1"], d["len1"]), o.process(d["seq1"], d["qual1"], d["len1"])
        cg, co = g.counters(), o.counters()
    finally:
        g.close()
        o.close()
    assert int((ro[0]["flags"] & abi.RF_DUP != 0).sum()) >= n // 2
    assert rg[0].tobytes() == ro[0].tobytes()
    assert np.array_equal(cg, co)


def test_a_front_trim_context_keeps_finish_at_1024_lanes():
    g = engines.gpu_engine(_params(FRONT_TRIM))
    try:
        regs, info = g.debug_kernel_regs(), g.debug_stats_fold()
    finally:
        g.close()
    stats, fin = regs["stats"]["vgprs"], regs["fq_dup_finish_kernel"]["vgprs"]
    assert stats > 0 and fin > 0
    assert 4 * _ceil8(stats) + _ceil8(fin) > 512, f"a wave of finish ({fin} VGPRs) fits beside 4 x {stats}: not the 128-VGPR instantiation"
    assert info["finish_threads"] == _expected_finish_threads(regs) == 1024, info
