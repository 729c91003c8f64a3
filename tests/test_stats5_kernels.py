"""Form 5 of the Stats kernel is a kernel per instantiation of stats_body5, picked on the host (stats5_inst_for in
fastp_gpu.hip).  One small batch through every instantiation a context can select on a 160 KB-LDS device: the intended
instantiation ran (fastp_gpu_debug_kernel_regs), counters and records equal the oracle's bit for bit.  And the
arithmetic that the split exists for: beside the default options' Stats kernel a wave of the tail stream's small
kernels fits the register file.

Which read length selects what follows stats5_copies (the table's columns Hs = the reads' 16-base columns H16, in as few
blocks as fit the LDS, with two copies of the 5-mer table where they fit) and stats5_inst_for:
    max_len 145..160   H16 = Hs = 10, two copies         ONE (+ NF without a front trim)
    max_len 113..128   H16 = Hs = 8, one block           the eight-column table
    max_len 225..256   H16 = 15 / 16 as two blocks of 8  the eight-column table, column blocks
    max_len 177..192   H16 = 12 as two blocks of 6       the general form, column blocks
    max_len <= 112     H16 = Hs <= 7                     the general form
    max_len 161..176   H16 = Hs = 11, one copy           the general form with one 5-mer copy
(ten columns in blocks - Hs = 10 under H16 = 19 / 20 - leave room for one 5-mer copy only in 160 KB: that instantiation
is selected on no device the engine runs on, and has no case here.)"""
import numpy as np
import pytest

import engines
import oraclelib
import synth
from fastp_amd import abi

pytestmark = pytest.mark.gpu

PAIRS = 300
ONE_NF, ONE, BLOCKS10, BLOCKS8, ANY_KC2, ANY_KC1 = range(6)

# name: (paired, max_len, read length, options, the instantiation stats5_inst_for picks)
CASES = {
    "default_one_nf": (True, 150, 100, {}, ONE_NF),
    "trim_front_one": (True, 150, 100, {"trim_front1": 5, "trim_front2": 5}, ONE),
    "cut_front_one": (True, 150, 100, {"cut_front": 1}, ONE),
    "eight_columns": (True, 128, 100, {}, BLOCKS8),
    "eight_columns_two_blocks": (True, 225, 225, {}, BLOCKS8),
    "general": (True, 100, 100, {}, ANY_KC2),
    "general_two_blocks": (True, 177, 177, {}, ANY_KC2),
    "general_one_kmer_copy": (True, 161, 161, {}, ANY_KC1),
    "single_end_one_nf": (False, 150, 100, {}, ONE_NF),   # the second mate's pass only flushes (m >= nm)
}


def _params(paired, max_len, opts):
    p = abi.default_params(paired, max_len)
    p.cut_right = 1
    if not paired:
        p.adapter_seq_r1 = None
    for k, v in opts.items():
        setattr(p, k, v)
    return p


def _args(d, paired):
    return (d["seq1"], d["qual1"], d["len1"]) + ((d["seq2"], d["qual2"], d["len2"]) if paired else ())


def check_case(name, make_engine):
    paired, max_len, L, opts, inst = CASES[name]
    p = _params(paired, max_len, opts)
    d = synth.synth_pairs(PAIRS, L=L, seed=505, insert_mean=1.4 * L, insert_sd=0.4 * L, paired=paired)
    g = make_engine(p)
    o = oraclelib.Oracle(p)
    try:
        regs = g.debug_kernel_regs()
        assert regs["stats_inst"] == inst, f"{name}: instantiation {regs['stats_inst']} selected, {inst} intended"
        rg, ro = g.process(*_args(d, paired)), o.process(*_args(d, paired))
        cg, co = g.counters(), o.counters()
    finally:
        g.close()
        o.close()
    for k, what in enumerate(("read1 results", "read2 results", "pair results")):
        if ro[k] is not None:
            assert rg[k].tobytes() == ro[k].tobytes(), f"{name}: {what} differ from the oracle"
    bad = np.nonzero(cg != co)[0]
    assert len(bad) == 0, f"{name}: {len(bad)} counters differ, first at {bad[:8]}: oracle {co[bad[:8]]} gpu {cg[bad[:8]]}"
    return regs


@pytest.mark.parametrize("name", list(CASES))
def test_instantiation_runs_and_equals_oracle(name):
    regs = check_case(name, engines.gpu_engine)
    st = regs["stats"]
    assert st["max_threads"] == 1024 and 0 < st["vgprs"] <= 128, f"{name}: {st}"   # sixteen waves of it fit a CU


def _ceil8(r):
    return (r + 7) // 8 * 8


def test_a_tail_wave_fits_beside_the_default_stats_kernel():
    """four waves of the Stats kernel per SIMD (a 1024-lane workgroup per CU) + one wave of a tail kernel within the
    512 registers of a SIMD, allocated in granules of 8 - a condition on the build, not a measurement"""
    g = engines.gpu_engine(_params(True, 150, {}))
    try:
        regs = g.debug_kernel_regs()
    finally:
        g.close()
    assert regs["stats_inst"] == ONE_NF
    stats = regs["stats"]["vgprs"]
    assert stats > 0
    for k in ("fq_reduce_kernel", "fq_dup_losers_kernel", "fq_dup_winners_kernel"):
        r = regs[k]["vgprs"]
        assert r > 0
        assert 4 * _ceil8(stats) + _ceil8(r) <= 512, f"{k}: {r} VGPRs beside 4 x {stats}"
