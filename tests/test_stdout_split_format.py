"""--stdout's interleaved stream and --split's pack table at the formatter (fastp_gpu_format_interleaved,
fastp_gpu_format_pack_cuts, both through fastp_gpu_format_all_streams) against the host writer
(fastp_amd.hostloop.apply_results).  The CPU suite runs the product sources on the SIMT emulator; every `-m gpu` test names
its emulator twin."""
import os

import numpy as np
import pytest

import engines
import format7_util as f7
import format_util
import outstream_util as ou
from fastp_amd import abi

# option set -> (--failed_out, --unpaired1, --unpaired2) given
INTERLEAVED_SETS = {
    "pe_default": (False, False, False),
    "pe_filters": (True, True, False),
    "pe_noadapter_dedup": (True, False, False),
    "pe_umi_per_read": (False, False, False),
    "pe_correction": (True, True, True),
}
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, 513]   # FMT_BLOCK is 256, a wave 64 lanes, a copy group 16 lanes
PACK_SIZES = [1000, 64, 7]
FIRST_UNITS = [0, 999, 1000, 1001, 123456789]
TABLE_SIZES = [0, 1, 255, 256, 257, 1000, 1001, 2049]


# ---- B1: the interleaved stream ------------------------------------------------------------------------------------
def _interleaved(mk_engine, mem, set_name, n):
    wf, u1, u2 = INTERLEAVED_SETS[set_name]
    params, fq1, fq2, umi = f7.inputs(set_name, n)
    want = ou.host_writer(mk_engine, params, fq1, fq2, 150, wf, u1, u2, umi)
    g = mk_engine(params)
    try:
        prep = ou.Prepared(g, mem, fq1, fq2, 150, umi)
        assert g.format_interleaved(True) == 0
        rc, got, lens = prep.format(wf, u1, u2, null_out2=(n == 65))   # (out2 needs no buffer in this mode)
        assert rc == 0
        both = ou.interleave(want["out1"], want["out2"])
        assert got["out1"] == both and lens[0] == len(both)
        assert got["out2"] == b"" and lens[1] == 0
        for k in ou.STREAMS[2:]:
            assert got[k] == want[k], f"{set_name}: stream {k} differs ({len(got[k])} vs {len(want[k])} bytes)"
        # ... and off again: the two streams of the parent
        assert g.format_interleaved(False) == 0
        rc, got, lens = prep.format(wf, u1, u2)
        assert rc == 0 and got["out1"] == want["out1"] and got["out2"] == want["out2"]
    finally:
        g.close()
    return want


def _b1(mk_engine, mem, set_name):
    want = _interleaved(mk_engine, mem, set_name, 600)
    pairs = len(ou.records(want["out1"]))
    print(f"{set_name}: {pairs} of 600 pairs in out1")
    assert 50 <= pairs                       # (the EXPECTED stream: a pass must not be vacuous)
    if set_name in ("pe_filters", "pe_noadapter_dedup"):
        assert pairs < 600                   # units that emit nothing into out1 lie between the ones that do
    if set_name == "pe_filters":
        assert len(want["failed"]) > 0 and len(want["unpaired1"]) > 0
    if set_name == "pe_umi_per_read":
        import re
        assert all(re.match(rb"@\S+:[ACGTN]{0,6}_[ACGTN]{0,6} ", r) for r in ou.records(want["out1"])[:20])


@pytest.mark.parametrize("set_name", list(INTERLEAVED_SETS))
def test_sim_interleaved_out1_equals_host_writer(set_name):
    _b1(engines.sim_engine, format_util.NumpyMem(), set_name)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sim_interleaved_out1_at_block_and_wave_edges(n):
    _interleaved(engines.sim_engine, format_util.NumpyMem(), "pe_filters", n)


def test_sim_interleaved_refused_on_single_end_and_merge():
    for name in ("se_adapter_cut", "pe_merge"):
        params = f7.inputs(name, 8)[0]
        g = engines.sim_engine(params)
        assert g.format_interleaved(True, check=False) == abi.E_INVALID
        assert g.format_interleaved(False, check=False) == abi.E_INVALID
        g.close()


# ---- B2: the pack table --------------------------------------------------------------------------------------------
def _table_case(mk_engine, mem, paired, n):
    """every (pack_size, first_unit) on one prepared batch of n units; the last plan with the interleaved stream"""
    set_name = "pe_filters" if paired else "se_polyx_complexity"
    params, fq1, fq2, umi = f7.inputs(set_name, max(n, 1))
    wf = True
    want = ou.host_writer(mk_engine, params, fq1, fq2, 150, wf, False, False, umi)
    if n == 0:
        want = {k: b"" for k in want}
    g = mk_engine(params)
    try:
        prep = ou.Prepared(g, mem, fq1, fq2, 150, umi)
        for pack_size in PACK_SIZES:
            for first in FIRST_UNITS:
                slices = 0 if n == 0 else (first + n - 1) // pack_size - first // pack_size + 1
                tab = ou.PackTable(mem, max(slices, 1) + 2)
                assert g.format_pack_cuts(tab.plan(first, pack_size)) == 0
                rc, got, lens = prep.format(wf, n=n)
                assert rc == 0
                for k in ou.STREAMS:
                    assert got[k] == want[k], f"stream {k} differs with a plan armed"
                cut, passed, behind = tab.read()
                ecut, epassed = ou.expected_table(want["out1"], want["out2"], n, first, pack_size)
                assert ecut.shape[1] == slices + 1
                where = f"paired={paired} n={n} pack_size={pack_size} first_unit={first}"
                assert np.array_equal(cut[:, :slices + 1].astype(np.int64), ecut), where
                assert np.array_equal(passed[:slices].astype(np.int64), epassed), where
                assert int(ecut[0, -1]) == lens[0] and int(ecut[1, -1]) == lens[1]
                # nothing behind the entries
                mark = np.uint8(ou.PackTable.MARK)
                assert (cut[:, slices + 1:].view(np.uint8) == mark).all() and (passed[slices:].view(np.uint8) == mark).all(), where
                assert behind == bytes([ou.PackTable.MARK]) * len(behind), where
                if n >= 1000 and pack_size == 1000 and first == 0:
                    assert slices == (n + 999) // 1000 and 0 < epassed[0] < 1000     # (a pack with passed < units)
        # a plan arms ONE call: the next one leaves the arrays alone; so does a call after the plan was taken back
        tab = ou.PackTable(mem, 8)
        rc, got, lens = prep.format(wf, n=n)
        assert rc == 0
        assert g.format_pack_cuts(tab.plan(0, 1000)) == 0
        assert g.format_pack_cuts(None) == 0
        rc, got, lens = prep.format(wf, n=n)
        assert rc == 0 and got["out1"] == want["out1"]
        cut, passed, behind = tab.read()
        assert (cut.view(np.uint8) == ou.PackTable.MARK).all() and (passed.view(np.uint8) == ou.PackTable.MARK).all()
        if paired and n > 0:   # the table of the interleaved stream: out2's offsets stay 0
            tab = ou.PackTable(mem, 64)
            assert g.format_interleaved(True) == 0
            assert g.format_pack_cuts(tab.plan(1001, 64)) == 0
            rc, got, lens = prep.format(wf, n=n)
            both = ou.interleave(want["out1"], want["out2"])
            assert rc == 0 and got["out1"] == both
            cut, passed, _ = tab.read()
            ecut, epassed = ou.expected_table(both, b"", n, 1001, 64)
            s = len(epassed)
            assert np.array_equal(cut[:, :s + 1].astype(np.int64), ecut) and np.array_equal(passed[:s].astype(np.int64), epassed)
        # too few entries: refused before anything is formatted
        if n > 7:
            tab = ou.PackTable(mem, 1)
            assert g.format_pack_cuts(tab.plan(0, 7)) == 0
            rc, got, lens = prep.format(wf, n=n)
            assert rc == abi.E_INVALID and sum(lens) == 0
    finally:
        g.close()


@pytest.mark.parametrize("n", TABLE_SIZES)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_sim_pack_table_equals_host_writer(paired, n):
    _table_case(engines.sim_engine, format_util.NumpyMem(), paired, n)


def test_sim_pack_cuts_rejects_bad_plans():
    params = f7.inputs("pe_default", 8)[0]
    g = engines.sim_engine(params)
    mem = format_util.NumpyMem()
    tab = ou.PackTable(mem, 4)
    for first, size, packs, cut, passed in ((-1, 1000, 4, True, True), (0, 0, 4, True, True), (0, 1000, 0, True, True),
                                            (0, 1000, 4, False, True), (0, 1000, 4, True, False)):
        p = tab.plan(first, size)
        p.max_packs = packs
        if not cut:
            p.cut = None
        if not passed:
            p.passed = None
        assert g.format_pack_cuts(p, check=False) == abi.E_INVALID
    g.close()


# ---- B3: a context that never arms a plan launches what the parent launched ---------------------------------------
def test_sim_unarmed_format_call_launches_the_parents_kernels(tmp_path):
    """the three kernels of fastp_gpu_format_all_streams with the parent's grids and LDS sizes and no memset; an armed
    call adds one memset (the counts) and no launch"""
    params, fq1, fq2, umi = f7.inputs("pe_filters", 600)   # (no -c: no correction kernel)
    g = engines.sim_engine(params)
    mem = format_util.NumpyMem()
    prep = ou.Prepared(g, mem, fq1, fq2, 150, umi)
    tab = ou.PackTable(mem, 4)

    def traced(arm):
        path = str(tmp_path / ("armed.txt" if arm else "plain.txt"))
        if arm:
            g.format_pack_cuts(tab.plan(0, 1000))
        os.environ["FASTP_SIM_TRACE"] = path
        try:
            rc, got, lens = prep.format(True)
        finally:
            del os.environ["FASTP_SIM_TRACE"]
        assert rc == 0
        lines = [ln.rsplit(" ", 1)[0] for ln in open(path).read().splitlines()]
        return [ln for ln in lines if ln.startswith(("launch", "memset"))], got

    nb = (600 + 255) // 256
    kernels = [f"launch fq_fmts7_len_kernel grid={nb} block=256 lds={7 * 4}",
               "launch fq_fmts_scan_kernel grid=7 block=1024 lds=8192",
               f"launch fq_fmts7_write_kernel grid={nb} block=256 lds={7 * 16 * 4 + 256 * 3 * 8}"]
    plain, got_plain = traced(False)
    armed, got_armed = traced(True)
    g.close()
    assert plain == kernels
    assert armed == ["memset value=0 bytes=4"] + kernels
    assert got_plain == got_armed


# ---- -m gpu -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.twin("test_sim_interleaved_out1_equals_host_writer")
@pytest.mark.parametrize("set_name", list(INTERLEAVED_SETS))
def test_gpu_interleaved_out1_equals_host_writer(set_name):
    _b1(engines.gpu_engine, format_util.TorchMem(), set_name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_interleaved_out1_at_block_and_wave_edges")
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_gpu_interleaved_out1_at_block_and_wave_edges(n):
    _interleaved(engines.gpu_engine, format_util.TorchMem(), "pe_filters", n)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_pack_table_equals_host_writer")
@pytest.mark.parametrize("n", TABLE_SIZES)
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_gpu_pack_table_equals_host_writer(paired, n):
    _table_case(engines.gpu_engine, format_util.TorchMem(), paired, n)
