"""The text kernel (fastp_amd/csrc/fq_text.h: one wavefront per unit, every step of the worker loop evaluated across the lanes in
blocks of 64 positions or candidates) on hand-built units whose events fall on steps 63 / 64 / 65 and 127 / 128 / 129 of each scan,
or whose state must survive from an earlier block (tests/text_util.py builds them and says what each is built for).

Every family goes through four routes, compared record by record (read and pair records, the sorted correction list, every
counter, the --adapter_fasta events) as tests/test_option_fuzz.py does:
  1. the oracle (plain-C literal loops) - after the check that it reaches every unit's stated outcome;
  2. the device with no switch: the plan's own kernels (the lane kernel's 16-base words and 32-base windows meet the same positions);
  3. FASTP_GPU_EXACT=1: the text kernel on every unit;
  4. the production route: a "soft" variant (lower case, IUPAC letters or '.' across the family's edge position in every third
     unit) lists only those units for the text kernel, the plan's kernels see them as empty reads, the ghost pass takes back what
     they counted for them.
On the emulator here; the GPU twins carry the same parameter ids.  The oracle itself is pinned on these inputs against the real
reference binary by the fixtures of tests/golden/text_edges/ (make_fixtures.py there)."""
import json
import os

import numpy as np
import pytest

import driver
import engines
import golden_util
import oraclelib
import text_util as tu
from fastp_amd import abi, hostloop

FIXTURES = os.path.join(golden_util.GOLDEN_DIR, "text_edges")
NAMES = list(tu.FAMILIES)
_ORACLE = {}


def run(eng, args):
    """(records, counters, adapter events) of one process() call; the engine is closed"""
    res = eng.process(*args)
    out = (res, eng.counters(), getattr(eng, "last_adapter_events", None))
    eng.close()
    return out


def oracle_of(name):
    """the oracle's result for a family: computed once, shared, never written to"""
    if name not in _ORACLE:
        fam = tu.family(name)
        _ORACLE[name] = run(oraclelib.Oracle(fam.params), fam.args())
        for a in _ORACLE[name][0] + (_ORACLE[name][1],):
            if a is not None:
                a.setflags(write=False)
    return _ORACLE[name]


def same(what, want, got, need_events=False):
    (ro, co, evo), (rg, cg, evg) = want, got
    for k, rec in enumerate(("read 1 records", "read 2 records", "pair records")):
        if ro[k] is not None:
            bad = np.nonzero(ro[k] != rg[k])[0]
            assert len(bad) == 0, f"{what}: {rec} differ at units {bad[:5]}: oracle {ro[k][bad[:3]]} device {rg[k][bad[:3]]}"
    assert np.array_equal(np.sort(ro[3], order=["read", "pos"]), np.sort(rg[3], order=["read", "pos"])), f"{what}: corrections differ"
    bad = np.nonzero(co != cg)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} counters differ, first at {bad[:6]}: oracle {co[bad[:6]]} device {cg[bad[:6]]}"
    if need_events:   # --adapter_fasta: both sides must have reported their events, an absent list is no agreement
        assert evo is not None and evg is not None, f"{what}: no adapter events came back"
    if evo is not None and evg is not None:
        assert np.array_equal(evo, evg), f"{what}: adapter events differ"


def soft_units(fam):
    return list(range(1, fam.n, 3))


def check_reached(name):
    fam = tu.family(name)
    res, ctr, ev = oracle_of(name)
    miss = tu.reached(fam, res, ev)
    assert not miss, f"{name}: {len(miss)} units do not reach what they were built for in the oracle: {miss[:4]}"
    if fam.counters:
        lay = oraclelib.layout_for_params(fam.params)
        assert not fam.counters(ctr, lay)


def routes(mk_engine, name, monkeypatch):
    fam = tu.family(name)
    check_reached(name)
    want = oracle_of(name)
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    g = mk_engine(fam.params)
    assert g.plan() == tu.PLAN[name], f"{name}: built for the {tu.PLAN[name]} plan, the context chose {g.plan()}"
    ev = bool(fam.params.n_adapter_fasta)
    same(f"{name}, the plan's own kernels", want, run(g, fam.args()), ev)
    monkeypatch.setenv("FASTP_GPU_EXACT", "1")
    same(f"{name}, the text kernel on every unit", want, run(mk_engine(fam.params), fam.args()), ev)
    monkeypatch.delenv("FASTP_GPU_EXACT")
    d = tu.soften(fam, soft_units(fam), "mixed")
    assert set(soft_units(fam)) - {u for u in soft_units(fam) if max(d["len1"][u], d["len2"][u] if fam.paired else 0) == 0} <= set(tu.listed(fam, d))
    same(f"{name}, soft units through the text kernel", run(oraclelib.Oracle(fam.params), fam.args(d)), run(mk_engine(fam.params), fam.args(d)), ev)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reaches_every_edge(name):
    """a cap, not a tolerance: no unit is exempt (text_util.py lists the constructions that cannot exist)"""
    check_reached(name)


@pytest.mark.parametrize("name", NAMES)
def test_sim_routes_equal_oracle(name, monkeypatch):
    routes(engines.sim_engine, name, monkeypatch)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_routes_equal_oracle")
@pytest.mark.parametrize("name", NAMES)
def test_gpu_routes_equal_oracle(name, monkeypatch):
    routes(engines.gpu_engine, name, monkeypatch)


# ---- the sparse route's geometry: 1, 7, 8, 9 listed units (TEXT_WAVES = 8 wavefronts per workgroup), and more than 8 x CUs, so
# that a wavefront's `i += nw` loop makes a second trip ----
def _cus(gpu):
    if not gpu:
        return int(os.environ.get("FASTP_SIM_CUS", "3"))   # tests/hostsim/sim.cpp
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def sparse_count(mk_engine, name, count, gpu, trace=None, monkeypatch=None):
    fam = tu.family(name)
    assert len(tu.listed(fam, fam.d)) == 0, "a family without foreign letters of its own: the count is exact"
    cus = _cus(gpu)
    k = tu.TEXT_WAVES * cus + 3 if count == "above_8_per_cu" else int(count)
    tiled = fam.tiled(max(2, -(-2 * k // fam.n)))
    nonempty = np.flatnonzero(tiled.d["len1"] > 0)
    units = [int(u) for u in nonempty[np.linspace(0, len(nonempty) - 1, k).astype(int)]]
    assert len(set(units)) == k
    d = tu.soften(tiled, units, "mixed")
    assert len(tu.listed(tiled, d)) == k
    want = run(oraclelib.Oracle(fam.params), tiled.args(d))
    g = mk_engine(fam.params)
    if trace is not None:
        monkeypatch.setenv("FASTP_SIM_TRACE", str(trace))
    got = run(g, tiled.args(d))
    same(f"{name}, {k} listed units", want, got)
    if trace is not None:   # one launch takes every listed unit, on at most one workgroup per CU: above 8 x CUs a wavefront's loop goes round again
        monkeypatch.delenv("FASTP_SIM_TRACE")
        lines = [x for x in trace.read_text().splitlines() if x.startswith("launch fq_text_kernel")]
        want_grid = min(-(-k // tu.TEXT_WAVES), cus)
        assert len(lines) == 1 and f" grid={want_grid} block={64 * tu.TEXT_WAVES} " in lines[0], (k, lines)
        assert (k > tu.TEXT_WAVES * want_grid) == (count == "above_8_per_cu")


COUNTS = ["1", "7", "8", "9", "above_8_per_cu"]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", ["poly_g_136", "cut_tail_w4_ft"])
def test_sim_sparse_listed_unit_counts(name, count, monkeypatch, tmp_path):
    """(the GPU twin has no trace: there the grid's cap at one workgroup per CU is launch_text's, read in the source)"""
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    sparse_count(engines.sim_engine, name, count, False, tmp_path / "trace.txt", monkeypatch)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_sparse_listed_unit_counts")
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", ["poly_g_136", "cut_tail_w4_ft"])
def test_gpu_sparse_listed_unit_counts(name, count, monkeypatch):
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    sparse_count(engines.gpu_engine, name, count, True)


# ---- three process() calls on one engine, listed units only in the first and the last: the counters of one call ----
def three_calls(mk_engine, name):
    fam = tu.family(name)
    native = set(tu.listed(fam, fam.d))   # (units that hold foreign letters as built: the middle call avoids them)
    w = fam.n // 4
    a = next(a for a in range(w, fam.n - w) if not native & set(range(a, a + w)))
    cut = [0, a, a + w, fam.n]
    units = [u for u in soft_units(fam) if not cut[1] <= u < cut[2]]
    d = tu.soften(fam, units, "mixed")
    listed = tu.listed(fam, d)
    assert not any(cut[1] <= u < cut[2] for u in listed) and any(u < cut[1] for u in listed) and any(u >= cut[2] for u in listed)
    whole = run(mk_engine(fam.params), fam.args(d))
    same(f"{name}, one call", run(oraclelib.Oracle(fam.params), fam.args(d)), whole)
    g = mk_engine(fam.params)
    parts = [g.process(*(a[cut[k]:cut[k + 1]] for a in fam.args(d))) for k in range(3)]
    ctr = g.counters()
    g.close()
    assert np.array_equal(ctr, whole[1]), f"{name}: {int((ctr != whole[1]).sum())} counters of three calls differ from one call's"
    for k in range(3 if fam.paired else 1):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[0][k])


@pytest.mark.parametrize("name", ["analyze_136", "poly_g_136"])
def test_sim_three_calls_count_like_one(name, monkeypatch):
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    three_calls(engines.sim_engine, name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_three_calls_count_like_one")
@pytest.mark.parametrize("name", ["analyze_136", "poly_g_136"])
def test_gpu_three_calls_count_like_one(name, monkeypatch):
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    three_calls(engines.gpu_engine, name)


# ---- FASTQ text -> fastp_gpu_parse_fastq -> fastp_gpu_submit_device: the listed units' text comes through the parser's line
# table (TextArgs::x_dense) instead of an offset list ----
def parsed_route(mk_engine, mem, name):
    import format7_util
    fam = tu.family(name)
    d = tu.soften(fam, soft_units(fam), "mixed")
    want = run(mk_engine(fam.params), fam.args(d))
    same(f"{name}, host-packed", run(oraclelib.Oracle(fam.params), fam.args(d)), want)
    fq1, fq2 = tu.fastq(fam, d)
    g = mk_engine(fam.params)
    c = format7_util.prepare(g, mem, fq1, fq2, fam.L)
    assert c["n"] == fam.n and c["n_exotic"] == len(tu.listed(fam, d))
    r1 = np.frombuffer(mem.download(c["res"][0], fam.n * 12), dtype=abi.READ_RESULT_DTYPE)
    assert np.array_equal(r1, want[0][0]), f"{name}: read 1 records of the parsed route differ from the host-packed route's"
    if fam.paired:
        assert np.array_equal(np.frombuffer(mem.download(c["res"][1], fam.n * 12), dtype=abi.READ_RESULT_DTYPE), want[0][1])
        assert np.array_equal(np.frombuffer(mem.download(c["pair"], fam.n * 8), dtype=abi.PAIR_RESULT_DTYPE), want[0][2])
    ctr = g.counters()
    g.close()
    assert np.array_equal(ctr, want[1]), f"{name}: {int((ctr != want[1]).sum())} counters of the parsed route differ"


@pytest.mark.parametrize("name", ["analyze_136", "cut_front_w4"])
def test_sim_soft_family_through_the_device_parser(name, monkeypatch):
    import format_util
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    parsed_route(engines.sim_engine, format_util.NumpyMem(), name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_soft_family_through_the_device_parser")
@pytest.mark.parametrize("name", ["analyze_136", "cut_front_w4"])
def test_gpu_soft_family_through_the_device_parser(name, monkeypatch):
    import format_util
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    parsed_route(engines.gpu_engine, format_util.TorchMem(0), name)


# ---- Stats' tables in LDS, and the global-atomic path of t_stat_read.  launch_text decides by read length alone (its inequality,
# text_util.text_tables_in_lds: FASTP_GPU_LDS_KB sizes the tile kernels and does not enter it), so the path is chosen by max_len:
# --merge at 136 bases keeps the tables in LDS, at 200 bases (400 cycles, three tables) they no longer fit 150 KiB ----
def test_sim_stats_tables_in_lds_and_global_atomics(tmp_path, monkeypatch):
    """the launch trace shows the kernel's dynamic LDS: the text buffers alone on the global-atomic path.  (The GPU twin of
    these families runs in test_gpu_routes_equal_oracle; the path is not asserted there, no trace exists on the device.)"""
    monkeypatch.delenv("FASTP_GPU_EXACT", raising=False)
    for name, in_lds in (("correct_merge_136", True), ("correct_merge_200_global_atomics", False)):
        fam = tu.family(name)
        fits, lds = tu.text_tables_in_lds(fam.params)
        assert fits == in_lds
        trace = tmp_path / (name + ".txt")
        g = engines.sim_engine(fam.params)
        monkeypatch.setenv("FASTP_SIM_TRACE", str(trace))
        got = run(g, fam.args())
        monkeypatch.delenv("FASTP_SIM_TRACE")
        same(name, oracle_of(name), got)
        lines = [x for x in trace.read_text().splitlines() if x.startswith("launch fq_text_kernel")]
        assert lines and all(f" lds={lds} " in x + " " for x in lines), (lds, lines)


# ---- the oracle on these inputs against the real reference binary (fixtures: tests/golden/text_edges/make_fixtures.py) ----
@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_hand_built_units(name):
    fam = tu.family(name)
    z = np.load(os.path.join(FIXTURES, name + ".npz"))
    meta = json.loads(z["meta"].tobytes().decode())
    fq1, fq2 = tu.fastq(fam)
    assert z["fq1"].tobytes() == fq1 and (fq2 is None or z["fq2"].tobytes() == fq2), f"{name}: the fixture is of other input: run make_fixtures.py"
    assert meta["flags"] == fam.flags
    eng = oraclelib.Oracle(fam.params)
    try:
        outs, ctr, rep = driver.run_engine(eng, fam.params, fq1, fq2, stride=(fam.L + 7) // 8 * 8,
                                           umi=hostloop.UmiNameEditor(*fam.umi) if fam.umi else None)
    finally:
        eng.close()
    golden_util.check_against_golden(name, outs, rep, meta)
