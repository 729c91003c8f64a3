"""The name options of the output side: UMIs taken from the index part of the name (--umi_loc index1 / index2 / per_index;
Read::firstIndex / lastIndex, UmiProcessor::process) and --fix_mgi_id (Read::fixMGI), which the reference applies first.
  T1  the host writer's functions against names recorded from the reference (tests/golden/read_names/names_table.json)
  T2  fastp_gpu_format_streams / fastp_gpu_format_all_streams and fq_glue.cpp == the host writer, every stream
  T3  block, wave and copy-group edges, every name of the zoo on both sides of a block boundary
  T4  the file loop and the pipeline against the reference's outputs and JSON (tests/golden/read_names/*.npz)
  T5  the documented capacity bound; overflow
  T6  the ground that does not change: locations 0..3 without the flag, unknown option words, index2 on single reads
The CPU suite runs the product sources on the SIMT emulator; every `-m gpu` test names its emulator twin."""
import gzip

import numpy as np
import pytest

import engines
import format7_util as f7
import format_util
import golden_util
import read_names_util as rn
import streamlib
from driver import md5
from fastp_amd import abi, engine, hostloop
from test_stream_abi import _files


# ---- T1: the host functions against the reference's table ---------------------------------------------------------
def test_host_name_functions_on_the_issue_examples():
    assert hostloop.first_index(b"@a:bc") == b"bc" and hostloop.first_index(b"@a:b") == b""
    assert hostloop.first_index(b"@abcd:x") == b"" and hostloop.last_index(b"@abcd:x") == b""
    assert hostloop.first_index(b"@r 1:N:0:ACGT+TTGA") == b"ACGT" and hostloop.last_index(b"@r 1:N:0:ACGT+TTGA") == b"TTGA"
    assert hostloop.last_index(b"@r 1:N:0:ACGT+TT+GA") == b"GA" and hostloop.first_index(b"@r 1:N:0:ACGT+TT+GA") == b"ACGT"
    assert hostloop.first_index(b"@r 1:N:0:ACGT+T") == b"ACGT+T" and hostloop.first_index(b"@r 1:N:0:+:AC") == b"AC"
    assert hostloop.first_index(b"@p+qqqq") == b"" and hostloop.last_index(b"@p+qqqq") == b"qqqq"
    assert hostloop.fix_mgi_name(b"@V300:L1:C2:R3/1") == b"@V300:L1:C2:R3 /1" and hostloop.fix_mgi_name(b"@/2") == b"@ /2"
    assert hostloop.fix_mgi_name(b"@x1") == b"@x1" and hostloop.fix_mgi_name(b"@a/3") == b"@a/3"
    assert hostloop.first_index(hostloop.fix_mgi_name(b"@V300:L1:C2:R3/1")) == b"R3 /1"


def test_host_name_editor_equals_the_reference_table():
    runs = rn.load_table()
    assert len(runs) == 20   # PE: 3 locations x MGI x prefix; SE: index1 and per_index (the reference's CLI refuses index2)
    seen = set()
    for run in runs:
        ed = rn.editor(run["loc"], run["mgi"], run["prefix"].encode(), run["delimiter"].encode())
        seen.add((run["loc"], run["mgi"], bool(run["prefix"]), run["paired"]))
        for i, (a, b) in enumerate(rn.ZOO):
            n1, n2 = ed.edit(a, b"ACGTACGTAC", b if run["paired"] else None, b"ACGTACGTAC" if run["paired"] else None)
            what = f"{run['loc']} mgi={run['mgi']} prefix={run['prefix']!r} paired={run['paired']}: {a!r}"
            assert n1 == run["names1"][i].encode("latin-1"), what
            if run["paired"]:
                assert n2 == run["names2"][i].encode("latin-1"), what
    assert len(seen) == 20
    # the functions one by one, on the per_index rows without a prefix: tag = ":" + firstIndex(r1) + "_" + lastIndex(r2)
    for mgi in (False, True):
        run = next(r for r in runs if r["loc"] == "per_index" and r["mgi"] == mgi and not r["prefix"] and r["paired"])
        for i, (a, b) in enumerate(rn.ZOO):
            fa, fb = (hostloop.fix_mgi_name(a), hostloop.fix_mgi_name(b)) if mgi else (a, b)
            tag = b":" + hostloop.first_index(fa) + b"_" + hostloop.last_index(fb)
            sp = fa.find(b" ")
            assert run["names1"][i].encode("latin-1") == (fa + tag if sp < 0 else fa[:sp] + tag + fa[sp:]), a


# ---- T2: the device formatter and fq_glue.cpp == the host writer ---------------------------------------------------
# id -> (case of tests/cases.py, seven-stream call, location, MGI fix, prefix, delimiter, want_unpaired, line end)
T2 = {}
for _loc in (None,) + rn.LOCATIONS:
    for _mgi in (False, True):
        if _loc or _mgi:
            T2[f"pe_all-{_loc or 'none'}-{'mgi' if _mgi else 'plain'}"] = ("pe_merge_overlapped_out", True, _loc, _mgi, b"", b":", False, b"\n")
T2["pe_six-index1-plain"] = ("pe_filters", False, "index1", False, b"", b":", True, b"\n")
T2["pe_six-per_index-mgi-prefix"] = ("pe_filters", False, "per_index", True, b"U", b"#~", True, b"\n")
T2["pe_six-index2-mgi"] = ("pe_merge_unmerged", False, "index2", True, b"UMI", b"_", False, b"\n")
T2["pe_six-per_read-mgi"] = ("pe_umi_per_read", False, "per_read", True, b"U", b":", False, b"\n")   # an old location with the new flag
T2["se_six-index1-plain"] = ("se_adapter_cut", False, "index1", False, b"", b":", False, b"\n")
T2["se_six-per_index-mgi"] = ("se_adapter_cut", False, "per_index", True, b"U", b"#~", False, b"\n")
T2["se_all-none-mgi"] = ("se_adapter_cut", True, None, True, b"", b":", False, b"\n")
T2["pe_all-per_index-mgi-crlf"] = ("pe_merge_overlapped_out", True, "per_index", True, b"U", b":", False, b"\r\n")
T2["pe_six-index1-mgi-crlf"] = ("pe_filters", False, "index1", True, b"", b":", True, b"\r\n")


def _t2(mk_engine, mem, key, cpp_lib=None):
    case, seven, loc, mgi, prefix, delim, unpaired, eol = T2[key]
    ed = rn.editor(loc, mgi, prefix, delim, umi_len=0 if loc in rn.LOCATIONS else 6)
    params, fq1, fq2 = rn.inputs(case, 600)
    want = rn.expected(mk_engine, params, fq1, fq2, 150, True, unpaired, ed)
    tagged, fixed, inside, untagged = rn.name_stats(want, fq1, fq2, ed)
    print(f"{key}: {tagged} tagged names, {fixed} MGI-fixed, {inside} with the MGI space inside the tag, {untagged} untagged")
    if loc:
        assert tagged >= 50
    if mgi:
        assert fixed >= 20
    if mgi and loc in rn.LOCATIONS:
        assert inside >= 5
    if loc == "index1":
        assert untagged >= 5
    if params.merge:
        assert b" merged_" in want["merged"]
    if params.overlapped_out:
        assert len(want["overlapped"]) > 1000
    if params.paired and not params.merge_include_unmerged:   # (--include_unmerged sends what merge mode keeps to one stream)
        assert len(want["failed"]) > 1000
    if unpaired:
        assert want["unpaired1"] and want["unpaired2"]
    if cpp_lib is not None:     # fq_glue.cpp through its C entry points
        glue = rn.expected(mk_engine, params, fq1, fq2, 150, True, unpaired, ed, cpp_lib=cpp_lib)
        for k in rn.STREAMS:
            assert glue[k] == want[k], f"{key}: fq_glue.cpp's stream {k} differs from hostloop's"
    g = mk_engine(params)
    rc, got, lens, caps = rn.run_formatter(g, mem, fq1.replace(b"\n", eol), fq2.replace(b"\n", eol) if fq2 is not None else None,
                                           150, ed, seven, True, unpaired)
    g.close()
    assert rc == 0, rc
    for i, k in enumerate(rn.STREAMS[:len(caps)]):
        assert got[k] == want[k], f"{key}: stream {k} differs ({len(got[k])} vs {len(want[k])} bytes)"
        assert lens[i] == len(want[k]) and b"\r" not in got[k]


@pytest.mark.parametrize("key", list(T2))
def test_sim_name_options_equal_host_writer(key):
    _t2(engines.sim_engine, format_util.NumpyMem(), key, cpp_lib=engine.load_library(engines.build_sim()))


@pytest.mark.gpu
@pytest.mark.twin("test_sim_name_options_equal_host_writer")
@pytest.mark.parametrize("key", list(T2))
def test_gpu_name_options_equal_host_writer(key):
    _t2(engines.gpu_engine, format_util.TorchMem(), key)


# ---- T3: edges -----------------------------------------------------------------------------------------------------
EDGE_SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]   # a copy group 16 lanes, a wave 64, FMT_BLOCK 256


def _t3(mk_engine, mk_mem, n, rot):
    """PE per_index + MGI + --overlapped_out: up to three emissions per unit; unit i is called ZOO[(i + rot) % len(ZOO)]"""
    ed = rn.editor("per_index", True, b"U", b"#")
    params, fq1, fq2 = rn.inputs("pe_overlapped_out_noadapter", n, rot=rot)
    want = rn.expected(mk_engine, params, fq1, fq2, 150, True, False, ed)
    g = mk_engine(params)
    rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, fq2, 150, ed, True)
    g.close()
    assert rc == 0
    for i, k in enumerate(rn.STREAMS):
        assert got[k] == want[k] and lens[i] == len(want[k]), f"n = {n}, rotation {rot}: stream {k} differs"
    return want


def _rotations(n):
    # from 257 units on there is a block boundary: every name of the zoo is unit 255 (and so its successor unit 256) once
    return range(len(rn.ZOO)) if n == 257 else [n % len(rn.ZOO)]


def _t3_all(mk_engine, mk_mem):
    for n in EDGE_SIZES:
        for rot in _rotations(n):
            want = _t3(mk_engine, mk_mem, n, rot)
        if n >= 255:
            assert f7.count_records(want["overlapped"])[0] >= 30 and len(want["out1"]) > 1000


def test_sim_name_options_over_all_edge_sizes():
    """every size and rotation the GPU test runs"""
    _t3_all(engines.sim_engine, format_util.NumpyMem)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_name_options_over_all_edge_sizes")
def test_gpu_name_options_over_all_edge_sizes():
    _t3_all(engines.gpu_engine, format_util.TorchMem)


# ---- T4: the file loop and the pipeline against the reference ----------------------------------------------------------
FILE_SETS = list(rn.FILE_SETS)


def _t4_stream(lib, name, tmp_path, chunk_bytes, gz, max_len=152):
    fq1, fq2, meta = rn.load_file_set(name)
    assert meta["json"] == meta["json_plain"], "the reference's report changed with the name options"
    assert fq1.count(b"\n") // 4 <= 600
    params = rn.file_set_params(name, max_len)
    p1, p2 = _files(tmp_path, fq1, fq2)
    want = list(meta["outputs"])
    outs, ctr, lay, amaps, st = rn.run_files(lib, params, p1, p2, str(tmp_path), want, chunk_bytes, rn.file_set_editor(name),
                                             compress=want if gz else ())
    if gz:
        outs = {k: gzip.decompress(v) for k, v in outs.items()}
    golden_util.check_against_golden(name, streamlib.as_outputs(outs, fq2 is not None), streamlib.report(ctr, lay, params, amaps), meta)
    assert "failed" in meta["outputs"] and all(v["size"] > 0 for v in meta["outputs"].values())
    return st, ctr


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("name", FILE_SETS)
def test_sim_stream_name_options_equal_reference(name, gz, tmp_path):
    st, _ = _t4_stream(engine.load_library(engines.build_sim()), name, tmp_path, 60000, gz)
    assert st.chunks >= 2


def test_sim_stream_name_options_survive_a_replan(tmp_path):
    st, _ = _t4_stream(engine.load_library(engines.build_sim()), "pe_per_index_mgi_merge", tmp_path, 60000, False, max_len=100)
    assert st.replans >= 1 and st.chunks >= 2


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_name_options_equal_reference")
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("name", FILE_SETS)
def test_gpu_stream_name_options_equal_reference(name, gz, tmp_path):
    _t4_stream(engine.load_library(), name, tmp_path, 1 << 20, gz)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_name_options_equal_reference")
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("name", FILE_SETS)
def test_gpu_pipeline_name_options_equal_reference(name, gz, tmp_path):
    """FastqPipeline.run(umi=, fix_mgi_id=) writes the reference's files; its counters are those of the file loop's run,
    whose report equals the reference's (the twin runs the same sets through the file loop: the pipeline needs torch
    tensors of a GPU)"""
    import os
    from fastp_amd.pipeline import FastqPipeline
    fq1, fq2, meta = rn.load_file_set(name)
    params = rn.file_set_params(name)
    (tmp_path / "s").mkdir()
    _, ctr = _t4_stream(engine.load_library(), name, tmp_path / "s", 1 << 20, False)
    p1, p2 = _files(tmp_path, fq1, fq2)
    path = {k: os.path.join(str(tmp_path), k + (".fq.gz" if gz else ".fq")) for k in ("out1", "out2", "failed", "merged")}
    loc, mgi, prefix, delim = rn.FILE_SETS[name][3]
    pipe = FastqPipeline(params, device=0, chunk_bytes=1 << 20)
    try:
        pipe.run(p1, p2, path["out1"], path["out2"] if fq2 is not None else None, failed_out=path["failed"],
                 merged_out=path["merged"] if params.merge else None, umi=(loc, 0, prefix, delim) if loc else None, fix_mgi_id=mgi)
        got_ctr = pipe.counters()
    finally:
        pipe.close()
    for k, exp in meta["outputs"].items():
        got = open(path[k], "rb").read()
        got = gzip.decompress(got) if gz else got
        assert md5(got) == exp["md5"], f"{k}: {len(got)} bytes, the reference wrote {exp['size']}"
    assert np.array_equal(got_ctr, ctr)


# ---- T5: capacity ------------------------------------------------------------------------------------------------------
def _one_base_pairs(n=300):
    """reads of one base under 200-byte names: the tag (both indexes) is far longer than the record it is added to"""
    rng = np.random.default_rng(5)
    r = [[], []]
    for i in range(n):
        stem = b"@" + b"%05d" % i + b"x" * 60
        for m in (0, 1):
            name = stem + b" %d:N:0:" % (m + 1) + b"ACGT" * 16 + b"+" + b"TGCA" * 16
            name += b"A" * (200 - len(name))
            r[m].append(name + b"\n" + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1)) + b"\n+\nI\n")
    return b"".join(r[0]), b"".join(r[1])


def _t5(mk_engine, mk_mem):
    fq1, fq2 = _one_base_pairs()
    p = abi.default_params(True, 64)
    p.length_filter = 0
    p.adapter_enabled = 0
    ed = rn.editor("per_index", False, b"U", b"#")
    want = rn.expected(mk_engine, p, fq1, fq2, 64, True, False, ed)
    assert len(want["out1"]) > 1.5 * len(fq1)        # the records grow by more than half: the old bound (text + n tags of 2 * umi_len) is no bound here
    g = mk_engine(p)
    rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, fq2, 64, ed, False)
    g.close()
    assert rc == 0 and all(lens[i] <= caps[i] for i in range(6))
    for k in format_util.STREAMS:
        assert got[k] == want[k], f"stream {k} differs"
    rec_len = len(want["out1"]) // 300
    assert rec_len > 300 and rec_len * 300 == len(want["out1"])   # (equal names and tags: equal records)
    # 100 bytes: no record fits; 2 * rec_len + 7: two whole records fit, a part of the third would
    for small in (100, 2 * rec_len + 7):
        g = mk_engine(p)
        rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, fq2, 64, ed, False, shrink=0, shrink_to=small)   # (checks the 0xEE fill
        g.close()                                                                                                   # behind the capacity)
        assert rc == abi.E_OVERFLOW and lens[0] == len(want["out1"]) and lens[1] == len(want["out2"])
        assert got["out2"] == want["out2"]
        fit = small // rec_len * rec_len   # the whole records that fit are written, the rest of the buffer keeps its fill
        assert fit == (0 if small == 100 else 2 * rec_len)
        assert got["out1"][:fit] == want["out1"][:fit] and got["out1"][fit:] == b"\xEE" * (small - fit), small


def test_sim_name_options_capacity_bound_and_overflow():
    _t5(engines.sim_engine, format_util.NumpyMem)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_name_options_capacity_bound_and_overflow")
def test_gpu_name_options_capacity_bound_and_overflow():
    _t5(engines.gpu_engine, format_util.TorchMem)


# ---- T6: unchanged ground ----------------------------------------------------------------------------------------------
OLD_LOCATIONS = [None, "read1", "read2", "per_read"]


def _t6_old(mk_engine, mk_mem, case, seven, loc):
    """locations 0..3 without the flag: the streams of the host writer, byte for byte (the kernels' uniform branch)"""
    ed = hostloop.UmiNameEditor(loc, 5, b"P", b"#") if loc else None
    params, fq1, fq2 = rn.inputs(case, 300)
    want = rn.expected(mk_engine, params, fq1, fq2, 150, True, False, ed)
    g = mk_engine(params)
    rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, fq2, 150, ed, seven)
    g.close()
    assert rc == 0 and sum(lens) > 10000
    for i, k in enumerate(rn.STREAMS[:len(caps)]):
        assert got[k] == want[k] and lens[i] == len(want[k]), f"{case} {loc}: stream {k} differs"


@pytest.mark.parametrize("loc", OLD_LOCATIONS, ids=lambda x: x or "none")
@pytest.mark.parametrize("case,seven", [("pe_filters", False), ("pe_merge_overlapped_out", True)], ids=["six", "seven"])
def test_sim_old_locations_unchanged(case, seven, loc):
    _t6_old(engines.sim_engine, format_util.NumpyMem, case, seven, loc)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_old_locations_unchanged")
@pytest.mark.parametrize("loc", OLD_LOCATIONS, ids=lambda x: x or "none")
@pytest.mark.parametrize("case,seven", [("pe_filters", False), ("pe_merge_overlapped_out", True)], ids=["six", "seven"])
def test_gpu_old_locations_unchanged(case, seven, loc):
    _t6_old(engines.gpu_engine, format_util.TorchMem, case, seven, loc)


def _t6_words(mk_engine, mk_mem, lib=None):
    params, fq1, fq2 = rn.inputs("se_adapter_cut", 64)
    for word in (7, 0x200, 0x200 | 4, 0x107, -1):
        g = mk_engine(params)
        rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, None, 150, None, False, word=word)
        g.close()
        assert rc == abi.E_UNSUPPORTED and sum(lens) == 0, hex(word)
        if lib is not None:
            assert rn.NamesCppHost(lib, params, True, False, None, word=word).rc == abi.E_UNSUPPORTED
    # index2 on single-end input: no edit (UmiProcessor::process takes no branch without a read 2)
    plain = rn.expected(mk_engine, params, fq1, None, 150, True, False, None)
    g = mk_engine(params)
    rc, got, lens, caps = rn.run_formatter(g, mk_mem(), fq1, None, 150, rn.editor("index2"), False)
    g.close()
    assert rc == 0 and got["out1"] == plain["out1"] and got["failed"] == plain["failed"] and len(got["out1"]) > 1000


def test_sim_unknown_option_words_and_index2_on_single_reads():
    _t6_words(engines.sim_engine, format_util.NumpyMem, engine.load_library(engines.build_sim()))


@pytest.mark.gpu
@pytest.mark.twin("test_sim_unknown_option_words_and_index2_on_single_reads")
def test_gpu_unknown_option_words_and_index2_on_single_reads():
    _t6_words(engines.gpu_engine, format_util.TorchMem)
