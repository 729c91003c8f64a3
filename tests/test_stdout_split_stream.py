"""--stdout and --split / --split_by_lines through the file loop (fastp_gpu_stream_set_interleaved_output,
fastp_gpu_stream_set_split) against what the real reference wrote (tests/golden/output_files/, -w 1): the set of file
names, and every file's text.  The CPU suite runs the product sources on the SIMT emulator; every `-m gpu` test names its
emulator twin."""
import os
import subprocess

import numpy as np
import pytest

import engines
import outfiles_util as ofu
import streamlib
from fastp_amd import abi, engine
from test_stream_abi import _files

GEOMETRIES = ["one_chunk", "64k", "pack_edge"]


def _record_bytes(fq):
    lines = fq.split(b"\n")
    return [sum(len(x) + 1 for x in lines[i:i + 4]) for i in range(0, len(lines) - 1, 4)]


def _trips(sizes, chunk):
    """units per trip of the file loop: each file gives the whole records that fit into `chunk` bytes, a unit needs all mates"""
    at, out, n = [0] * len(sizes), [], min(len(s) for s in sizes)
    while at[0] < n:
        fit = []
        for m, s in enumerate(sizes):
            k, b = 0, 0
            while at[m] + k < len(s) and b + s[at[m] + k] <= chunk:
                b += s[at[m] + k]
                k += 1
            fit.append(k)
        k = min(min(fit), n - at[0])
        assert k > 0
        out.append(k)
        at = [a + k for a in at]
    return out


def _chunk_bytes(geometry, fq1, fq2):
    """one chunk for the whole input; 64 KiB, so that packs span chunks; the smallest multiple of 256 at which a trip that is
    not the last one ends exactly on a pack boundary (worked out from the fixture's record sizes; _golden_case checks that the
    loop made the trips this was worked out for)"""
    if geometry == "one_chunk":
        return 1 << 22
    if geometry == "64k":
        return 1 << 16
    sizes = [_record_bytes(f) for f in (fq1, fq2) if f is not None]
    # (the --stdout cases hold 500 units, no pack boundary: a formatter block's edge, or else a wave's)
    for edge, first in ((1000, 1 << 16),) if len(sizes[0]) > 1000 else ((256, 1 << 13), (64, 1 << 13)):
        for chunk in range(first, 1 << 19, 256):
            ends = np.cumsum(_trips(sizes, chunk))[:-1]
            if len(ends) and any(e % edge == 0 for e in ends):
                return chunk
    raise AssertionError("no chunk size puts a trip's end on a pack boundary")


def _plain_run(lib, name, tmp_path, fq1, fq2, params, max_units=0):
    """the same input without --split / --stdout: its counters and adapter maps"""
    d = tmp_path / "plain"
    d.mkdir(exist_ok=True)
    p1, p2 = _files(d, fq1, fq2)
    want = ("out1", "out2") if fq2 is not None and not params.merge else (("out1",) if fq2 is None else ("out1", "out2", "merged"))
    files, ctr, lay, amaps, st, info = ofu.run(lib, params, p1, p2, str(d), want=want, umi=ofu.case_umi(name), chunk_bytes=1 << 22,
                                               reads_to_process=max_units)
    return streamlib.report(ctr, lay, params, amaps), ctr


def _split_arg(name):
    c = ofu.CASES[name]
    how, v = c["split"]
    return dict(by_lines=how == "lines", reads_per_file=ofu.reads_per_file(name), number=v if how == "files" else 0, digits=c.get("digits", 4))


def _check_split_files(files, st, info, gz, paired):
    for q, tag in enumerate(("o1", "o2")[:2 if paired else 1]):
        mine = {k: v for k, v in files.items() if k.split(".")[1] == tag}
        assert info["split_files"] == len(mine), (info, sorted(files))
        assert st.bytes_out[q] == sum(len(v) for v in mine.values())
        if gz:
            assert all(v.endswith(ofu.BGZF_EOF) for v in mine.values())


def _golden_case(lib, name, geometry, tmp_path, max_len=56):
    c = ofu.CASES[name]
    fq1, fq2, meta = ofu.load(name)
    assert (fq1, fq2) == ofu.case_input(name)      # (the fixture's text is the generator's: the case table describes it)
    params = ofu.case_params(name, max_len)
    chunk = _chunk_bytes(geometry, fq1, fq2)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    p1, p2 = _files(tmp_path, fq1, fq2)
    umi = ofu.case_umi(name)
    if c.get("split"):
        files, ctr, lay, amaps, st, info = ofu.run(lib, params, p1, p2, str(run_dir), chunk_bytes=chunk, umi=umi, split=_split_arg(name),
                                                   gz=bool(c.get("gz")))
        _check_split_files(files, st, info, bool(c.get("gz")), fq2 is not None)
        expected = meta["files"]
    else:
        paired_plain = fq2 is not None and not params.merge
        want = tuple(c.get("want", ())) + (("merged",) if params.merge else ("out1",))
        files, ctr, lay, amaps, st, info = ofu.run(lib, params, p1, p2, str(run_dir), want=want, chunk_bytes=chunk, umi=umi,
                                                   interleaved_out=paired_plain)
        main = "merged.fq" if params.merge else "out1.fq"
        assert st.bytes_out[3 if params.merge else 0] == len(files[main]) and st.bytes_out[1] == 0
        expected = dict(meta["files"])
        expected[main] = meta["stdout"]
    assert sorted(files) == sorted(expected), (sorted(files), sorted(expected))
    for fn, exp in expected.items():
        text = ofu.text_of(fn, files[fn])
        assert (ofu.md5(text), len(text)) == (exp["md5"], exp["size"]), f"{name} {geometry}: {fn} differs from the reference's"
    if geometry != "one_chunk":
        sizes = [_record_bytes(f) for f in (fq1, fq2) if f is not None]
        trips = _trips(sizes, chunk)
        assert st.chunks == len(trips) >= 2, (st.chunks, trips)      # (the trips are where _chunk_bytes put them)
    rep, plain_ctr = _plain_run(lib, name, tmp_path, fq1, fq2, params)
    assert np.array_equal(ctr, plain_ctr) and streamlib.report(ctr, lay, params, amaps) == rep
    return st


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", list(ofu.CASES))
def test_sim_stream_output_files_equal_reference_golden(name, geometry, tmp_path):
    _golden_case(engine.load_library(engines.build_sim()), name, geometry, tmp_path)


def _replan_case(lib, tmp_path):
    """a read longer than max_len in the third pack: the file state survives the new context"""
    name = "split_pe_files5"
    fq1, fq2, meta = ofu.load(name)
    lines = fq1.split(b"\n")
    u = 2500
    lines[4 * u + 1] += b"ACGTTGCA" * 5
    lines[4 * u + 3] += b"F" * 40
    fq1 = b"\n".join(lines)
    got = {}
    for tag, max_len in (("replan", 56), ("wide", 96)):
        d = tmp_path / tag
        d.mkdir()
        p1, p2 = _files(d, fq1, fq2)
        params = ofu.case_params(name, max_len)
        files, ctr, lay, amaps, st, info = ofu.run(lib, params, p1, p2, str(d), chunk_bytes=1 << 16, split=_split_arg(name))
        _check_split_files(files, st, info, False, True)
        got[tag] = ({k: v for k, v in files.items() if k[0].isdigit()}, st.replans)
        # counters and adapter maps: those of the unsplit run of the same text (which re-plans at the same read)
        u = tmp_path / (tag + "_unsplit")
        u.mkdir()
        _, uctr, ulay, uamaps, ust, _ = ofu.run(lib, ofu.case_params(name, max_len), p1, p2, str(u), want=("out1", "out2"), chunk_bytes=1 << 16)
        assert ust.replans == st.replans and np.array_equal(ctr, uctr)
        assert streamlib.report(ctr, lay, params, amaps) == streamlib.report(uctr, ulay, params, uamaps)
    assert got["replan"][1] >= 1 and got["wide"][1] == 0
    assert got["replan"][0] == got["wide"][0] and len(got["wide"][0]) == 10
    assert b"ACGTTGCAACGTTGCA" in got["replan"][0]["03.o1.fq"]


def _limit_case(lib, tmp_path):
    """--reads_to_process 1500: the files of the input's first 1500 units"""
    name = "split_se_lines"
    fq1, _, meta = ofu.load(name)
    head = b"\n".join(fq1.split(b"\n")[:4 * 1500]) + b"\n"
    got = {}
    for tag, text, limit in (("limit", fq1, 1500), ("head", head, 0)):
        d = tmp_path / tag
        d.mkdir()
        p1, _ = _files(d, text, None)
        params = ofu.case_params(name)
        files, ctr, lay, amaps, st, info = ofu.run(lib, params, p1, None, str(d), chunk_bytes=1 << 16, split=_split_arg(name),
                                                   reads_to_process=limit)
        _check_split_files(files, st, info, False, False)
        got[tag] = {k: v for k, v in files.items() if k[0].isdigit()}
        assert st.units == 1500
        # counters and adapter maps: those of the unsplit run of the same text with the same limit
        u = tmp_path / (tag + "_unsplit")
        u.mkdir()
        _, uctr, ulay, uamaps, ust, _ = ofu.run(lib, ofu.case_params(name), p1, None, str(u), want=("out1",), chunk_bytes=1 << 16,
                                                reads_to_process=limit)
        assert ust.units == 1500 and np.array_equal(ctr, uctr)
        assert streamlib.report(ctr, lay, params, amaps) == streamlib.report(uctr, ulay, params, uamaps)
    assert got["limit"] == got["head"] and len(got["head"]) >= 2


def test_sim_stream_split_survives_a_replan(tmp_path):
    _replan_case(engine.load_library(engines.build_sim()), tmp_path)


def test_sim_stream_split_with_reads_to_process(tmp_path):
    _limit_case(engine.load_library(engines.build_sim()), tmp_path)


# ---- the setters' refusals -----------------------------------------------------------------------------------------
def _refused(lib, tmp_path, name, **kw):
    fq1, fq2, _ = ofu.load(name)
    d = tmp_path / ("r%d" % len(os.listdir(tmp_path)))
    d.mkdir()
    p1, p2 = _files(d, fq1, fq2)
    params = kw.pop("params", None) or ofu.case_params(name)
    with pytest.raises(streamlib.StreamError) as e:
        ofu.run(lib, params, p1, p2, str(d), chunk_bytes=1 << 22, **kw)
    assert e.value.code == abi.E_INVALID, e.value
    return str(e.value)


def _setter_errors(lib, tmp_path):
    pe, se = "split_pe_files5", "split_se_files2"
    ok = dict(by_lines=False, reads_per_file=640, number=5, digits=2)
    merge = ofu.case_params("stdout_pe_merge")
    assert "--merge" in _refused(lib, tmp_path, "stdout_pe_merge", params=merge, split=ok)
    assert "--stdout" in _refused(lib, tmp_path, pe, want=("out1",), interleaved_out=True, split=ok)
    assert "--failed_out" in _refused(lib, tmp_path, pe, want=("failed",), split=ok)
    assert "--unpaired1" in _refused(lib, tmp_path, pe, want=("unpaired1",), split=ok)
    assert "--unpaired2" in _refused(lib, tmp_path, pe, want=("unpaired2",), split=ok)
    ov = ofu.case_params(pe)
    ov.overlapped_out = 1
    assert "--overlapped_out" in _refused(lib, tmp_path, pe, params=ov, want=("overlapped",), split=ok)
    # (--merged_out cannot be wanted without merge mode, which is refused by name above)
    assert "reads_per_file" in _refused(lib, tmp_path, pe, split=dict(ok, reads_per_file=0))
    for number in (1, 1000):
        assert "number" in _refused(lib, tmp_path, pe, split=dict(ok, number=number))
    for digits in (-1, 11):
        assert "digits" in _refused(lib, tmp_path, pe, split=dict(ok, digits=digits))
    assert "out2" in _refused(lib, tmp_path, pe, split=dict(ok, out2=False))
    assert "out1" in _refused(lib, tmp_path, se, split=dict(ok, out1=False))
    # interleaved output: single-end, merge, out2 wanted, out1 not wanted
    assert "paired" in _refused(lib, tmp_path, se, want=("out1",), interleaved_out=True)
    assert "merge" in _refused(lib, tmp_path, "stdout_pe_merge", params=merge, want=("out1",), interleaved_out=True)
    assert "out2" in _refused(lib, tmp_path, pe, want=("out1", "out2"), interleaved_out=True)
    assert "OUT1" in _refused(lib, tmp_path, pe, want=(), interleaved_out=True)

    # both setters once the run has started
    def late(lib_, s):
        sp = ofu.StreamSplit()
        sp.by_lines, sp.reads_per_file, sp.number, sp.digits, sp.out1, sp.out2 = 0, 640, 5, 2, b"/nonexistent/o1.fq", b"/nonexistent/o2.fq"
        import ctypes as C
        return lib_.fastp_gpu_stream_set_split(s, C.byref(sp)), lib_.fastp_gpu_stream_set_interleaved_output(s, 1)
    fq1, fq2, _ = ofu.load(pe)
    d = tmp_path / "late"
    d.mkdir()
    p1, p2 = _files(d, fq1, fq2)
    info = ofu.run(lib, ofu.case_params(pe), p1, p2, str(d), want=("out1", "out2"), chunk_bytes=1 << 22, after_run=late)[5]
    assert info["late"] == (abi.E_INVALID, abi.E_INVALID) and info["split_files"] == 0


def test_sim_stream_output_setters_refuse(tmp_path):
    _setter_errors(engine.load_library(engines.build_sim()), tmp_path)


# ---- the live reference ----------------------------------------------------------------------------------------------
def test_sim_stream_split_equals_live_reference(tmp_path):
    """4,100 pairs, -S 4000, against oracle/_ref/fastp_ref -w 1 run here (skips itself where the binary is not built)"""
    import cases
    import synth
    ref = os.path.join(engines.ROOT, "oracle", "_ref", "fastp_ref")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/fastp_ref is not built")
    d = synth.synth_pairs(4100, L=50, seed=77, paired=True)
    fq1, fq2 = synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1), synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2)
    p1, p2 = _files(tmp_path, fq1, fq2)
    want_dir, got_dir = tmp_path / "ref", tmp_path / "got"
    want_dir.mkdir()
    got_dir.mkdir()
    subprocess.run([ref, "-i", p1, "-I", p2, "-o", str(want_dir / "o1.fq"), "-O", str(want_dir / "o2.fq"), "-S", "4000", "-w", "1",
                    "-j", str(tmp_path / "r.json"), "-h", str(tmp_path / "r.html")] + cases.CASES["pe_default"][1],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = ofu.run(engine.load_library(engines.build_sim()), cases.CASES["pe_default"][2](56), p1, p2, str(got_dir), chunk_bytes=1 << 16,
                    split=dict(by_lines=True, reads_per_file=1000, digits=4))[0]
    want = {fn: open(want_dir / fn, "rb").read() for fn in sorted(os.listdir(want_dir))}
    assert len(want) >= 6 and files == want


# ---- -m gpu -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_output_files_equal_reference_golden")
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", list(ofu.CASES))
def test_gpu_stream_output_files_equal_reference_golden(name, geometry, tmp_path):
    _golden_case(engine.load_library(), name, geometry, tmp_path)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_split_survives_a_replan")
def test_gpu_stream_split_survives_a_replan(tmp_path):
    _replan_case(engine.load_library(), tmp_path)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_split_with_reads_to_process")
def test_gpu_stream_split_with_reads_to_process(tmp_path):
    _limit_case(engine.load_library(), tmp_path)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_output_setters_refuse")
def test_gpu_stream_output_setters_refuse(tmp_path):
    _setter_errors(engine.load_library(), tmp_path)
