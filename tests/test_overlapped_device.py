"""--overlapped_out's stream written by the device formatter: fastp_gpu_format_all_streams (seven streams, up to three
records per pair) against the host writer (fastp_amd.hostloop.apply_results), and the file loop's device path
(fastp_gpu_stream_set_overlapped_output / FASTP_GPU_STREAM_OVERLAPPED=device) against the reference's goldens.
The CPU suite runs the product sources on the SIMT emulator; every `-m gpu` test names its emulator twin, but for the
pipeline's (fastp_amd/pipeline.py runs on torch tensors of a GPU)."""
import gzip
import os

import numpy as np
import pytest

import engines
import format7_util as f7
import format_util
import golden_util
import streamlib
import streamlib7
import test_ref_binding as rb
from fastp_amd import abi, engine
from test_stream_abi import OVERLAPPED_GOLDENS, _files

SET_NAMES = list(f7.SETS)
DEVICE_GOLDENS = OVERLAPPED_GOLDENS + ["pe_exotic_default"]
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, 513]   # FMT_BLOCK is 256, a wave 64 lanes, a copy group 16 lanes
OVERLAPPED_BINDING_CASES = [n for n in rb.BINDING_CASES if rb._overlapped_out(n)]


# ---- A1: seven streams equal the host writer ----------------------------------------------------------------------
def _a1(mk_engine, mem, set_name):
    got, want = f7.case(mk_engine, mem, set_name, 600)
    records, nonempty = f7.count_records(want["overlapped"])   # (the EXPECTED stream: a pass must not be vacuous)
    print(f"{set_name}: {records} overlapped records, {nonempty} with bases")
    assert records >= 50 and nonempty >= 5
    if set_name.endswith(("_trims", "_noadapter")) or set_name == "correction":
        assert nonempty >= 100
    if set_name == "umi":   # the name edit of out1: ":<UMI of read 1>_<UMI of read 2>" in front of the first space
        import re
        names = want["overlapped"].split(b"\n")[0::4][:-1]
        assert names and all(re.match(rb"@\S+:[ACGTN]{0,6}_[ACGTN]{0,6}( |$)", x) for x in names), names[:3]   # (reads shorter than the UMI)
        assert sum(1 for x in names if re.match(rb"@\S+:[ACGTN]{6}_[ACGTN]{6}( |$)", x)) >= 50
    if "merge" in set_name:
        assert b" merged_" in want["merged"]


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_sim_all_seven_streams_equal_host_writer(set_name):
    _a1(engines.sim_engine, format_util.NumpyMem(), set_name)


# ---- A2: block, wave and slot edges -------------------------------------------------------------------------------
def _a2_sizes(mk_engine, mk_mem, sizes):
    for n in sizes:
        got, want = f7.case(mk_engine, mk_mem(), "pe_overlapped_out_noadapter", n)
        if n == 257:
            records, nonempty = f7.count_records(want["overlapped"])
            print(f"n = 257: {records} overlapped records, {nonempty} with bases")
            assert records >= 50 and nonempty >= 30


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sim_all_seven_streams_at_block_and_wave_edges(n):
    _a2_sizes(engines.sim_engine, format_util.NumpyMem, [n])


def test_sim_all_seven_streams_over_all_edge_sizes():
    """the twin of the GPU test that runs every size in one test"""
    _a2_sizes(engines.sim_engine, format_util.NumpyMem, [1, 257])


def _hand_made_pairs(n=300):
    """records a generator does not make: names without a space, strand lines that repeat the name; pair i's insert
    is chosen so that pair 255 - the last unit of the first block - overlaps (out1 + out2 + overlapped: three
    emissions), its neighbour 254 fails the length filter in both mates without --failed_out (overlapped only)"""
    rng = np.random.default_rng(23)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    r1, r2 = [], []
    for i in range(n):
        if i == 254 or i % 7 == 3:
            L, ins = 40, 45      # reads below length_required that still overlap: the overlapped record is the only emission
        elif i % 3 == 0:
            L, ins = 60, 200     # no overlap
        else:
            L, ins = 60, int(rng.integers(40, 110))   # overlap; inserts below 60: read 1 ends where the overlap ends (cnt 0)
        if i == 255:
            L, ins = 60, 80
        frag = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=max(ins, L)))
        s1 = frag[:L]
        s2 = frag[max(0, ins - L):ins][::-1].translate(comp)[:L]
        s1, s2 = s1[:min(L, len(s1))], s2[:min(L, len(s2))]
        q1, q2 = bytes(rng.integers(60, 74, size=len(s1), dtype=np.uint8)), bytes(rng.integers(60, 74, size=len(s2), dtype=np.uint8))
        for mate, out, s, q in ((1, r1, s1, q1), (2, r2, s2, q2)):
            name = [b"@p%d" % i, b"@p%d %d:N:0:ACGT" % (i, mate), b"@p%d/%d" % (i, mate)][i % 3]
            strand = b"+" if i % 5 else b"+" + name[1:]
            out.append(name + b"\n" + s + b"\n" + strand + b"\n" + q + b"\n")
    return b"".join(r1), b"".join(r2)


@pytest.mark.parametrize("umi", [None, ("per_read", 4)])
def test_sim_all_seven_streams_on_hand_made_pairs(umi):
    fq1, fq2 = _hand_made_pairs()
    p = abi.default_params(True, 64)
    p.overlapped_out = 1
    p.adapter_enabled = 0
    p.length_required = 50
    p.dup_enabled = 0
    if umi:
        p.umi_len1 = p.umi_len2 = umi[1]
    want = f7.expected(engines.sim_engine, p, fq1, fq2, 64, False, False, umi)
    g = engines.sim_engine(p)
    rc, got, lens = f7.run_all_streams(g, format_util.NumpyMem(), p, fq1, fq2, 64, False, False, umi)
    g.close()
    assert rc == 0
    for k in f7.STREAMS:
        assert got[k] == want[k], f"stream {k} differs ({len(got[k])} vs {len(want[k])} bytes)"
    ov_names = want["overlapped"].split(b"\n")[0::4][:-1]
    out1_names = set(want["out1"].split(b"\n")[0::4])
    records, nonempty = f7.count_records(want["overlapped"])
    assert records >= 100 and nonempty >= 20 and records - nonempty >= 5
    stem = lambda x: x.split(b" ")[0].split(b"/")[0].split(b":")[0]
    assert b"@p255" in {stem(x) for x in ov_names} and b"@p255" in {stem(x) for x in out1_names}    # three emissions, a block's last unit
    assert b"@p254" in {stem(x) for x in ov_names} and b"@p254" not in {stem(x) for x in out1_names}  # the overlapped one alone
    assert any(b" " not in x for x in ov_names) and b"\n+p" in want["overlapped"]


# ---- A3: CRLF input -----------------------------------------------------------------------------------------------
def test_sim_all_seven_streams_crlf_input():
    params, fq1, fq2, umi = f7.inputs("pe_merge_overlapped_out_trims", 300)
    want = f7.expected(engines.sim_engine, params, fq1, fq2, 150, True, False, umi)
    g = engines.sim_engine(params)
    rc, got, lens = f7.run_all_streams(g, format_util.NumpyMem(), params, fq1.replace(b"\n", b"\r\n"), fq2.replace(b"\n", b"\r\n"), 150)
    g.close()
    assert rc == 0 and f7.count_records(want["overlapped"])[1] >= 30
    for k in f7.STREAMS:
        assert got[k] == want[k] and b"\r" not in got[k], f"stream {k} differs"


# ---- A4: six of seven ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pe_filters", "pe_merge", "se_adapter_cut"])
def test_sim_six_of_seven_equal_the_six_stream_call(name):
    params, fq1, fq2, umi = f7.inputs(name, 400)
    g = engines.sim_engine(params)
    rc6, six, lens6 = format_util.run_streams(g, format_util.NumpyMem(), params, fq1, fq2, 150, True, fq2 is not None, umi)
    g.close()
    g = engines.sim_engine(params)
    rc7, seven, lens7 = f7.run_all_streams(g, format_util.NumpyMem(), params, fq1, fq2, 150, True, fq2 is not None, umi,
                                           null_overlapped=True)
    g.close()
    assert rc6 == 0 and rc7 == 0
    assert lens7[:6] == lens6 and lens7[6] == 0
    for k in format_util.STREAMS:
        assert seven[k] == six[k], f"{name}: stream {k} differs"
    assert sum(lens6) > 0


# ---- A5: errors ---------------------------------------------------------------------------------------------------
def test_sim_all_seven_streams_overflow_and_missing_buffer():
    params, fq1, fq2, umi = f7.inputs("pe_overlapped_out_noadapter", 300)
    want = f7.expected(engines.sim_engine, params, fq1, fq2, 150, True, False, umi)
    assert len(want["overlapped"]) > 100
    g = engines.sim_engine(params)
    rc, got, lens = f7.run_all_streams(g, format_util.NumpyMem(), params, fq1, fq2, 150, shrink=6)   # (checks the 0xEE fill)
    g.close()
    assert rc == abi.E_OVERFLOW and lens[6] == len(want["overlapped"])
    for i, k in enumerate(format_util.STREAMS):
        assert got[k] == want[k] and lens[i] == len(want[k]), f"stream {k}"
    fit = 0   # the whole records that fit are written, the rest of the buffer keeps its fill
    for rec in want["overlapped"].split(b"\n@"):
        if fit + len(rec) + 1 > 100:
            break
        fit += len(rec) + 1
    assert fit > 0 and got["overlapped"][:fit] == want["overlapped"][:fit] and got["overlapped"][fit:] == b"\xEE" * (100 - fit)
    g = engines.sim_engine(params)
    rc, got, lens = f7.run_all_streams(g, format_util.NumpyMem(), params, fq1, fq2, 150, null_overlapped=True)
    g.close()
    assert rc == abi.E_INVALID


# ---- A6: the file loop's device path against the reference's goldens ----------------------------------------------
def _golden7(lib, name, tmp_path, chunk_bytes, overlapped, max_len=152):
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=max_len, fq1=fq1, fq2=fq2)
    p1, p2 = _files(tmp_path, fq1, fq2)
    want = list(meta["outputs"])
    assert "overlapped" in want
    if "out1" not in want:
        want += ["out1", "out2"]
    outs, ctr, lay, amaps, st, info = streamlib7.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=chunk_bytes,
                                                           umi=golden_util.umi_for(name), overlapped=overlapped)
    assert info["on_device"] == 1
    if overlapped == "gz":
        raw = outs["overlapped"]
        assert raw[-28:] == streamlib7.BGZF_EOF and st.bytes_overlapped == len(raw)
        outs["overlapped"] = gzip.decompress(raw)
    if overlapped == "emit":
        assert info["emit_calls"] == st.chunks    # one call per chunk, empty ones included
    golden_util.check_against_golden(name, streamlib.as_outputs(outs, True), streamlib.report(ctr, lay, params, amaps), meta)
    return st


@pytest.mark.parametrize("how", ["fd", "emit", "gz"])
@pytest.mark.parametrize("name", DEVICE_GOLDENS)
def test_sim_stream_overlapped_on_device_equals_reference_golden(name, how, tmp_path):
    lib = engine.load_library(engines.build_sim())
    st = _golden7(lib, name, tmp_path, 60000, how)
    assert st.chunks >= 2


def test_sim_stream_overlapped_on_device_survives_a_replan(tmp_path):
    lib = engine.load_library(engines.build_sim())
    st = _golden7(lib, "pe_overlapped_out_noadapter", tmp_path, 60000, "fd", max_len=100)
    assert st.replans >= 1


def _phred64_case(lib, tmp_path, chunk_bytes, n=900):
    """tests/test_stream_abi.py's --phred64 run with --overlapped_out, the seventh stream from the device: the formatter
    copies the qualities the device converted"""
    import synth
    d = synth.synth_pairs(n, L=150, seed=96, insert_mean=120.0, insert_sd=30.0)
    q64 = {}
    for m in ("1", "2"):
        q = d["qual" + m]
        body = q >= 33
        hi = q.copy()
        hi[body] = np.minimum(q[body] + 31, 126)
        q64[m] = hi
        conv = hi.copy()
        conv[body] = np.maximum(33, hi[body].astype(np.int32) - 31).astype(q.dtype)
        d["qual" + m] = conv
    a1, a2 = synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1), synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2)
    b1, b2 = synth.to_fastq(d["seq1"], q64["1"], d["len1"], 1), synth.to_fastq(d["seq2"], q64["2"], d["len2"], 2)
    ov = golden_util.params_for("pe_overlapped_out_noadapter", max_len=152)
    ov.dup_enabled = 0
    ov.correction = 1
    streams = ("out1", "out2", "failed", "overlapped")
    p1, p2 = _files(tmp_path, a1, a2)
    want = streamlib.run_files(lib, ov, p1, p2, str(tmp_path), chunk_bytes=chunk_bytes, want=streams)   # host path, phred33 text
    p1, p2 = _files(tmp_path, b1, b2)
    got = streamlib7.run_files(lib, ov, p1, p2, str(tmp_path), chunk_bytes=chunk_bytes, want=streams, phred64=True, overlapped="fd")
    body = [ln for ln in want[0]["overlapped"].split(b"\n")[3::4] if ln]
    assert len(body) > 100 and got[5]["on_device"] == 1
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


def test_sim_stream_overlapped_on_device_phred64(tmp_path):
    _phred64_case(engine.load_library(engines.build_sim()), tmp_path, 60000)


def test_sim_stream_overlapped_on_device_without_replay_or_other_streams(tmp_path):
    """no host glue object (the records then stay on the device) and no other stream wanted: the seventh alone"""
    lib = engine.load_library(engines.build_sim())
    name = "pe_overlapped_out_noadapter"
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    p1, p2 = _files(tmp_path, fq1, fq2)
    outs, _, _, _, st, info = streamlib7.run_files(lib, params, p1, p2, str(tmp_path), want=("overlapped",), chunk_bytes=60000,
                                                   overlapped="fd", with_host=False)
    from driver import md5
    assert info["on_device"] == 1 and md5(outs["overlapped"]) == meta["outputs"]["overlapped"]["md5"]


# ---- A7: switches -------------------------------------------------------------------------------------------------
def test_sim_stream_overlapped_switches(tmp_path, monkeypatch):
    lib = engine.load_library(engines.build_sim())
    name = "pe_overlapped_out_noadapter"
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    p1, p2 = _files(tmp_path, fq1, fq2)
    want = list(meta["outputs"])
    monkeypatch.setenv("FASTP_GPU_STREAM_OVERLAPPED", "device")
    outs, ctr, lay, amaps, st = streamlib.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=60000)
    golden_util.check_against_golden(name, streamlib.as_outputs(outs, True), streamlib.report(ctr, lay, params, amaps), meta)
    info = streamlib7.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=60000, overlapped=None)[5]
    assert info["on_device"] == 1      # the variable alone chose the device path
    monkeypatch.setenv("FASTP_GPU_STREAM_OVERLAPPED", "host")
    info = streamlib7.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=60000, overlapped=None)[5]
    assert info["on_device"] == 0
    monkeypatch.setenv("FASTP_GPU_STREAM_OVERLAPPED", "bogus")
    with pytest.raises(streamlib.StreamError) as e:
        streamlib.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=60000)
    assert e.value.code == abi.E_INVALID
    monkeypatch.delenv("FASTP_GPU_STREAM_OVERLAPPED")
    # the setter once the run has started
    info = streamlib7.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=60000, overlapped="emit", setter_after_run=True)[5]
    assert info["late_rc"] == abi.E_INVALID and info["on_device"] == 0
    # ... and on a stream without want_overlapped
    plain = golden_util.params_for("pe_default", max_len=152)
    with pytest.raises(streamlib.StreamError) as e:
        streamlib7.run_files(lib, plain, p1, p2, str(tmp_path), chunk_bytes=60000, overlapped="emit")
    assert e.value.code == abi.E_INVALID


def test_sim_six_stream_call_still_refuses_overlapped_out():
    params, fq1, fq2, umi = f7.inputs("pe_overlapped_out", 64)
    g = engines.sim_engine(params)
    rc, got, lens = format_util.run_streams(g, format_util.NumpyMem(), params, fq1, fq2, 150)
    g.close()
    assert rc == abi.E_UNSUPPORTED and sum(lens) == 0


# ---- A8: the patched reference with the device path ---------------------------------------------------------------
# (the binding reads FASTP_GPU_STREAM_OVERLAPPED as a number - 0 sends --overlapped_out runs to pack mode - so it gets "1",
# which the stream takes as "device")
DEVICE_ENV = {"FASTP_GPU_STREAM_OVERLAPPED": "1"}


@pytest.mark.parametrize("name", OVERLAPPED_BINDING_CASES)
def test_patched_reference_overlapped_on_device_on_emulator(name, tmp_path):
    if not rb._ensure_built() or not os.path.exists(rb.REF_SIM):
        pytest.skip("reference binaries not built")
    rb._check(name, rb.REF_SIM, 600, tmp_path, seed=41, extra_env=DEVICE_ENV)


# ---- -m gpu -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.twin("test_sim_all_seven_streams_equal_host_writer")
@pytest.mark.parametrize("set_name", SET_NAMES)
def test_gpu_all_seven_streams_equal_host_writer(set_name):
    _a1(engines.gpu_engine, format_util.TorchMem(), set_name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_all_seven_streams_over_all_edge_sizes")
def test_gpu_all_seven_streams_over_all_edge_sizes():
    _a2_sizes(engines.gpu_engine, format_util.TorchMem, EDGE_SIZES)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_overlapped_on_device_equals_reference_golden")
@pytest.mark.parametrize("how", ["fd", "gz"])
@pytest.mark.parametrize("name", DEVICE_GOLDENS)
def test_gpu_stream_overlapped_on_device_equals_reference_golden(name, how, tmp_path):
    _golden7(engine.load_library(), name, tmp_path, 1 << 20, how)


@pytest.mark.gpu
@pytest.mark.twin("test_patched_reference_overlapped_on_device_on_emulator")
@pytest.mark.parametrize("name", OVERLAPPED_BINDING_CASES)
def test_gpu_patched_reference_overlapped_on_device(name, tmp_path):
    if not (os.path.exists(rb.REF) and os.path.exists(rb.REF_GPU)):
        pytest.skip("oracle/_ref binaries did not travel to this box")
    rb._check(name, rb.REF_GPU, 3000, tmp_path, seed=48, threads=3, extra_env=DEVICE_ENV)


def _pipeline_case(tmp_path, gz):
    """FastqPipeline.run writes all seven files of an --overlapped_out run"""
    from driver import md5
    from fastp_amd.pipeline import FastqPipeline, PipelineError
    name = "pe_merge_overlapped_out_trims"
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    p1, p2 = _files(tmp_path, fq1, fq2)
    ext = ".fq.gz" if gz else ".fq"
    path = {k: os.path.join(str(tmp_path), k + ext) for k in ("out1", "out2", "failed", "merged", "overlapped")}
    pipe = FastqPipeline(params, device=0, chunk_bytes=1 << 20)
    try:
        with pytest.raises(PipelineError):
            pipe.run(p1, p2, path["out1"], path["out2"], failed_out=path["failed"], merged_out=path["merged"])
        pipe.run(p1, p2, path["out1"], path["out2"], failed_out=path["failed"], merged_out=path["merged"],
                 overlapped_out=path["overlapped"])
    finally:
        pipe.close()
    for k, exp in meta["outputs"].items():
        raw = open(path[k], "rb").read()
        got = gzip.decompress(raw) if gz else raw
        assert md5(got) == exp["md5"], f"{k}: {len(got)} bytes, the reference wrote {exp['size']}"
        assert not gz or raw[-28:] == streamlib7.BGZF_EOF
    assert "overlapped" in meta["outputs"] and meta["outputs"]["overlapped"]["size"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_gpu_pipeline_overlapped_out(gz, tmp_path):
    _pipeline_case(tmp_path, gz)
