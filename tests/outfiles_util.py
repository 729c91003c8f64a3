"""--stdout / --split through the file loop (include/fastp_gpu_stream.h: fastp_gpu_stream_set_interleaved_output,
fastp_gpu_stream_set_split): the cases of tests/golden/output_files/ (written by tests/golden/make_golden_output_files.py
from the real reference, -w 1) and a streamlib-style runner that returns every file the run wrote."""
import ctypes as C
import gzip
import hashlib
import json
import os

import numpy as np

import cases
import cpphost
import synth
from fastp_amd import abi, hostloop
from streamlib import EMIT_FN, N_OUT, STREAM_NAMES, StreamConfig, StreamError, StreamStats

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "output_files")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# name -> dict(base: case of tests/cases.py (flags, parameters, synth options), n: units, seed,
#              extra: parameter fields on top, flags: reference flags on top,
#              split: ("lines", L) | ("files", N) | None, digits, gz: ".gz" outputs,
#              stdout: --stdout, want: the other streams given, drop_flags: flags of the base case left out,
#              short_units: (a, b) - read 1 of units [a, b) is cut to 30 bases, no other read is shorter than 45;
#              long_only: no read is shorter than 45 (an empty read fails with the filters off too))
CASES = {
    "split_se_lines": dict(base="se_adapter_cut", n=3200, split=("lines", 4000)),
    # (1000 reads per file and three packs: a third file exists only if packs 1 and 2 pass whole, so the reads that fail - read 1
    # cut to 30 bases, under -l 40 - all lie in pack 3)
    "split_pe_lines_gz": dict(base="pe_nofilters", n=3000, split=("lines", 4000), gz=True, short_units=(2100, 2400),
                              extra=dict(length_filter=1, length_required=40, adapter_enabled=0), flags=["-l", "40", "-A"], drop_flags=["-L"]),
    # (four packs, reads fail in every one: the packs' passed counts, not their units, put the cuts behind packs 2 and 4)
    "split_pe_lines_gz_early": dict(base="pe_default", n=3200, split=("lines", 4000), gz=True),
    "split_pe_files5": dict(base="pe_default", n=3200, split=("files", 5), digits=2),
    "split_se_files2": dict(base="se_default_noadapter", n=2300, split=("files", 2), digits=0),
    "split_pe_nofilters_lines": dict(base="pe_nofilters", n=2000, split=("lines", 4000), long_only=True),
    "stdout_pe_failed_unpaired1": dict(base="pe_filters", n=500, stdout=True, want=("failed", "unpaired1")),
    "stdout_pe_dedup_umi": dict(base="pe_umi_per_read", n=500, stdout=True, extra=dict(dedup=1, dup_accuracy_level=3), flags=["--dedup"],
                                synth=dict(dup_frac=0.3)),
    "stdout_se": dict(base="se_adapter_cut", n=500, stdout=True),
    "stdout_pe_merge": dict(base="pe_merge", n=500, stdout=True, drop_flags=["--merged_out", "@TMP@/merged.fq"],
                            synth=dict(insert_mean=70.0, insert_sd=10.0)),     # (reads of 50 bases that overlap)
}
SPLIT_CASES = [k for k, v in CASES.items() if v.get("split")]
STDOUT_CASES = [k for k, v in CASES.items() if v.get("stdout")]
L = 50


def md5(b):
    return hashlib.md5(b).hexdigest()


def case_input(name):
    """(fq1, fq2 | None) of a case: synth.synth_pairs(L=50)"""
    c = CASES[name]
    paired, _, _, skw = cases.CASES[c["base"]]
    kw = dict(skw)
    kw.update(c.get("synth", {}))
    d = synth.synth_pairs(c["n"], L=L, seed=c.get("seed", 4321), paired=paired, **kw)
    if "short_units" in c or c.get("long_only"):
        # the generator's own short reads (small inserts) would fail -l anywhere: every unit with one becomes a copy of the last
        # unit in front of it that has none (the names, made from the index, stay distinct)
        a, b = c.get("short_units", (0, 0))
        good = (d["len1"] >= 45) & (d["len2"] >= 45)
        assert good[0]
        src = np.maximum.accumulate(np.where(good, np.arange(c["n"]), 0))
        for k in ("seq1", "qual1", "len1", "seq2", "qual2", "len2"):
            d[k] = d[k][src].copy()
        d["len1"][a:b] = 30
    fq1 = synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1)
    fq2 = synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2) if paired else None
    return fq1, fq2


def case_params(name, max_len=56):
    c = CASES[name]
    p = cases.CASES[c["base"]][2](max_len)
    for k, v in c.get("extra", {}).items():
        setattr(p, k, v)
    return p


def case_umi(name):
    base = CASES[name]["base"]
    return hostloop.UmiNameEditor(*cases.UMI[base]) if base in cases.UMI else None


def reads_per_file(name):
    """the reference's split.size: lines / 4, or the input's reads / N (options.cpp:332-348; Evaluator::evaluateReadNum counts
    inputs of this size exactly)"""
    c = CASES[name]
    how, v = c["split"]
    return v // 4 if how == "lines" else max(1, c["n"] // v)


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    meta = json.loads(z["meta"].tobytes().decode())
    return z["fq1"].tobytes(), (z["fq2"].tobytes() if "fq2" in z.files else None), meta


def text_of(name, raw):
    return gzip.decompress(raw) if name.endswith(".gz") and raw else raw


def _protos(lib):
    lib.fastp_gpu_stream_last_error.restype = C.c_char_p
    lib.fastp_gpu_stream_last_error.argtypes = [C.c_void_p]
    lib.fastp_gpu_stream_create.argtypes = [C.POINTER(abi.Params), C.POINTER(StreamConfig), C.POINTER(C.c_void_p)]
    for fn in (lib.fastp_gpu_stream_run, lib.fastp_gpu_stream_destroy):
        fn.argtypes = [C.c_void_p]
    lib.fastp_gpu_stream_layout.argtypes = [C.c_void_p, C.POINTER(abi.CounterLayout)]
    lib.fastp_gpu_stream_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.fastp_gpu_stream_get_stats.argtypes = [C.c_void_p, C.POINTER(StreamStats)]
    lib.fastp_gpu_stream_set_interleaved_output.restype = C.c_int
    lib.fastp_gpu_stream_set_interleaved_output.argtypes = [C.c_void_p, C.c_int]
    lib.fastp_gpu_stream_set_split.restype = C.c_int
    lib.fastp_gpu_stream_set_split.argtypes = [C.c_void_p, C.POINTER(StreamSplit)]
    lib.fastp_gpu_stream_split_files.restype = C.c_int32
    lib.fastp_gpu_stream_split_files.argtypes = [C.c_void_p]


class StreamSplit(C.Structure):
    """fastp_gpu_stream_split"""
    _fields_ = [("by_lines", C.c_int32), ("reads_per_file", C.c_int64), ("number", C.c_int32), ("digits", C.c_int32),
                ("out1", C.c_char_p), ("out2", C.c_char_p)]


def run(lib, params, in1, in2, outdir, want=(), chunk_bytes=0, umi=None, interleaved_out=False, split=None, gz=False,
        reads_to_process=0, device=0, after_run=None):
    """the file loop with the two setters.  want: streams with a file of their own (outdir/<name>.fq);
    interleaved_out: fastp_gpu_stream_set_interleaved_output (out1 must be in want);
    split: dict(by_lines, reads_per_file, number, digits) - the files are outdir/<k>.o1.fq[.gz] [and <k>.o2.fq[.gz]].
    after_run(lib, s): called behind fastp_gpu_stream_run (late setter calls).
    returns (files: name -> bytes as written, counters, layout, AdapterMaps, StreamStats, info)"""
    _protos(lib)
    paired = bool(params.paired)
    host = cpphost.CppHost(lib, params, "failed" in want, "unpaired1" in want, umi)
    cfg = StreamConfig()
    cfg.in1 = in1.encode()
    cfg.in2 = in2.encode() if in2 else None
    cfg.chunk_bytes = chunk_bytes
    cfg.device = device
    cfg.reads_to_process = reads_to_process
    cfg.format.want_failed = int("failed" in want)
    cfg.format.want_unpaired1 = int("unpaired1" in want)
    cfg.format.want_unpaired2 = int("unpaired2" in want)
    cfg.want_overlapped = int("overlapped" in want)   # (--overlapped_out's stream, through the emit callback)
    if umi is not None:
        cfg.format.umi_loc, cfg.format.umi_len = cpphost.UMI_LOC[umi.loc], umi.umi_len
        cfg.format.umi_prefix = umi.prefix or None
        cfg.format.umi_delimiter = umi.delimiter
    fds, paths = {}, {}
    for q, name in enumerate(STREAM_NAMES):
        cfg.out_fd[q] = -1
        if name not in want:
            continue
        cfg.want[q] = 1
        paths[name] = os.path.join(outdir, name + ".fq")
        fds[q] = os.open(paths[name], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        cfg.out_fd[q] = fds[q]
    if split is not None and gz:
        cfg.compress[0] = cfg.compress[1] = 1
    cb = EMIT_FN(lambda user, stream, data, n: 0)
    cfg.emit = cb
    cfg.host = host.h
    s = C.c_void_p()
    rc = lib.fastp_gpu_stream_create(C.byref(params), C.byref(cfg), C.byref(s))
    if rc != 0:
        host.close()
        for fd in fds.values():
            os.close(fd)
        raise StreamError(rc, (lib.fastp_gpu_stream_last_error(None) or b"").decode())
    info = {}
    before = set(os.listdir(outdir))
    try:
        if interleaved_out:
            rc = lib.fastp_gpu_stream_set_interleaved_output(s, 1)
            if rc != 0:
                raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        if split is not None:
            ext = ".fq.gz" if gz else ".fq"
            sp = StreamSplit()
            sp.by_lines, sp.reads_per_file = int(split["by_lines"]), split["reads_per_file"]
            sp.number, sp.digits = split.get("number", 0), split.get("digits", 4)
            sp.out1 = os.path.join(outdir, "o1" + ext).encode() if split.get("out1", True) else None
            sp.out2 = os.path.join(outdir, "o2" + ext).encode() if paired and split.get("out2", True) else None
            rc = lib.fastp_gpu_stream_set_split(s, C.byref(sp))
            if rc != 0:
                raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        rc = lib.fastp_gpu_stream_run(s)
        if rc != 0:
            raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        if after_run:
            info["late"] = after_run(lib, s)
        info["split_files"] = lib.fastp_gpu_stream_split_files(s)
        lay = abi.CounterLayout()
        assert lib.fastp_gpu_stream_layout(s, C.byref(lay)) == 0
        ctr = np.zeros(lay.total, dtype=np.int64)
        rc = lib.fastp_gpu_stream_counters(s, ctr.ctypes.data, lay.total)
        if rc != 0:
            raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        st = StreamStats()
        lib.fastp_gpu_stream_get_stats(s, C.byref(st))
        amaps = host.adapter_maps()
    finally:
        lib.fastp_gpu_stream_destroy(s)
        host.close()
        for fd in fds.values():
            os.close(fd)
    files = {}
    for name, path in paths.items():
        files[name + ".fq"] = open(path, "rb").read()
    for fn in sorted(set(os.listdir(outdir)) - before):
        files[fn] = open(os.path.join(outdir, fn), "rb").read()
    return files, ctr, lay, amaps, st, info
