"""Helpers of tests/test_adapter_census.py: hand the adapter census (fastp_gpu_adapter_census, csrc/fq_census.h) records
and text the way the formatter gets them, and replay the same records through hostloop.apply_results - the literal
port of the reference's FilterResult::addAdapterTrimmed - for the expected maps."""
import ctypes as C

import numpy as np

from fastp_amd import abi, hostloop


def record(front=0, length=0, flags=0, adapter_pos=0, adapter_len=0, code=0):
    r = np.zeros(1, dtype=abi.READ_RESULT_DTYPE)
    r["front"], r["len"], r["code"], r["flags"] = front, length, code, flags
    r["adapter_pos"], r["adapter_len"] = adapter_pos, adapter_len
    return r[0]


def records(rows):
    out = np.zeros(len(rows), dtype=abi.READ_RESULT_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def fastq_text(seqs, tag=b"r"):
    """four-line records over the given sequence lines, with the parser's line tables"""
    parts, off, ln = [], [], []
    at = 0
    for i, s in enumerate(seqs):
        for line in (b"@" + tag + b"%d" % i, bytes(s), b"+", b"I" * len(s)):
            off.append(at)
            ln.append(len(line))
            parts.append(line + b"\n")
            at += len(line) + 1
    return b"".join(parts), np.array(off, dtype=np.uint32), np.array(ln, dtype=np.uint32)


class _Dev:
    """device copies that live for one call"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, data):
        a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data)
        raw = a.view(np.uint8).reshape(-1)
        p = self.eng.device_alloc(max(16, raw.size))
        self.ptrs.append(p)
        if raw.size:
            self.eng.device_upload(p, raw)
        return p

    def free(self):
        for p in self.ptrs:
            self.eng.device_free(p)
        self.ptrs = []


def census(eng, seqs1, r1, seqs2=None, r2=None, corrections=None, events=None, corr_capacity=None, ev_capacity=None,
           n_corr=None, n_events=None, interleaved=False, check=True):
    """one fastp_gpu_adapter_census call over hand-built units.  n_corr / n_events: what the lists' counters say (default:
    their lengths); interleaved: both mates' tables point into ONE text.  Returns the call's return code."""
    paired = seqs2 is not None
    n = len(seqs1)
    d = _Dev(eng)
    try:
        if interleaved and paired:
            both = [s for pr in zip(seqs1, seqs2) for s in pr]
            text, off, ln = fastq_text(both)
            off, ln = off.reshape(n, 2, 4), ln.reshape(n, 2, 4)
            tp = d.put(text)
            mates = [(tp, np.ascontiguousarray(off[:, m].reshape(-1)), np.ascontiguousarray(ln[:, m].reshape(-1))) for m in (0, 1)]
        else:
            mates = []
            for s in ((seqs1, seqs2) if paired else (seqs1,)):
                text, off, ln = fastq_text(s)
                mates.append((d.put(text), off, ln))
        ins = []
        for (tp, off, ln), res in zip(mates, (r1, r2)):
            f = abi.FormatIn()
            f.text, f.line_off, f.line_len, f.res = tp, d.put(off), d.put(ln), d.put(res)
            ins.append(f)
        corr = np.zeros(0, dtype=abi.CORRECTION_DTYPE) if corrections is None else corrections
        ev = np.zeros(0, dtype=abi.ADAPTER_EVENT_DTYPE) if events is None else events
        cp, ep = d.put(corr), d.put(ev)
        ncp = d.put(np.array([len(corr) if n_corr is None else n_corr], dtype=np.int32))
        nep = d.put(np.array([len(ev) if n_events is None else n_events], dtype=np.int32))
        return eng.adapter_census(n, ins[0], ins[1] if paired else None, cp, ncp,
                                  len(corr) if corr_capacity is None else corr_capacity, ep, nep,
                                  len(ev) if ev_capacity is None else ev_capacity, check=check)
    finally:
        d.free()


def replay(params, amaps, seqs1, r1, seqs2=None, r2=None, corrections=None, events=None):
    """the same units through hostloop.apply_results: amaps (hostloop.AdapterMaps) is updated in place"""
    paired = seqs2 is not None
    st = max(8, (max(len(s) for s in list(seqs1) + (list(seqs2) if paired else [])) + 7) // 8 * 8)
    b1 = hostloop.parse_fastq(fastq_text(seqs1)[0], st)
    b2 = hostloop.parse_fastq(fastq_text(seqs2)[0], st) if paired else None
    outs = hostloop.Outputs(paired, True)
    pair = np.zeros(len(seqs1), dtype=abi.PAIR_RESULT_DTYPE) if paired else None
    ev = None if events is None else np.sort(events, order=["read", "adapter"])
    hostloop.apply_results(params, b1, b2, r1, r2, pair, corrections, outs, amaps, None, adapter_events=ev)
    return amaps


def maps_of(eng):
    return eng.adapter_counts(False), eng.adapter_counts(True)


def stream_run(lib, params, in1, in2, outdir, census=None, chunk_bytes=0, umi=None, with_host=True, late_setter=False):
    """streamlib.run_files with the adapter census chosen through fastp_gpu_stream_set_adapter_census (census None: the call
    is not made - FASTP_GPU_STREAM_ADAPTERS or the default decides).  Returns (outputs, counters, layout, the host object's
    AdapterMaps or None, stats, {"entries": the two maps through fastp_gpu_stream_adapter_entry, "set_rc", "late_rc"})"""
    import os

    import cpphost
    import streamlib as SL
    paired = bool(params.paired)
    lib.fastp_gpu_stream_last_error.restype = C.c_char_p
    lib.fastp_gpu_stream_last_error.argtypes = [C.c_void_p]
    host = cpphost.CppHost(lib, params, True, False, umi) if with_host else None
    cfg = SL.StreamConfig()
    cfg.in1, cfg.in2 = in1.encode(), (in2.encode() if in2 else None)
    cfg.chunk_bytes = chunk_bytes
    cfg.format.want_failed = 1
    if umi is not None:
        cfg.format.umi_loc, cfg.format.umi_len = cpphost.UMI_LOC[umi.loc], umi.umi_len
        cfg.format.umi_prefix = umi.prefix or None
        cfg.format.umi_delimiter = umi.delimiter
    fds, paths = {}, {}
    for q, name in enumerate(SL.STREAM_NAMES):
        cfg.out_fd[q] = -1
        if name in ("out1", "failed") or (paired and name == "out2"):
            cfg.want[q] = 1
            paths[q] = os.path.join(outdir, name + ".fq")
            fds[q] = os.open(paths[q], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            cfg.out_fd[q] = fds[q]
    cfg.host = host.h if host else None
    s = C.c_void_p()
    lib.fastp_gpu_stream_create.argtypes = [C.POINTER(abi.Params), C.POINTER(SL.StreamConfig), C.POINTER(C.c_void_p)]
    rc = lib.fastp_gpu_stream_create(C.byref(params), C.byref(cfg), C.byref(s))
    if rc != 0:
        if host:
            host.close()
        for fd in fds.values():
            os.close(fd)
        raise SL.StreamError(rc, (lib.fastp_gpu_stream_last_error(None) or b"").decode())
    info = {}
    try:
        setter = lib.fastp_gpu_stream_set_adapter_census
        setter.restype, setter.argtypes = C.c_int, [C.c_void_p, C.c_int]
        if census is not None and not late_setter:
            info["set_rc"] = setter(s, int(census))
        lib.fastp_gpu_stream_run.argtypes = [C.c_void_p]
        rc = lib.fastp_gpu_stream_run(s)
        if rc != 0:
            raise SL.StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        if late_setter:
            info["late_rc"] = setter(s, int(census))
        lay = abi.CounterLayout()
        lib.fastp_gpu_stream_layout.argtypes = [C.c_void_p, C.POINTER(abi.CounterLayout)]
        assert lib.fastp_gpu_stream_layout(s, C.byref(lay)) == 0
        ctr = np.zeros(lay.total, dtype=np.int64)
        lib.fastp_gpu_stream_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        assert lib.fastp_gpu_stream_counters(s, ctr.ctypes.data, lay.total) == 0
        st = SL.StreamStats()
        lib.fastp_gpu_stream_get_stats.argtypes = [C.c_void_p, C.POINTER(SL.StreamStats)]
        lib.fastp_gpu_stream_get_stats(s, C.byref(st))
        count = lib.fastp_gpu_stream_adapter_entries
        count.restype, count.argtypes = C.c_int64, [C.c_void_p, C.c_int]
        entry = lib.fastp_gpu_stream_adapter_entry
        entry.restype = C.c_int
        entry.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        info["entries"] = []
        for m in (0, 1):
            d = {}
            for i in range(count(s, m)):
                sp, ln, cnt = C.c_void_p(), C.c_int32(), C.c_int64()
                assert entry(s, m, i, C.byref(sp), C.byref(ln), C.byref(cnt)) == 0
                d[C.string_at(sp.value, ln.value)] = int(cnt.value)
            assert entry(s, m, count(s, m), None, None, None) != 0
            info["entries"].append(d)
        amaps = host.adapter_maps() if host else None
    finally:
        lib.fastp_gpu_stream_destroy.argtypes = [C.c_void_p]
        lib.fastp_gpu_stream_destroy(s)
        if host:
            host.close()
        for fd in fds.values():
            os.close(fd)
    outs = {SL.STREAM_NAMES[q]: open(pth, "rb").read() for q, pth in paths.items()}
    return outs, ctr, lay, amaps, st, info
