"""streamlib.run_files with --overlapped_out's stream on the device path of include/fastp_gpu_stream.h
(fastp_gpu_stream_set_overlapped_output): to a file descriptor, plain or compressed, or through the emit callback"""
import ctypes as C
import os

import numpy as np

import cpphost
from fastp_amd import abi
from streamlib import EMIT_FN, N_OUT, STREAM_NAMES, StreamConfig, StreamError, StreamStats

OVERLAPPED = 6
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _protos(lib):
    lib.fastp_gpu_stream_last_error.restype = C.c_char_p
    lib.fastp_gpu_stream_last_error.argtypes = [C.c_void_p]
    lib.fastp_gpu_stream_create.argtypes = [C.POINTER(abi.Params), C.POINTER(StreamConfig), C.POINTER(C.c_void_p)]
    lib.fastp_gpu_stream_run.argtypes = [C.c_void_p]
    lib.fastp_gpu_stream_destroy.argtypes = [C.c_void_p]
    lib.fastp_gpu_stream_layout.argtypes = [C.c_void_p, C.POINTER(abi.CounterLayout)]
    lib.fastp_gpu_stream_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.fastp_gpu_stream_get_stats.argtypes = [C.c_void_p, C.POINTER(StreamStats)]
    lib.fastp_gpu_stream_set_overlapped_output.restype = C.c_int
    lib.fastp_gpu_stream_set_overlapped_output.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int]
    lib.fastp_gpu_stream_overlapped_on_device.restype = C.c_int
    lib.fastp_gpu_stream_overlapped_on_device.argtypes = [C.c_void_p]


def run_files(lib, params: abi.Params, in1, in2, outdir, want=("out1", "out2", "failed"), chunk_bytes=0, umi=None,
              overlapped="fd", device=0, phred64=False, with_host=True, setter_after_run=False):
    """overlapped: "fd" | "gz" (an fd, compressed) | "emit" | None (the setter is not called).
    returns (outputs: name -> bytes as written, counters, layout, AdapterMaps | None, StreamStats, info dict)"""
    _protos(lib)
    paired = bool(params.paired)
    host = cpphost.CppHost(lib, params, "failed" in want, "unpaired1" in want, umi) if with_host else None
    cfg = StreamConfig()
    cfg.in1 = in1.encode()
    cfg.in2 = in2.encode() if in2 else None
    cfg.chunk_bytes = chunk_bytes
    cfg.device = device
    cfg.phred64 = int(phred64)
    cfg.format.want_failed = int("failed" in want)
    cfg.format.want_unpaired1 = int("unpaired1" in want)
    cfg.format.want_unpaired2 = int("unpaired2" in want)
    if umi is not None:
        cfg.format.umi_loc, cfg.format.umi_len = cpphost.UMI_LOC[umi.loc], umi.umi_len
        cfg.format.umi_prefix = umi.prefix or None
        cfg.format.umi_delimiter = umi.delimiter
    cfg.want_overlapped = int(bool(params.overlapped_out) and "overlapped" in want)
    fds, paths, collected, calls = {}, {}, {q: bytearray() for q in range(N_OUT + 1)}, {q: 0 for q in range(N_OUT + 1)}
    for q, name in enumerate(STREAM_NAMES):
        cfg.out_fd[q] = -1
        if name not in want or (not paired and q in (1, 3, 4, 5)):
            continue
        cfg.want[q] = 1
        paths[q] = os.path.join(outdir, name + ".fq")
        fds[q] = os.open(paths[q], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        cfg.out_fd[q] = fds[q]

    def on_emit(user, stream, data, n):
        collected[stream] += C.string_at(data, n) if n else b""
        calls[stream] += 1
        return 0
    cb = EMIT_FN(on_emit)
    cfg.emit = cb
    cfg.host = host.h if host else None
    s = C.c_void_p()
    rc = lib.fastp_gpu_stream_create(C.byref(params), C.byref(cfg), C.byref(s))
    if rc != 0:
        if host:
            host.close()
        for fd in fds.values():
            os.close(fd)
        raise StreamError(rc, (lib.fastp_gpu_stream_last_error(None) or b"").decode())
    info = {}
    try:
        if overlapped in ("fd", "gz"):
            paths[OVERLAPPED] = os.path.join(outdir, "overlapped.fq" + (".gz" if overlapped == "gz" else ""))
            fds[OVERLAPPED] = os.open(paths[OVERLAPPED], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        if overlapped is not None and not setter_after_run:
            rc = lib.fastp_gpu_stream_set_overlapped_output(s, fds.get(OVERLAPPED, -1), 0, int(overlapped == "gz"))
            if rc != 0:
                raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        info["on_device"] = lib.fastp_gpu_stream_overlapped_on_device(s)
        rc = lib.fastp_gpu_stream_run(s)
        if rc != 0:
            raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        if setter_after_run:
            info["late_rc"] = lib.fastp_gpu_stream_set_overlapped_output(s, fds.get(OVERLAPPED, -1), 0, 0)
        lay = abi.CounterLayout()
        assert lib.fastp_gpu_stream_layout(s, C.byref(lay)) == 0
        ctr = np.zeros(lay.total, dtype=np.int64)
        rc = lib.fastp_gpu_stream_counters(s, ctr.ctypes.data, lay.total)
        if rc != 0:
            raise StreamError(rc, (lib.fastp_gpu_stream_last_error(s) or b"").decode())
        st = StreamStats()
        lib.fastp_gpu_stream_get_stats(s, C.byref(st))
        amaps = host.adapter_maps() if host else None
    finally:
        lib.fastp_gpu_stream_destroy(s)
        if host:
            host.close()
        for fd in fds.values():
            os.close(fd)
    outs = {}
    for q, name in enumerate(STREAM_NAMES):
        if cfg.want[q]:
            outs[name] = open(paths[q], "rb").read()
    if cfg.want_overlapped:
        outs["overlapped"] = open(paths[OVERLAPPED], "rb").read() if OVERLAPPED in paths else bytes(collected[OVERLAPPED])
        assert st.bytes_overlapped == len(outs["overlapped"])
    info["emit_calls"] = calls[OVERLAPPED]
    return outs, ctr, lay, amaps, st, info
