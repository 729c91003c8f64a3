"""Python host mirror of the engine: thin ctypes layer over libfastp_gpu.so (the C ABI of
include/fastp_gpu.h).  No computation happens here, and there is NO CPU fallback: if the HIP
library is missing or no MI355X is visible, construction fails loudly."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_PKG, "libfastp_gpu.so")
_LIBS: dict[str, C.CDLL] = {}

EXPORTS = [
    "fastp_gpu_default_params", "fastp_gpu_seq_stride", "fastp_gpu_qual_stride", "fastp_gpu_cycles_for",
    "fastp_gpu_counter_layout_for", "fastp_gpu_counter_layout_for_params", "fastp_gpu_create", "fastp_gpu_destroy", "fastp_gpu_last_error",
    "fastp_gpu_pack_reads", "fastp_gpu_pack_reads_x", "fastp_gpu_bgzf_index", "fastp_gpu_inflate_bgzf", "fastp_gpu_parse_fastq", "fastp_gpu_parse_exotic", "fastp_gpu_phred64_to_33", "fastp_gpu_host_writes_overlapped", "fastp_gpu_format_fastq", "fastp_gpu_format_streams", "fastp_gpu_format_all_streams", "fastp_gpu_format_interleaved", "fastp_gpu_format_pack_cuts", "fastp_gpu_deflate_bgzf", "fastp_gpu_deflate_bgzf_level", "fastp_gpu_deflate_bgzf_segments", "fastp_gpu_adapter_census", "fastp_gpu_adapter_census_size", "fastp_gpu_adapter_census_read", "fastp_gpu_adapter_census_load", "fastp_gpu_device_alloc", "fastp_gpu_device_free", "fastp_gpu_device_upload", "fastp_gpu_device_download", "fastp_gpu_eval_seq_len", "fastp_gpu_eval_adapter_kmers", "fastp_gpu_eval_overrep", "fastp_gpu_eval_known_adapters", "fastp_gpu_eval_adapter_seed", "fastp_gpu_eval_adapter_kmers_x", "fastp_gpu_eval_overrep_x", "fastp_gpu_eval_known_adapters_x", "fastp_gpu_eval_adapter_seed_x", "fastp_gpu_submit_host", "fastp_gpu_submit_device", "fastp_gpu_synchronize",
    "fastp_gpu_counters_device", "fastp_gpu_counters", "fastp_gpu_kernel_time",
    "fastp_gpu_counters_export", "fastp_gpu_counters_import",
    "fastp_gpu_dup_scan_bytes", "fastp_gpu_submit_pass1_device", "fastp_gpu_dup_bitmap_bytes", "fastp_gpu_dup_bitmap_export",
    "fastp_gpu_dup_prefix_set", "fastp_gpu_prefix_or_images", "fastp_gpu_submit_pass2_device", "fastp_gpu_stream_set_origin", "fastp_gpu_overrep_device",
    "fastp_gpu_device", "fastp_gpu_reset", "fastp_gpu_plan", "fastp_gpu_debug_overrep_plan",
    "fastp_gpu_host_alloc", "fastp_gpu_host_free", "fastp_gpu_submit_host_async", "fastp_gpu_wait", "fastp_gpu_poll",
    "fastp_gpu_comm_id", "fastp_gpu_comm_init", "fastp_gpu_comm_init_local", "fastp_gpu_comm_destroy", "fastp_gpu_allreduce",
    "fastp_gpu_exchange_dup_prefix", "fastp_gpu_comm_last_error", "fastp_gpu_dup_bitmap_import", "fastp_gpu_warmup",
    # include/fastp_gpu_host.h
    "fastp_gpu_host_create", "fastp_gpu_host_destroy", "fastp_gpu_host_apply", "fastp_gpu_host_output", "fastp_gpu_host_clear_outputs",
    "fastp_gpu_host_adapter_entries", "fastp_gpu_host_adapter_entry", "fastp_gpu_host_add_adapter", "fastp_gpu_host_add_adapter_pair", "fastp_gpu_host_set_adapter_entries",
    # include/fastp_gpu_stream.h
    "fastp_gpu_stream_create", "fastp_gpu_stream_run", "fastp_gpu_stream_layout", "fastp_gpu_stream_counters", "fastp_gpu_stream_get_stats",
    "fastp_gpu_stream_last_error", "fastp_gpu_stream_destroy", "fastp_gpu_stream_set_deflate_level", "fastp_gpu_stream_set_overlapped_output", "fastp_gpu_stream_overlapped_on_device", "fastp_gpu_stream_set_adapter_census", "fastp_gpu_stream_set_interleaved_output", "fastp_gpu_stream_set_split", "fastp_gpu_stream_split_files", "fastp_gpu_stream_adapter_entries", "fastp_gpu_stream_adapter_entry", "fastp_gpu_stream_gunzip_file", "fastp_gpu_stream_gunzip_file_mt",
]


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fastp_gpu error {code}: {msg}")
        self.code = code


def load_library(path: str | None = None) -> C.CDLL:
    path = path or os.environ.get("FASTP_GPU_LIB") or DEFAULT_LIB
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'`).  fastp_amd has no CPU fallback.")
    L = C.CDLL(path)
    L.fastp_gpu_default_params.argtypes = [C.POINTER(abi.Params), C.c_int, C.c_int]
    L.fastp_gpu_seq_stride.restype = C.c_size_t
    L.fastp_gpu_seq_stride.argtypes = [C.c_int]
    L.fastp_gpu_qual_stride.restype = C.c_size_t
    L.fastp_gpu_qual_stride.argtypes = [C.c_int]
    L.fastp_gpu_cycles_for.restype = C.c_int
    L.fastp_gpu_cycles_for.argtypes = [C.POINTER(abi.Params)]
    L.fastp_gpu_counter_layout_for.argtypes = [C.c_int, C.c_int, C.POINTER(abi.CounterLayout)]
    L.fastp_gpu_counter_layout_for_params.argtypes = [C.POINTER(abi.Params), C.POINTER(abi.CounterLayout)]
    L.fastp_gpu_counter_layout_for_params.restype = None
    L.fastp_gpu_create.restype = C.c_int
    L.fastp_gpu_create.argtypes = [C.POINTER(abi.Params), C.c_int, C.POINTER(C.c_void_p)]
    L.fastp_gpu_destroy.argtypes = [C.c_void_p]
    L.fastp_gpu_last_error.restype = C.c_char_p
    L.fastp_gpu_last_error.argtypes = [C.c_void_p]
    L.fastp_gpu_pack_reads.restype = C.c_int
    L.fastp_gpu_pack_reads.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.fastp_gpu_pack_reads_x.restype = C.c_int
    L.fastp_gpu_pack_reads_x.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    L.fastp_gpu_submit_host.restype = C.c_int
    L.fastp_gpu_submit_host.argtypes = [C.c_void_p, C.POINTER(abi.Batch), C.POINTER(abi.Results)]
    L.fastp_gpu_submit_device.restype = C.c_int
    L.fastp_gpu_submit_device.argtypes = [C.c_void_p, C.POINTER(abi.Batch), C.POINTER(abi.Results), C.c_void_p]
    L.fastp_gpu_synchronize.restype = C.c_int
    L.fastp_gpu_synchronize.argtypes = [C.c_void_p]
    L.fastp_gpu_counters_device.restype = C.c_int
    L.fastp_gpu_counters_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_void_p]
    L.fastp_gpu_counters.restype = C.c_int
    L.fastp_gpu_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    for fn in (L.fastp_gpu_counters_export, L.fastp_gpu_counters_import):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.fastp_gpu_kernel_time.restype = C.c_int
    L.fastp_gpu_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    _LIBS[path] = L
    return L


def counter_layout(params: abi.Params, lib=None) -> abi.CounterLayout:
    L = lib or load_library()
    lay = abi.CounterLayout()
    L.fastp_gpu_counter_layout_for_params(C.byref(params), C.byref(lay))
    return lay


def pack_ascii(lib, max_len, seq, qual, lens, exotic=None):
    """ASCII rows [n, stride] -> packed rows via the library's host packer.  `exotic`: uint8 [n], gets 1 where a read
    holds a letter outside ACGTN (fastp_gpu_pack_reads_x); without it such a read is an error."""
    n = int(len(lens))
    ss, qs = int(lib.fastp_gpu_seq_stride(max_len)), int(lib.fastp_gpu_qual_stride(max_len))
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    lens32 = np.ascontiguousarray(lens, dtype=np.int32)
    stride = seq.shape[1] if n else 0
    sp = (seq.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
    qp = (qual.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
    so = np.zeros((n, ss), dtype=np.uint8)
    qo = np.zeros((n, qs), dtype=np.uint8)
    lo = np.zeros(n, dtype=np.uint16)
    bad = C.c_int32(-1)
    if exotic is not None:
        rc = lib.fastp_gpu_pack_reads_x(max_len, n, sp.ctypes.data, qp.ctypes.data, lens32.ctypes.data, so.ctypes.data,
                                        qo.ctypes.data, lo.ctypes.data, C.byref(bad), exotic.ctypes.data)
    else:
        rc = lib.fastp_gpu_pack_reads(max_len, n, sp.ctypes.data, qp.ctypes.data, lens32.ctypes.data, so.ctypes.data,
                                      qo.ctypes.data, lo.ctypes.data, C.byref(bad))
    if rc != 0:
        raise EngineError(rc, f"fastp_gpu_pack_reads failed at read {bad.value}")
    return so, qo, lo


class GpuEngine:
    """One fastp run on one GPU: Stats x4 + FilterResult + Duplicate + insert-size histogram live in HBM."""

    def __init__(self, params: abi.Params, device: int = 0, lib_path: str | None = None):
        self.lib = load_library(lib_path)
        self.params = params
        h = C.c_void_p()
        rc = self.lib.fastp_gpu_create(C.byref(params), device, C.byref(h))
        if rc != 0:
            raise EngineError(rc, (self.lib.fastp_gpu_last_error(None) or b"").decode())
        self.h = h
        self.layout = counter_layout(params, self.lib)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fastp_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, (self.lib.fastp_gpu_last_error(self.h) or b"").decode())

    # -- packed host buffers -> results (H2D + kernels + D2H) ---------------------------------
    def submit_packed(self, s1, q1, l1, s2=None, q2=None, l2=None, flags=abi.BATCH_STAT_ISIZE, corr_capacity=None, exotic=None):
        # exotic: (units int32 ascending, [text1, text2], [off1, off2]) - the raw sequence bytes of the units with letters
        # outside ACGTN (fastp_gpu_batch.exotic_*)
        n = int(len(l1))
        paired = s2 is not None
        r1 = np.zeros(n, dtype=abi.READ_RESULT_DTYPE)
        r2 = np.zeros(n if paired else 0, dtype=abi.READ_RESULT_DTYPE)
        pr = np.zeros(n if paired else 0, dtype=abi.PAIR_RESULT_DTYPE)
        if corr_capacity is None:
            corr_capacity = getattr(self, "corr_capacity", None)   # (tests: a caller's list that is too small)
        if corr_capacity is None:
            corr_capacity = max(1024, n * 32)
        corr = np.zeros(corr_capacity, dtype=abi.CORRECTION_DTYPE)
        ncorr = C.c_int32(0)
        b = abi.Batch()
        b.n, b.flags = n, flags
        b.seq1, b.qual1, b.len1 = s1.ctypes.data, q1.ctypes.data, l1.ctypes.data
        if paired:
            b.seq2, b.qual2, b.len2 = s2.ctypes.data, q2.ctypes.data, l2.ctypes.data
        if exotic is not None and len(exotic[0]):
            xu, xt, xo = exotic
            b.n_exotic = len(xu)
            b.exotic_unit = xu.ctypes.data
            for m in range(2 if paired else 1):
                b.exotic_text[m] = xt[m].ctypes.data
                b.exotic_off[m] = xo[m].ctypes.data
                b.exotic_text_bytes[m] = xt[m].nbytes
        res = abi.Results()
        res.r1 = r1.ctypes.data
        res.r2 = r2.ctypes.data if paired else None
        res.pair = pr.ctypes.data if paired else None
        res.corrections = corr.ctypes.data
        res.corrections_capacity = corr_capacity
        res.n_corrections = C.addressof(ncorr)
        nfasta = int(self.params.n_adapter_fasta)
        ev = np.zeros(max(16, n * 2 * min(nfasta, 8)) if nfasta else 0, dtype=abi.ADAPTER_EVENT_DTYPE)
        nev = C.c_int32(0)
        if nfasta:
            res.adapter_events = ev.ctypes.data
            res.adapter_events_capacity = len(ev)
            res.n_adapter_events = C.addressof(nev)
        self._check(self.lib.fastp_gpu_submit_host(self.h, C.byref(b), C.byref(res)))
        # --adapter_fasta trims of this batch, per read in adapter order (the device emits them unordered)
        self.last_adapter_events = np.sort(ev[:nev.value].copy(), order=["read", "adapter"])
        return r1, (r2 if paired else None), (pr if paired else None), corr[:min(ncorr.value, corr_capacity)].copy()

    # -- ASCII rows (what the FASTQ decoder produces) -> results -------------------------------
    def process(self, seq1, qual1, len1, seq2=None, qual2=None, len2=None, flags=abi.BATCH_STAT_ISIZE):
        ml = self.params.max_len
        n = int(len(len1))
        mask = np.zeros(n, dtype=np.uint8)
        s1, q1, l1 = pack_ascii(self.lib, ml, seq1, qual1, len1, mask)
        s2 = q2 = l2 = None
        if seq2 is not None:
            s2, q2, l2 = pack_ascii(self.lib, ml, seq2, qual2, len2, mask)
        exotic = None
        if mask.any():   # letters outside ACGTN: the units' raw rows travel with the batch
            xu = np.flatnonzero(mask).astype(np.int32)
            rows = [np.ascontiguousarray(np.asarray(a, dtype=np.uint8)[xu]) for a in ((seq1, seq2) if seq2 is not None else (seq1,))]
            offs = [(np.arange(len(xu), dtype=np.uint32) * np.uint32(r.shape[1])) for r in rows]
            exotic = (xu, rows, offs)
        if seq2 is not None:
            return self.submit_packed(s1, q1, l1, s2, q2, l2, flags, exotic=exotic)
        return self.submit_packed(s1, q1, l1, flags=flags, exotic=exotic)

    # -- device-resident batches (bench / multi-GPU hosts) ---------------------------------------
    def submit_device(self, batch: abi.Batch, results: abi.Results, stream=None):
        self._check(self.lib.fastp_gpu_submit_device(self.h, C.byref(batch), C.byref(results), stream))

    # ---- sharded runs (include/fastp_gpu.h "Sharded runs") ----
    def dup_scan_bytes(self, n: int) -> int:
        fn = self.lib.fastp_gpu_dup_scan_bytes
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int32]
        return int(fn(self.h, n))

    def submit_pass1_device(self, batch: abi.Batch, scan_ptr: int, results, stream=None):
        fn = self.lib.fastp_gpu_submit_pass1_device
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Batch), C.c_void_p, C.POINTER(abi.Results), C.c_void_p]
        self._check(fn(self.h, C.byref(batch), scan_ptr, C.byref(results) if results is not None else None, stream))

    def submit_pass2_device(self, batch: abi.Batch, scan_ptr: int, results: abi.Results, stream=None):
        fn = self.lib.fastp_gpu_submit_pass2_device
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Batch), C.c_void_p, C.POINTER(abi.Results), C.c_void_p]
        self._check(fn(self.h, C.byref(batch), scan_ptr, C.byref(results), stream))

    def prefix_or_images(self, images_ptr: int, n_images: int, bytes_each: int):
        fn = self.lib.fastp_gpu_prefix_or_images
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]
        self._check(fn(self.h, images_ptr, n_images, bytes_each))

    def dup_bitmap_bytes(self) -> int:
        fn = self.lib.fastp_gpu_dup_bitmap_bytes
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
        return int(fn(self.h))

    def dup_bitmap_export(self, dst_ptr: int):
        fn = self.lib.fastp_gpu_dup_bitmap_export
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, dst_ptr))

    def dup_prefix_set(self, images_ptr, n_images: int):
        fn = self.lib.fastp_gpu_dup_prefix_set
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]
        self._check(fn(self.h, images_ptr, n_images))

    def stream_set_origin(self, units_before: int, post_reads_before: int):
        fn = self.lib.fastp_gpu_stream_set_origin
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_int64]
        self._check(fn(self.h, units_before, post_reads_before))

    def overrep_device(self, batch: abi.Batch, results: abi.Results, stream=None):
        fn = self.lib.fastp_gpu_overrep_device
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(abi.Batch), C.POINTER(abi.Results), C.c_void_p]
        self._check(fn(self.h, C.byref(batch), C.byref(results), stream))

    # ---- BGZF input (include/fastp_gpu.h) ----
    def bgzf_index(self, host_bytes: np.ndarray, max_blocks: int, max_text_bytes: int, check=True):
        """header walk over HOST bytes -> (info, pay_off, pay_len, isize, crc, out_off) numpy arrays"""
        fn = self.lib.fastp_gpu_bgzf_index
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(abi.InflateInfo)]
        arrs = [np.zeros(max(1, max_blocks), dtype=np.uint32) for _ in range(4)] + [np.zeros(max(1, max_blocks), dtype=np.uint64)]
        info = abi.InflateInfo()
        rc = fn(host_bytes.ctypes.data, host_bytes.size, max_blocks, max_text_bytes, *[a.ctypes.data for a in arrs], C.byref(info))
        if check and rc != 0:
            raise EngineError(rc, f"not a BGZF member at block {info.first_bad}")
        info.rc = rc
        return (info,) + tuple(a[:info.n_blocks] for a in arrs)

    def inflate_bgzf(self, comp_ptr, n_blocks, pay_off_ptr, pay_len_ptr, isize_ptr, crc_ptr, out_off_ptr, out_ptr, out_cap,
                     check_crc=True, check=True):
        fn = self.lib.fastp_gpu_inflate_bgzf
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
        bad = C.c_int32(-1)
        rc = fn(self.h, comp_ptr, n_blocks, pay_off_ptr, pay_len_ptr, isize_ptr, crc_ptr, out_off_ptr, out_ptr, out_cap,
                int(check_crc), C.byref(bad))
        if check:
            self._check(rc)
        return rc, int(bad.value)

    def parse_fastq(self, text_ptr: int, nbytes: int, is_last: bool, max_records: int, seq_ptr: int, qual_ptr: int,
                    len_ptr: int, line_off_ptr: int, line_len_ptr: int, check=True) -> abi.ParseInfo:
        """FASTQ text resident on the device -> packed rows on the device (fastp_gpu_parse_fastq)"""
        info = abi.ParseInfo()
        fn = self.lib.fastp_gpu_parse_fastq
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_void_p, C.POINTER(abi.ParseInfo)]
        rc = fn(self.h, text_ptr, nbytes, int(is_last), max_records, seq_ptr, qual_ptr, len_ptr, line_off_ptr,
                line_len_ptr, C.byref(info))
        if check:
            self._check(rc)
        info.rc = rc
        return info

    def parse_exotic(self) -> np.ndarray:
        """records of the last parse_fastq call with letters outside ACGTN (ascending), fastp_gpu_parse_exotic"""
        fn = self.lib.fastp_gpu_parse_exotic
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        n = int(fn(self.h, None, 0))
        out = np.zeros(max(n, 1), dtype=np.int32)
        fn(self.h, out.ctypes.data, n)
        return out[:n]

    def format_fastq(self, n, m1: abi.FormatIn, m2, corrections_ptr, n_corrections_ptr, out1_ptr, out1_cap, out2_ptr,
                     out2_cap, check=True):
        """result records + parsed text on the device -> out1 / out2 FASTQ text on the device"""
        fn = self.lib.fastp_gpu_format_fastq
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.FormatIn), C.POINTER(abi.FormatIn), C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        lens = (C.c_int64 * 2)()
        rc = fn(self.h, n, C.byref(m1), C.byref(m2) if m2 is not None else None, corrections_ptr, n_corrections_ptr,
                out1_ptr, out1_cap, out2_ptr, out2_cap, lens)
        if check:
            self._check(rc)
        return rc, int(lens[0]), int(lens[1])

    def format_streams(self, n, m1: abi.FormatIn, m2, pair_ptr, corrections_ptr, n_corrections_ptr,
                       opts: abi.FormatOptions | None, out_ptrs, out_caps, check=True):
        """every output stream of the worker loop on the device (out1, out2, failed, merged, unpaired1, unpaired2);
        corrections are patched into the mates' text.  Returns (rc, [needed bytes per stream])"""
        return self._format_n(self.lib.fastp_gpu_format_streams, abi.N_OUTPUTS, n, m1, m2, pair_ptr, corrections_ptr,
                              n_corrections_ptr, opts, out_ptrs, out_caps, check)

    def format_all_streams(self, n, m1: abi.FormatIn, m2, pair_ptr, corrections_ptr, n_corrections_ptr,
                           opts: abi.FormatOptions | None, out_ptrs, out_caps, check=True):
        """format_streams' six streams plus --overlapped_out's as the seventh (fastp_gpu_format_all_streams): lists of
        abi.N_ALL_OUTPUTS entries.  Returns (rc, [needed bytes per stream])"""
        return self._format_n(self.lib.fastp_gpu_format_all_streams, abi.N_ALL_OUTPUTS, n, m1, m2, pair_ptr, corrections_ptr,
                              n_corrections_ptr, opts, out_ptrs, out_caps, check)

    def _format_n(self, fn, ns, n, m1, m2, pair_ptr, corrections_ptr, n_corrections_ptr, opts, out_ptrs, out_caps, check):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.FormatIn), C.POINTER(abi.FormatIn), C.c_void_p, C.c_void_p,
                       C.c_void_p, C.POINTER(abi.FormatOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                       C.POINTER(C.c_int64)]
        outs = (C.c_void_p * ns)(*[p or None for p in out_ptrs])
        caps = (C.c_int64 * ns)(*out_caps)
        lens = (C.c_int64 * ns)()
        rc = fn(self.h, n, C.byref(m1), C.byref(m2) if m2 is not None else None, pair_ptr, corrections_ptr,
                n_corrections_ptr, C.byref(opts) if opts is not None else None, outs, caps, lens)
        if check:
            self._check(rc)
        return rc, [int(x) for x in lens]

    def deflate_bgzf(self, text_ptr, nbytes, out_ptr, out_capacity, write_eof=False, check=True, level=None):
        """device text -> BGZF-framed gzip members on the device; returns (rc, bytes written / needed).
        level: the reference's -z (0 = the default, 1..9) through fastp_gpu_deflate_bgzf_level; None: fastp_gpu_deflate_bgzf"""
        n = C.c_int64(0)
        if level is None:
            fn = self.lib.fastp_gpu_deflate_bgzf
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            rc = fn(self.h, text_ptr, nbytes, int(write_eof), out_ptr, out_capacity, C.byref(n))
        else:
            fn = self.lib.fastp_gpu_deflate_bgzf_level
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            rc = fn(self.h, text_ptr, nbytes, int(write_eof), int(level), out_ptr, out_capacity, C.byref(n))
        if check:
            self._check(rc)
        return rc, int(n.value)

    def format_interleaved(self, on=True, check=True):
        """--stdout's stream of a paired run: a passing pair's two records go to out1, out2 gets nothing
        (fastp_gpu_format_interleaved).  Returns rc"""
        fn = self.lib.fastp_gpu_format_interleaved
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int]
        rc = fn(self.h, int(bool(on)))
        if check:
            self._check(rc)
        return rc

    def format_pack_cuts(self, plan: abi.PackCuts | None, check=True):
        """arm the next format_streams / format_all_streams call with a pack table (fastp_gpu_format_pack_cuts);
        None disarms.  Returns rc"""
        fn = self.lib.fastp_gpu_format_pack_cuts
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.PackCuts)]
        rc = fn(self.h, C.byref(plan) if plan is not None else None)
        if check:
            self._check(rc)
        return rc

    def deflate_bgzf_segments(self, text_ptr, seg_off, seg_eof, level, out_ptr, out_capacity, check=True):
        """device text cut at seg_off (host list of n + 1 ascending offsets) -> BGZF members that never span a cut
        (fastp_gpu_deflate_bgzf_segments); seg_eof: host list of n flags or None.  Returns (rc, [n + 1 output offsets])"""
        fn = self.lib.fastp_gpu_deflate_bgzf_segments
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                       C.POINTER(C.c_int64)]
        n = len(seg_off) - 1
        offs = (C.c_int64 * (n + 1))(*[int(x) for x in seg_off])
        eof = (C.c_uint8 * max(n, 1))(*[1 if x else 0 for x in seg_eof]) if seg_eof is not None else None
        out_off = (C.c_int64 * (n + 1))()
        rc = fn(self.h, text_ptr, n, offs, eof, int(level), out_ptr, out_capacity, out_off)
        if check:
            self._check(rc)
        return rc, [int(x) for x in out_off]

    # ---- FilterResult's adapter-string maps on the device (csrc/fq_census.h) ----
    def adapter_census(self, n, m1: abi.FormatIn, m2, corrections_ptr, n_corrections_ptr, corrections_capacity,
                       events_ptr=None, n_events_ptr=None, events_capacity=0, check=True):
        """add the n units of one launch to the context's two adapter maps (fastp_gpu_adapter_census): the inputs of
        format_streams plus the --adapter_fasta event list, all DEVICE pointers; calls in stream order.  Returns rc"""
        fn = self.lib.fastp_gpu_adapter_census
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.FormatIn), C.POINTER(abi.FormatIn), C.c_void_p, C.c_void_p,
                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        rc = fn(self.h, n, C.byref(m1), C.byref(m2) if m2 is not None else None, corrections_ptr, n_corrections_ptr,
                corrections_capacity, events_ptr, n_events_ptr, events_capacity)
        if check:
            self._check(rc)
        return rc

    def adapter_counts(self, is_r2: bool) -> dict:
        """FilterResult::mAdapter1 (mAdapter2) as the census holds it: {adapter bytes: count}, in the reference's map
        order (by length, then bytes)"""
        size = self.lib.fastp_gpu_adapter_census_size
        size.restype = C.c_int
        size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        ne, nb = C.c_int64(0), C.c_int64(0)
        self._check(size(self.h, int(is_r2), C.byref(ne), C.byref(nb)))
        chars = np.zeros(max(1, nb.value), dtype=np.uint8)
        off = np.zeros(ne.value + 1, dtype=np.int64)
        cnt = np.zeros(max(1, ne.value), dtype=np.int64)
        read = self.lib.fastp_gpu_adapter_census_read
        read.restype = C.c_int
        read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        self._check(read(self.h, int(is_r2), chars.ctypes.data, chars.size, off.ctypes.data, cnt.ctypes.data))
        raw = chars.tobytes()
        return {raw[off[i]:off[i + 1]]: int(cnt[i]) for i in range(ne.value)}

    def load_adapter_counts(self, is_r2: bool, counts, check=True):
        """replace a map's contents with {adapter bytes: count} (or a list of such pairs): fastp_gpu_adapter_census_load"""
        items = list(counts.items()) if isinstance(counts, dict) else list(counts)
        chars = np.frombuffer(b"".join(k for k, _ in items) or b"\0", dtype=np.uint8)
        off = np.zeros(len(items) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(k) for k, _ in items], dtype=np.int64) if items else 0
        cnt = np.array([v for _, v in items] or [0], dtype=np.int64)
        fn = self.lib.fastp_gpu_adapter_census_load
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        rc = fn(self.h, int(is_r2), chars.ctypes.data, off.ctypes.data, cnt.ctypes.data, len(items))
        if check:
            self._check(rc)
        return rc

    # ---- the Evaluator pre-pass on the device (csrc/fq_eval.h); device pointers of one mate's packed rows ----
    def eval_seq_len(self, len_ptr, n):
        fn = self.lib.fastp_gpu_eval_seq_len
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        out = C.c_int32(0)
        self._check(fn(self.h, len_ptr, n, C.byref(out)))
        return int(out.value)

    # `exotic` (every call below): None, or (units, text_ptr, off_ptr, dense) naming the reads with letters outside ACGTN -
    # ascending int32 read indexes (HOST), the DEVICE text that holds their sequence bytes, the DEVICE offsets (dense: the
    # parser's line_off table) - which sends the call through its fastp_gpu_eval_*_x form (abi.EvalText); units None: that
    # form with a NULL list
    @staticmethod
    def _eval_text(exotic):
        """-> (abi.EvalText or None, the object that keeps its host list alive)"""
        if exotic is None:
            return None, None
        units, text_ptr, off_ptr, dense = exotic
        if units is None:             # the _x form with a NULL list: the plain call by another name
            return None, None
        units = np.ascontiguousarray(units, dtype=np.int32)
        x = abi.EvalText(len(units), int(bool(dense)), units.ctypes.data if len(units) else None, text_ptr, off_ptr)
        return x, units

    def _eval_fn(self, name, argtypes, exotic):
        """the plain entry point, or with `exotic` its _x form: (function, trailing arguments, keep-alive)"""
        x, keep = self._eval_text(exotic)
        fn = getattr(self.lib, name + ("_x" if exotic is not None else ""))
        fn.restype = C.c_int
        fn.argtypes = argtypes + ([C.POINTER(abi.EvalText)] if exotic is not None else [])
        tail = [] if exotic is None else [C.byref(x) if x is not None else None]
        return fn, tail, (x, keep)

    def eval_adapter_kmers(self, seq_ptr, qual_ptr, len_ptr, n, trim_tail1, counts_ptr, exotic=None, check=True):
        """4^10 ten-mer histogram into DEVICE uint32[1 << 20] at counts_ptr; returns the records used"""
        fn, tail, keep = self._eval_fn("fastp_gpu_eval_adapter_kmers",
                                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.POINTER(C.c_int64)], exotic)
        rec = C.c_int64(0)
        rc = fn(self.h, seq_ptr, qual_ptr, len_ptr, n, trim_tail1, counts_ptr, C.byref(rec), *tail)
        if check:
            self._check(rc)
            return int(rec.value)
        return rc, int(rec.value)

    def eval_overrep(self, seq_ptr, qual_ptr, len_ptr, n, seq_len, max_seqs=1 << 16, text_capacity=1 << 22, check=True,
                     exotic=None):
        """Evaluator::computeOverRepSeq: returns (rc, [(sequence bytes, count)] in std::map order)"""
        fn, tail, keep = self._eval_fn("fastp_gpu_eval_overrep",
                                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int64,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)], exotic)
        text = C.create_string_buffer(max(1, text_capacity))
        off = (C.c_int64 * (max_seqs + 1))()
        cnt = (C.c_int64 * max(1, max_seqs))()
        ns = C.c_int32(0)
        rc = fn(self.h, seq_ptr, qual_ptr, len_ptr, n, seq_len, text, text_capacity, off, cnt, max_seqs, C.byref(ns), *tail)
        if check:
            self._check(rc)
        if rc != 0:
            return rc, int(ns.value)
        raw = text.raw
        return rc, [(raw[off[i]:off[i + 1]], int(cnt[i])) for i in range(ns.value)]

    def eval_known_adapters(self, seq_ptr, qual_ptr, len_ptr, n, adapters, check=True, exotic=None):
        """Evaluator::checkKnownAdapters over `adapters` (a list of bytes): returns (rc, counts int32[len(adapters)],
        mismatches int32[len(adapters)], checked_reads, best) - best an index into `adapters` or -1"""
        fn, tail, keep = self._eval_fn("fastp_gpu_eval_known_adapters",
                                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)], exotic)
        na = len(adapters)
        arr = (C.c_char_p * max(1, na))(*[bytes(x) for x in adapters])
        counts = np.zeros(max(1, na), dtype=np.int32)
        mism = np.zeros(max(1, na), dtype=np.int32)
        checked, best = C.c_int64(0), C.c_int32(-1)
        rc = fn(self.h, seq_ptr, qual_ptr, len_ptr, n, arr, na, counts.ctypes.data, mism.ctypes.data, C.byref(checked),
                C.byref(best), *tail)
        if check:
            self._check(rc)
        return rc, counts[:na], mism[:na], int(checked.value), int(best.value)

    def eval_adapter_seed(self, seq_ptr, qual_ptr, len_ptr, n, trim_tail1, seed, check=True, exotic=None):
        """the scans and dominant-path walks of Evaluator::getAdapterWithSeed for one seed (a bin of eval_adapter_kmers):
        returns (rc, forward bytes, backward bytes - as the tree returns it, not reversed -, reached_leaf, hits).
        With `exotic` the paths may hold any byte (a tree node prints the byte of the sequence that created it)"""
        fn, tail, keep = self._eval_fn("fastp_gpu_eval_adapter_seed",
                                       [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p,
                                        C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int64)], exotic)
        fwd, bwd = C.create_string_buffer(abi.MAX_READ_LEN), C.create_string_buffer(abi.MAX_READ_LEN)
        nf, nb, leaf, hits = C.c_int32(0), C.c_int32(0), C.c_int32(1), C.c_int64(0)
        rc = fn(self.h, seq_ptr, qual_ptr, len_ptr, n, trim_tail1, seed, fwd, C.byref(nf), bwd, C.byref(nb), C.byref(leaf),
                C.byref(hits), *tail)
        if check:
            self._check(rc)
        return rc, fwd.raw[:nf.value], bwd.raw[:nb.value], bool(leaf.value), int(hits.value)

    # ---- device memory through the engine (fastp_gpu_device_*): for hosts that hold no HIP runtime of their own ----
    def device_alloc(self, nbytes: int) -> int:
        fn = self.lib.fastp_gpu_device_alloc
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        p = C.c_void_p()
        self._check(fn(self.h, nbytes, C.byref(p)))
        return int(p.value)

    def device_free(self, ptr: int):
        fn = self.lib.fastp_gpu_device_free
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, ptr))

    def device_upload(self, dst_ptr: int, data):
        fn = self.lib.fastp_gpu_device_upload
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8))
        self._check(fn(self.h, dst_ptr, a.ctypes.data, a.size))

    def device_download(self, src_ptr: int, nbytes: int) -> np.ndarray:
        fn = self.lib.fastp_gpu_device_download
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(fn(self.h, out.ctypes.data, src_ptr, nbytes))
        return out

    def synchronize(self):
        self._check(self.lib.fastp_gpu_synchronize(self.h))

    # ---- pipelined host submits (include/fastp_gpu.h "Pipelined host submits") ----
    def host_alloc(self, nbytes: int) -> int:
        """page-locked host memory (fastp_gpu_host_alloc): what the batches and result arrays of submit_host_async live in"""
        fn = self.lib.fastp_gpu_host_alloc
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        p = C.c_void_p()
        self._check(fn(self.h, nbytes, C.byref(p)))
        return int(p.value)

    def host_free(self, ptr: int):
        fn = self.lib.fastp_gpu_host_free
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, ptr))

    @staticmethod
    def host_view(ptr: int, shape, dtype) -> np.ndarray:
        """a numpy array over memory of host_alloc (no copy; it must not outlive the allocation)"""
        shape = tuple(np.atleast_1d(shape))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr)).view(dtype).reshape(shape)

    def submit_host_async(self, batch: abi.Batch, results: abi.Results, slot: int, check=True) -> int:
        """queue one batch on `slot`; `batch`, `results` and what they point to stay untouched until the slot has been waited for"""
        fn = self.lib.fastp_gpu_submit_host_async
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(abi.Batch), C.POINTER(abi.Results), C.c_int]
        rc = fn(self.h, C.byref(batch), C.byref(results), slot)
        if check:
            self._check(rc)
        return rc

    def wait(self, slot: int, check=True) -> int:
        fn = self.lib.fastp_gpu_wait
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        rc = fn(self.h, slot)
        if check:
            self._check(rc)
        return rc

    def poll(self, slot: int) -> int:
        """1: the slot's batch has arrived (the slot is free), 0: still running, < 0: an error code"""
        fn = self.lib.fastp_gpu_poll
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
        return int(fn(self.h, slot))

    def reset(self):
        """a new run on the same context (fresh Stats / FilterResult / Duplicate)"""
        self._check(self.lib.fastp_gpu_reset(self.h))
        self._shard_stream_done = (0, 0)   # multigpu.run_shard's running stream origin belongs to the run that just ended

    # ---- collectives behind the C ABI (RCCL; csrc/fq_comm.cpp) ----
    def _comm_check(self, rc):
        if rc != 0:
            self.lib.fastp_gpu_comm_last_error.restype = C.c_char_p
            raise EngineError(rc, (self.lib.fastp_gpu_comm_last_error() or b"").decode())

    def comm_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._comm_check(self.lib.fastp_gpu_comm_id(buf))
        return bytes(buf)

    def comm_init(self, comm_id: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(comm_id)
        self.lib.fastp_gpu_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        self._comm_check(self.lib.fastp_gpu_comm_init(self.h, buf, nranks, rank))

    def _ctx_array(self):
        arr = (C.c_void_p * 1)(self.h)
        return arr

    def allreduce(self):
        """Stats::merge / FilterResult::merge over the communicator (this process owns one rank)"""
        self.lib.fastp_gpu_allreduce.argtypes = [C.c_void_p, C.c_int]
        self._comm_check(self.lib.fastp_gpu_allreduce(self._ctx_array(), 1))

    def exchange_dup_prefix(self):
        self.lib.fastp_gpu_exchange_dup_prefix.argtypes = [C.c_void_p, C.c_int]
        self._comm_check(self.lib.fastp_gpu_exchange_dup_prefix(self._ctx_array(), 1))

    def counters(self):
        out = np.zeros(self.layout.total, dtype=np.int64)
        self._check(self.lib.fastp_gpu_counters(self.h, out.ctypes.data, out.size))
        return out

    def counters_device(self):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.fastp_gpu_counters_device(self.h, C.byref(p), C.byref(n), None))
        return p.value, n.value

    def counters_export(self, dst_device_ptr: int):
        self._check(self.lib.fastp_gpu_counters_export(self.h, dst_device_ptr, self.layout.total))

    def counters_import(self, src_device_ptr: int):
        self._check(self.lib.fastp_gpu_counters_import(self.h, src_device_ptr, self.layout.total))

    def debug_phase_cycles(self):
        """cycles per phase of the fused kernel (context created with FASTP_GPU_PHASE_TIMING=1)"""
        out = (C.c_uint64 * 16)()
        fn = self.lib.fastp_gpu_debug_phase_cycles
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self.h, out))
        return list(out)

    KERNEL_REGS_NAMES = ("stats", "fq_reduce_kernel", "fq_dup_losers_kernel", "fq_dup_winners_kernel", "fq_dup_finish_kernel")
    STATS5_INSTANTIATIONS = {0: "one_nf", 1: "one", 2: "blocks10", 3: "blocks8", 4: "any_kc2", 5: "any_kc1", 6: "ablation"}

    def debug_kernel_regs(self):
        """what the runtime allocates the Stats kernel this context launches and the tail stream's small kernels:
        {"stats_inst": id of form 5's instantiation (-1: form 4), name: {"vgprs", "max_threads", "static_lds"}} (zeros on the emulator)"""
        out = (C.c_int32 * 16)()
        fn = self.lib.fastp_gpu_debug_kernel_regs
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        self._check(fn(self.h, out, 16))
        d = {"stats_inst": int(out[0])}
        for k, name in enumerate(self.KERNEL_REGS_NAMES):
            d[name] = {"vgprs": int(out[1 + 3 * k]), "max_threads": int(out[2 + 3 * k]), "static_lds": int(out[3 + 3 * k])}
        return d

    STATS_FOLDS = {-1: None, 0: "groups", 1: "wide"}

    def debug_stats_fold(self, slabs_ptr: int = 0, nblocks: int = 0, which: str = "auto"):
        """the Stats fold on its own, and what the context chose for the step's tail.  With slabs_ptr (device memory, 8-byte
        aligned, [nblocks][slab_dwords] uint32 in the layout the returned dict describes) the slabs are folded into the
        context's counter block on its stream - which = "groups": fq_reduce_kernel, "wide": fq_reduce_wide_kernel, "auto": what
        a launch with that many Stats slabs takes; synchronize() before the slabs are freed.  Returns {"finish_threads":
        fq_dup_finish_kernel's workgroup size, "last_stats_fold": "groups" / "wide" / None, "slab_dwords", "cp" (cycles a
        slab has cells for), "c" (cycles in use), "reduce_group", "wide_group", "wide_unroll", "wide_parts"}"""
        out = (C.c_int32 * 9)()
        fn = self.lib.fastp_gpu_debug_stats_fold
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        self._check(fn(self.h, slabs_ptr or None, nblocks, {"auto": -1, "groups": 0, "wide": 1}[which], out, 9))
        keys = ("finish_threads", "last_stats_fold", "slab_dwords", "cp", "c", "reduce_group", "wide_group", "wide_unroll", "wide_parts")
        d = {k: int(v) for k, v in zip(keys, out)}
        d["last_stats_fold"] = self.STATS_FOLDS[d["last_stats_fold"]]
        return d

    def debug_overrep_plan(self):
        """the LDS plan of this context's most recent overrepresentation launch as launch_overrep chose it:
        {"launches": how many so far, "sym_cap": positions of a read staged in LDS (0: none), "table_lds": (dword offset of
        read 1's / read 2's seed table in LDS, -1: probed in global memory)} - the same from the emulator"""
        out = (C.c_int32 * 4)()
        fn = self.lib.fastp_gpu_debug_overrep_plan
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        self._check(fn(self.h, out, 4))
        return {"launches": int(out[0]), "sym_cap": int(out[1]), "table_lds": (int(out[2]), int(out[3]))}

    def plan(self) -> str:
        """which kernels run the worker loop for this context's options"""
        self.lib.fastp_gpu_plan.argtypes = [C.c_void_p]
        return {0: "fused", 1: "split", 2: "lane"}.get(int(self.lib.fastp_gpu_plan(self.h)), "?")

    def kernel_time(self):
        ms, k = C.c_double(), C.c_int64()
        self._check(self.lib.fastp_gpu_kernel_time(self.h, C.byref(ms), C.byref(k)))
        return ms.value, k.value
