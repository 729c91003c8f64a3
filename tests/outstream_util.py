"""helpers for the --stdout / --split formatter tests (fastp_gpu_format_interleaved, fastp_gpu_format_pack_cuts): format7_util's
preparation once, then any number of fastp_gpu_format_all_streams calls on it; the expected values come from the host writer
(fastp_amd.hostloop.apply_results) on the same engine parameters"""
import numpy as np

import format7_util as f7
from fastp_amd import abi, hostloop

STREAMS = f7.STREAMS


def host_writer(mk_engine, params, fq1, fq2, max_len, want_failed, want_u1, want_u2, umi):
    """{stream: bytes} of hostloop.apply_results over the whole text as one pack (driver.run_engine with the two unpaired
    streams chosen one by one)"""
    editor = hostloop.UmiNameEditor(*umi) if umi else None
    stride = abi.qual_stride(max_len)
    b1 = hostloop.parse_fastq(fq1, stride)
    b2 = hostloop.parse_fastq(fq2, stride) if fq2 is not None else None
    outs = hostloop.Outputs(b2 is not None, want_failed, want_u1, want_u2)
    amaps = hostloop.AdapterMaps()
    eng = mk_engine(params)
    if b2 is not None:
        r1, r2, pr, corr = eng.process(b1.seq, b1.qual, b1.lens, b2.seq, b2.qual, b2.lens)
        hostloop.apply_results(params, b1, b2, r1, r2, pr, corr, outs, amaps, editor, adapter_events=getattr(eng, "last_adapter_events", None))
    else:
        r1, _, _, corr = eng.process(b1.seq, b1.qual, b1.lens)
        hostloop.apply_results(params, b1, None, r1, None, None, corr, outs, amaps, editor, adapter_events=getattr(eng, "last_adapter_events", None))
    eng.close()
    out = {}
    for k in STREAMS:
        w = getattr(outs, k, None)
        out[k] = bytes(w) if w is not None else b""
    return out


def records(text: bytes):
    """the four-line records of FASTQ text"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def unit_of(record: bytes) -> int:
    """synth.to_fastq's names: @SIM:1:FC:1:1101:<unit // 1000>:<unit>[:UMI tag] <mate>:N:0:ATCG"""
    return int(record.split(b"\n", 1)[0].split(b" ")[0].split(b":")[6])


def interleave(out1: bytes, out2: bytes) -> bytes:
    """--stdout's stream (peprocessor.cpp:577-585): read 1's record, then read 2's, pair by pair"""
    a, b = records(out1), records(out2)
    assert len(a) == len(b)
    return b"".join(x + y for x, y in zip(a, b))


class Prepared:
    """text parsed and run through the engine once; format() may be called again and again (the corrections are patched into
    the text by every call: the same bytes)"""

    def __init__(self, eng, mem, fq1, fq2, max_len, umi=None):
        self.eng, self.mem, self.umi = eng, mem, umi
        self.c = f7.prepare(eng, mem, fq1, fq2, max_len)
        self.n, self.paired = self.c["n"], self.c["paired"]

    def format(self, want_failed=True, want_u1=False, want_u2=False, n=None, null_out2=False):
        """(rc, {stream: bytes}, [needed lengths]) of fastp_gpu_format_all_streams over the first n units"""
        c, mem, umi = self.c, self.mem, self.umi
        n = self.n if n is None else n
        ios = []
        for m in range(2 if self.paired else 1):
            f = abi.FormatIn()
            f.text, f.line_off, f.line_len, f.res = (mem.ptr(c["mates"][m]["text"]), mem.ptr(c["mates"][m]["loff"]),
                                                     mem.ptr(c["mates"][m]["llen"]), mem.ptr(c["res"][m]))
            ios.append(f)
        o = abi.FormatOptions()
        o.want_failed, o.want_unpaired1, o.want_unpaired2 = int(want_failed), int(want_u1), int(want_u2)
        if umi is not None:
            o.umi_loc = {"read1": 1, "read2": 2, "per_read": 3}[umi[0]]
            o.umi_len = umi[1]
        total = sum(m["nbytes"] for m in c["mates"])
        # "both mates" bound of include/fastp_gpu.h: T1 + T2 + 2 * (sum G + n) + 96 * n, G = 1 + 2 * umi_len + 1
        g = (2 + 2 * umi[1]) if umi is not None else 0
        caps = [total + 2 * self.n * (g + 1) + 96 * self.n + 16] * 7
        outs = [mem.alloc(max(16, k), 0xEE) for k in caps]
        ptrs = [mem.ptr(x) for x in outs]
        if null_out2:
            ptrs[1], caps[1] = None, 0
        mem.sync()
        rc, lens = self.eng.format_all_streams(n, ios[0], ios[1] if self.paired else None, mem.ptr(c["pair"]) if self.paired else None,
                                               mem.ptr(c["corr"]), mem.ptr(c["nc"]), o, ptrs, caps, check=False)
        got = {}
        for i, k in enumerate(STREAMS):
            whole = mem.download(outs[i])
            keep = min(lens[i], caps[i])
            got[k] = whole[:keep]
            tail = whole[keep:]
            assert tail.count(b"\xEE") == len(tail), f"stream {k}: bytes written past its length"
        return rc, got, lens


class PackTable:
    """device arrays of a fastp_gpu_pack_cuts plan, filled with a mark so that untouched entries show"""
    MARK = 0xA5

    def __init__(self, mem, max_packs):
        self.mem, self.max_packs = mem, max_packs
        self.cut = mem.alloc(2 * (max_packs + 1) * 8 + 64, self.MARK)
        self.passed = mem.alloc(max_packs * 4 + 64, self.MARK)
        assert mem.ptr(self.cut) % 8 == 0 and mem.ptr(self.passed) % 4 == 0

    def plan(self, first_unit, pack_size):
        p = abi.PackCuts()
        p.first_unit, p.pack_size, p.max_packs = first_unit, pack_size, self.max_packs
        p.cut, p.passed = self.mem.ptr(self.cut), self.mem.ptr(self.passed)
        return p

    def read(self):
        """(cut [2][max_packs + 1] u64, passed [max_packs] u32, the bytes behind both arrays)"""
        self.mem.sync()
        rawc, rawp = self.mem.download(self.cut), self.mem.download(self.passed)
        nc, npd = 2 * (self.max_packs + 1) * 8, self.max_packs * 4
        cut = np.frombuffer(rawc[:nc], dtype=np.uint64).reshape(2, self.max_packs + 1)
        passed = np.frombuffer(rawp[:npd], dtype=np.uint32)
        return cut, passed, rawc[nc:nc + 64] + rawp[npd:npd + 64]


def expected_table(out1: bytes, out2: bytes, n, first_unit, pack_size):
    """(cut [2][S + 1], passed [S]) from the host writer's streams: per-unit byte counts by the unit index in the names"""
    size = np.zeros((2, n), dtype=np.int64)
    for q, text in enumerate((out1, out2)):
        for r in records(text):
            size[q, unit_of(r)] += len(r)
    wrote = size[0] > 0
    if n == 0:
        return np.zeros((2, 1), dtype=np.int64), np.zeros(0, dtype=np.int64)
    heads = [0] + [g for g in range(1, n) if (first_unit + g) % pack_size == 0]
    edges = heads + [n]
    pre = np.concatenate([np.zeros((2, 1), dtype=np.int64), np.cumsum(size, axis=1)], axis=1)
    cut = pre[:, edges]
    passed = np.array([int(wrote[a:b].sum()) for a, b in zip(edges[:-1], edges[1:])], dtype=np.int64)
    return cut, passed
