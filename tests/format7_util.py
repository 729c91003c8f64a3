"""helpers for the seven-stream device formatter tests (fastp_gpu_format_all_streams): format_util's preparation
(text -> fastp_gpu_parse_fastq -> fastp_gpu_submit_device), then every stream of the worker loop plus
--overlapped_out's; the expected value is fastp_amd.hostloop.apply_results through driver.run_engine"""
import cases
import driver
import format_util
import synth
from fastp_amd import abi, hostloop

STREAMS = format_util.STREAMS + ("overlapped",)

# parameter sets: name -> (case of tests/cases.py, fields set on top of it)
SETS = {
    "pe_overlapped_out": ("pe_overlapped_out", {}),
    "pe_overlapped_out_trims": ("pe_overlapped_out_trims", {}),
    "pe_overlapped_out_noadapter": ("pe_overlapped_out_noadapter", {}),
    "pe_merge_overlapped_out": ("pe_merge_overlapped_out", {}),
    "pe_merge_overlapped_out_trims": ("pe_merge_overlapped_out_trims", {}),
    "pe_exotic_default": ("pe_exotic_default", {}),
    "umi": ("pe_umi_per_read", dict(overlapped_out=1, adapter_enabled=0)),
    "dedup": ("pe_noadapter_dedup", dict(overlapped_out=1)),
    "correction": ("pe_correction", dict(overlapped_out=1, adapter_enabled=0)),
}
# (records, records with a non-empty sequence line) the host writer makes of 600 pairs, seed 77 - measured on the emulator and
# on the GPU; the tests assert lower bounds on the expected stream, these are for the reader
COUNTS_600 = {
    "pe_overlapped_out": (201, 6), "pe_overlapped_out_trims": (307, 172), "pe_overlapped_out_noadapter": (283, 172),
    "pe_merge_overlapped_out": (320, 6), "pe_merge_overlapped_out_trims": (307, 172), "pe_exotic_default": (257, 19),
    "umi": (74, 17), "dedup": (78, 12), "correction": (321, 122),
}


def inputs(set_name, n, seed=77):
    """(params, fq1, fq2, umi tuple | None) of a parameter set"""
    case, extra = SETS.get(set_name, (set_name, {}))
    paired, flags, pf, skw = cases.CASES[case]
    d = synth.synth_pairs(n, L=150, seed=seed, paired=paired, **skw)
    p = pf(150)
    for k, v in extra.items():
        setattr(p, k, v)
    params = cases.finalize_params(case, p, d["seq1"], d["len1"], d.get("seq2"), d.get("len2"))
    fq1 = synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1)
    fq2 = synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2) if paired else None
    return params, fq1, fq2, cases.UMI.get(case)


def expected(mk_engine, params, fq1, fq2, max_len, want_failed, want_unpaired, umi, pack=None):
    """{stream: bytes} of the host writer (hostloop.apply_results) on the same engine parameters"""
    editor = hostloop.UmiNameEditor(*umi) if umi else None
    ref = mk_engine(params)
    n = fq1.count(b"\n") // 4
    want, _, _ = driver.run_engine(ref, params, fq1, fq2, pack=pack or max(n, 1), stride=abi.qual_stride(max_len),
                                   want_failed=want_failed, want_unpaired=want_unpaired, umi=editor)
    ref.close()
    out = {}
    for k in STREAMS:
        w = getattr(want, k, None)
        out[k] = bytes(w) if w is not None else b""
    return out


def prepare(eng, mem, fq1, fq2, max_len, corr_cap=1 << 16):
    """format_util._prepare with the parser's list of records that hold letters outside ACGTN handed on to the engine
    (fastp_gpu_parse_exotic -> the batch's exotic_* fields), as the file loop and the pipeline do"""
    import numpy as np
    paired = fq2 is not None
    ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
    mates, exotic, n = [], [], None
    for txt in ((fq1, fq2) if paired else (fq1,)):
        cap = txt.count(b"\n") // 4 + 2
        t = mem.upload(txt, (-len(txt)) % 16 + 16)
        seq, qual = mem.alloc(cap * ss), mem.alloc(cap * qs)
        lens, loff, llen = mem.alloc(cap * 2), mem.alloc(cap * 16), mem.alloc(cap * 16)
        mem.sync()
        info = eng.parse_fastq(mem.ptr(t), len(txt), True, cap, mem.ptr(seq), mem.ptr(qual), mem.ptr(lens), mem.ptr(loff), mem.ptr(llen))
        assert info.first_bad == -1
        if info.n_exotic:
            exotic.append(eng.parse_exotic())
        n = info.n_records if n is None else min(n, info.n_records)
        mates.append(dict(text=t, seq=seq, qual=qual, lens=lens, loff=loff, llen=llen, nbytes=len(txt)))
    res = [mem.alloc(n * 12), mem.alloc(n * 12)]
    pr, corr, nc = mem.alloc(n * 8), mem.alloc(corr_cap * 8), mem.alloc(16)
    b = abi.Batch()
    b.n, b.flags = n, abi.BATCH_STAT_ISIZE
    b.seq1, b.qual1, b.len1 = (mem.ptr(mates[0][k]) for k in ("seq", "qual", "lens"))
    if paired:
        b.seq2, b.qual2, b.len2 = (mem.ptr(mates[1][k]) for k in ("seq", "qual", "lens"))
    xu = np.zeros(0, dtype=np.int32)
    if exotic:
        xu = np.unique(np.concatenate(exotic)).astype(np.int32)
        xu = np.ascontiguousarray(xu[xu < n])
    if len(xu):
        b.n_exotic, b.exotic_dense, b.exotic_unit = len(xu), 1, xu.ctypes.data
        for m in range(len(mates)):
            b.exotic_text[m], b.exotic_off[m] = mem.ptr(mates[m]["text"]), mem.ptr(mates[m]["loff"])
    r = abi.Results()
    r.r1, r.r2, r.pair = mem.ptr(res[0]), mem.ptr(res[1]) if paired else None, mem.ptr(pr) if paired else None
    r.corrections, r.corrections_capacity, r.n_corrections = mem.ptr(corr), corr_cap, mem.ptr(nc)
    ev_cap = 4 * n + 16
    ev, nev = mem.alloc(ev_cap * 12), mem.alloc(16)
    r.adapter_events, r.adapter_events_capacity, r.n_adapter_events = mem.ptr(ev), ev_cap, mem.ptr(nev)
    mem.sync()
    eng.submit_device(b, r)
    eng.synchronize()
    return dict(n=n, mates=mates, res=res, pair=pr, corr=corr, nc=nc, paired=paired, n_exotic=len(xu))


def run_all_streams(eng, mem, params, fq1, fq2, max_len, want_failed=True, want_unpaired=False, umi=None, shrink=None,
                    null_overlapped=False):
    """every stream through fastp_gpu_format_all_streams; returns (rc, {stream: bytes}, [needed lengths]).
    shrink = index of the stream whose buffer holds 100 bytes; null_overlapped: no seventh buffer"""
    c = prepare(eng, mem, fq1, fq2, max_len)
    n, mates, res, paired = c["n"], c["mates"], c["res"], c["paired"]
    ios = []
    for m in range(2 if paired else 1):
        f = abi.FormatIn()
        f.text, f.line_off, f.line_len, f.res = (mem.ptr(mates[m]["text"]), mem.ptr(mates[m]["loff"]),
                                                 mem.ptr(mates[m]["llen"]), mem.ptr(res[m]))
        ios.append(f)
    o = abi.FormatOptions()
    o.want_failed, o.want_unpaired1, o.want_unpaired2 = int(want_failed), int(want_unpaired), int(want_unpaired)
    tag = 0
    if umi is not None:
        o.umi_loc = {"read1": 1, "read2": 2, "per_read": 3}[umi[0]]
        o.umi_len = umi[1]
        o.umi_prefix = umi[2] if len(umi) > 2 and umi[2] else None
        o.umi_delimiter = umi[3] if len(umi) > 3 else None
        tag = len(umi[3] if len(umi) > 3 and umi[3] else b":") + (len(umi[2]) + 1 if len(umi) > 2 and umi[2] else 0) + 2 * umi[1] + 1
    total = sum(m["nbytes"] for m in mates)
    caps = [total + n * 2 * 160 + 64] * 6
    caps.append(mates[0]["nbytes"] + n * tag)   # the header's bound for the seventh stream: mate 1's text + n UMI tags
    if shrink is not None:
        caps[shrink] = 100
    outs = [mem.alloc(max(16, k), 0xEE) for k in caps]
    ptrs = [mem.ptr(x) for x in outs]
    if null_overlapped:
        ptrs[6], caps[6] = None, 0
    mem.sync()
    rc, lens = eng.format_all_streams(n, ios[0], ios[1] if paired else None, mem.ptr(c["pair"]) if paired else None,
                                      mem.ptr(c["corr"]), mem.ptr(c["nc"]), o, ptrs, caps, check=False)
    assert len(lens) == 7
    got = {}
    for i, k in enumerate(STREAMS):
        whole = mem.download(outs[i])
        keep = min(lens[i], caps[i])
        got[k] = whole[:keep]
        tail = whole[keep:]   # nothing past the reported length (a NULL seventh buffer: its stand-in stays untouched)
        assert tail.count(b"\xEE") == len(tail), f"stream {k}: bytes written past its length"
    return rc, got, lens


def count_records(text: bytes):
    """(records, records whose sequence line is not empty) of FASTQ text"""
    lines = text.split(b"\n")
    seqs = lines[1::4]
    return len(lines) // 4, sum(1 for s in seqs if s)


def case(mk_engine, mem, set_name, n, want_failed=True, want_unpaired=False, eol=b"\n", seed=77):
    """all seven streams of a parameter set == the host writer; returns (got, expected)"""
    params, fq1, fq2, umi = inputs(set_name, n, seed)
    want = expected(mk_engine, params, fq1, fq2, 150, want_failed, want_unpaired, umi)
    g = mk_engine(params)
    rc, got, lens = run_all_streams(g, mem, params, fq1.replace(b"\n", eol), fq2.replace(b"\n", eol) if fq2 is not None else None,
                                    150, want_failed, want_unpaired, umi)
    g.close()
    assert rc == 0, rc
    for k in STREAMS:
        assert got[k] == want[k], f"{set_name}: stream {k} differs ({len(got[k])} vs {len(want[k])} bytes)"
        assert lens[STREAMS.index(k)] == len(want[k])
    return got, want
