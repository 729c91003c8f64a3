"""Adapter auto-detection for `pipeline.py` users: the adapter decision of the reference's
Evaluator::evalAdapterAndReadNum (src/evaluator.cpp:308-483), which fastp runs before any worker starts for
single-end input and, with --detect_adapter_for_pe, for each mate of paired input.

The loops over the reads run on the device, through the engine's Evaluator calls (include/fastp_gpu.h):
`fastp_gpu_eval_known_adapters` (checkKnownAdapters), `fastp_gpu_eval_adapter_kmers` (the ten-mer histogram) and
`fastp_gpu_eval_adapter_seed` (the scans and tree walks of getAdapterWithSeed).  The decisions between them - the
10000-read gate, the top-10 seeds, the fold / count / complexity tests, the assembly of the adapter from a seed's two
paths, matchKnownAdapter, the reachedLeaf rule - are restated here once, in the reference's order.

The list of known adapters is the caller's (the reference compiles its own in; this package ships none):
`load_adapter_list` reads one from a file.

`FastqPipeline` does not call this module and its `run` signature is unchanged: a caller who wants fastp's
auto-detection calls `detect_adapter_in_file` on each input first and puts the result into the parameters
(`params.adapter_seq_r1` / `adapter_seq_r2`) before building the pipeline.
"""
from __future__ import annotations

import gzip

import numpy as np

from . import abi, engine

READ_LIMIT = 256 * 1024            # evaluator.cpp:314
BASE_LIMIT = 151 * READ_LIMIT      # :315
KEYLEN = 10
_ELIGIBLE = None


def int2seq(val: int, seqlen: int = KEYLEN) -> bytes:
    """Evaluator::int2seq (:561-571): first base in the most significant pair, A=0 T=1 C=2 G=3"""
    return bytes(b"ATCG"[(val >> (2 * (seqlen - 1 - i))) & 3] for i in range(seqlen))


def _eligible() -> np.ndarray:
    """the bins the top-10 loop looks at (:404-422): no base six or more times, fewer than eight of C and G, not
    starting with GGGG"""
    global _ELIGIBLE
    if _ELIGIBLE is None:
        k = np.arange(1 << (2 * KEYLEN), dtype=np.int64)
        digit = np.stack([(k >> (2 * i)) & 3 for i in range(KEYLEN)])
        atcg = np.stack([(digit == b).sum(axis=0) for b in range(4)])
        ok = (atcg < KEYLEN - 4).all(axis=0) & (atcg[2] + atcg[3] < KEYLEN - 2) & ((k >> 12) != 0xff)
        _ELIGIBLE = ok
    return _ELIGIBLE


def top_seeds(counts) -> tuple[list[int], int]:
    """the top-10 choice of :399-443 over the histogram `counts` (1 << 20 bins): (topkeys, total).  The insertion loop
    moves a bin past every entry that is not larger, so the ten are the eligible bins by count, largest first, and
    among equal counts the later key first; `total` sums the eligible bins only."""
    counts = np.asarray(counts).astype(np.int64)
    ok = _eligible()
    keys = np.flatnonzero(ok)
    total = int(counts[keys].sum())
    rank = counts[keys] * (1 << 20) + keys          # count, then key, both descending
    top = keys[np.argsort(-rank, kind="stable")[:10]]
    return [int(k) for k in top], total


def match_known_adapter(seq: bytes, known_adapters) -> bytes:
    """Evaluator::matchKnownAdapter (:541-559): the first known adapter, in std::map order, that `seq` starts with"""
    for a in sorted(known_adapters):
        if len(seq) >= len(a) and seq[:len(a)] == a:
            return a
    return b""


def detect_adapter(g: engine.GpuEngine, seq_ptr, qual_ptr, len_ptr, n, known_adapters, trim_tail1: int = 0) -> bytes:
    """evalAdapterAndReadNum's adapter for the n reads whose packed rows (one mate) are at the DEVICE pointers, laid
    out for `g`'s max_len: the adapter sequence, or b"" when none is found.  known_adapters: distinct bytes of ACGT."""
    known = [bytes(a) for a in known_adapters]
    # the reads the loading loop admits (:328-343)
    lens = g.device_download(len_ptr, 2 * min(n, READ_LIMIT)).view(np.uint16) if n > 0 else np.zeros(0, np.uint16)
    records = int(min(len(lens), np.searchsorted(np.cumsum(lens.astype(np.int64)), BASE_LIMIT, side="left") + 1)) if len(lens) else 0
    if records < 10000:                              # :357
        return b""
    rc, _, _, _, best = g.eval_known_adapters(seq_ptr, qual_ptr, len_ptr, records, known)
    if best >= 0 and len(known[best]) > 8:           # :367
        return known[best]
    counts_ptr = g.device_alloc(4 << 20)
    try:
        g.eval_adapter_kmers(seq_ptr, qual_ptr, len_ptr, records, trim_tail1, counts_ptr)
        counts = g.device_download(counts_ptr, 4 << 20).view(np.uint32)
    finally:
        g.device_free(counts_ptr)
    topkeys, total = top_seeds(counts)
    size = 1 << (2 * KEYLEN)
    for key in topkeys:                              # :446-473
        if key == 0:
            continue
        count = int(counts[key])
        if count < 10 or count * size < total * 20:  # FOLD_THRESHOLD
            break
        seq = int2seq(key)
        if sum(1 for s in range(len(seq) - 1) if seq[s] != seq[s + 1]) < 3:
            continue
        # getAdapterWithSeed :485-539
        _, fwd, bwd, reached_leaf, _ = g.eval_adapter_seed(seq_ptr, qual_ptr, len_ptr, records, trim_tail1, key)
        adapter = (bwd[::-1] + seq + fwd)[:60]
        matched = match_known_adapter(adapter, known)
        if matched:
            return matched
        if reached_leaf:
            return adapter
    return b""


def _read_prefix(path: str) -> tuple[bytes, int, int]:
    """the records the loading loop :328-343 reads from a plain or gzip-compressed FASTQ: (text, records, longest read)"""
    opener = gzip.open if path.endswith(".gz") else open
    out = []
    records = bases = longest = 0
    with opener(path, "rb") as f:
        while records < READ_LIMIT and bases < BASE_LIMIT:
            rec = [f.readline() for _ in range(4)]
            if not rec[0]:
                break
            rec = [ln if ln.endswith(b"\n") else ln + b"\n" for ln in rec]   # (a last line without its newline)
            rlen = len(rec[1].rstrip(b"\r\n"))
            out.extend(rec)
            records += 1
            bases += rlen
            longest = max(longest, rlen)
    return b"".join(out), records, longest


def detect_adapter_in_file(path: str, known_adapters, trim_tail1: int = 0, device: int = 0, lib_path: str | None = None) -> bytes:
    """fastp's adapter auto-detection for one input file (plain or ".gz" FASTQ): reads the prefix the reference's
    Evaluator would load, parses it on the device with an engine of its own and returns `detect_adapter`'s answer"""
    text, records, longest = _read_prefix(path)
    if longest > abi.MAX_READ_LEN:
        raise ValueError(f"{path}: a read of {longest} bases; the device path holds reads of up to {abi.MAX_READ_LEN}")
    if records < 10000:
        return b""
    max_len = max(longest, 32)
    g = engine.GpuEngine(abi.default_params(False, max_len), device=device, lib_path=lib_path)
    ptrs = []
    try:
        ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
        cap = records + 2

        def alloc(nbytes):
            ptrs.append(g.device_alloc(nbytes))
            return ptrs[-1]
        t = alloc(len(text) + 32)
        g.device_upload(t, text + b"\0" * ((-len(text)) % 16 + 16))
        seq, qual, lens = alloc(cap * ss), alloc(cap * qs), alloc(cap * 2)
        loff, llen = alloc(cap * 16), alloc(cap * 16)
        info = g.parse_fastq(t, len(text), True, cap, seq, qual, lens, loff, llen)
        if info.first_bad != -1:
            raise ValueError(f"{path}: record {info.first_bad} is not FASTQ the device parser takes")
        return detect_adapter(g, seq, qual, lens, int(info.n_records), known_adapters, trim_tail1)
    finally:
        for p in ptrs:
            g.device_free(p)
        g.close()


def load_adapter_list(path: str) -> list[bytes]:
    """known adapters from a file: one sequence per line, or FASTA (a sequence may span lines); upper-cased,
    duplicates dropped, first occurrence kept"""
    seqs: list[bytes] = []
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f.read().splitlines()]
    if any(ln.startswith(b">") for ln in lines):
        cur = None
        for ln in lines:
            if ln.startswith(b">"):
                if cur:
                    seqs.append(cur)
                cur = b""
            elif ln and cur is not None:
                cur += ln
        if cur:
            seqs.append(cur)
    else:
        seqs = [ln for ln in lines if ln and not ln.startswith(b"#")]
    out, seen = [], set()
    for s in seqs:
        s = s.upper()
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out
