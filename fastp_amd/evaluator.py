"""Adapter auto-detection for `pipeline.py` users: the adapter decision of the reference's
Evaluator::evalAdapterAndReadNum (src/evaluator.cpp:308-483), which fastp runs before any worker starts for
single-end input and, with --detect_adapter_for_pe, for each mate of paired input.

The loops over the reads run on the device, through the engine's Evaluator calls (include/fastp_gpu.h):
`fastp_gpu_eval_known_adapters` (checkKnownAdapters), `fastp_gpu_eval_adapter_kmers` (the ten-mer histogram) and
`fastp_gpu_eval_adapter_seed` (the scans and tree walks of getAdapterWithSeed).  The decisions between them - the
10000-read gate, the top-10 seeds, the fold / count / complexity tests, the assembly of the adapter from a seed's two
paths, matchKnownAdapter, the reachedLeaf rule - are restated here once, in the reference's order.

Reads with letters outside ACGTN (soft-masked lower case, IUPAC codes, '.') are stored in the packed rows as if the
letter were an A; `detect_adapter(..., exotic=...)` names them and the calls take their symbols from the FASTQ text
(the `fastp_gpu_eval_*_x` forms), so the answer is the reference's for such samples too.  `detect_adapter_in_file` and
`overrep_in_file` do this on their own.

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


def detect_adapter(g: engine.GpuEngine, seq_ptr, qual_ptr, len_ptr, n, known_adapters, trim_tail1: int = 0, exotic=None) -> bytes:
    """evalAdapterAndReadNum's adapter for the n reads whose packed rows (one mate) are at the DEVICE pointers, laid
    out for `g`'s max_len: the adapter sequence, or b"" when none is found.  known_adapters: distinct bytes of ACGT.

    exotic: None, or (units, text_ptr, off_ptr, dense) for the reads with letters outside ACGTN - ascending int32 read
    indexes, the DEVICE text holding their sequence bytes and the DEVICE offsets (dense: the parser's line_off table), as
    the engine's eval_* calls take them.  After `parse_fastq`: (g.parse_exotic(), the chunk, its line_off table, True).

    The result is what the reference returns, and with such reads it may itself hold a letter outside ACGT: a tree node
    prints the byte of the read that created it (nucleotidetree.cpp:48-51).  The reference then ends with "the adapter
    <adapter_sequence> can only have bases in {A, T, C, G}" (options.cpp:375-381), and `fastp_gpu_create` refuses such a
    string as adapter_seq_r1 / r2 the same way (FASTP_GPU_E_INVALID, "adapter sequence may only contain A, T, C, G"):
    what to do with such a result is the caller's decision."""
    if exotic is not None and len(exotic[0]) == 0:
        exotic = None
    known = [bytes(a) for a in known_adapters]
    # the reads the loading loop admits (:328-343)
    lens = g.device_download(len_ptr, 2 * min(n, READ_LIMIT)).view(np.uint16) if n > 0 else np.zeros(0, np.uint16)
    records = int(min(len(lens), np.searchsorted(np.cumsum(lens.astype(np.int64)), BASE_LIMIT, side="left") + 1)) if len(lens) else 0
    if records < 10000:                              # :357
        return b""
    rc, _, _, _, best = g.eval_known_adapters(seq_ptr, qual_ptr, len_ptr, records, known, exotic=_first(exotic, records))
    if best >= 0 and len(known[best]) > 8:           # :367
        return known[best]
    counts_ptr = g.device_alloc(4 << 20)
    try:
        g.eval_adapter_kmers(seq_ptr, qual_ptr, len_ptr, records, trim_tail1, counts_ptr, exotic=_first(exotic, records))
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
        _, fwd, bwd, reached_leaf, _ = g.eval_adapter_seed(seq_ptr, qual_ptr, len_ptr, records, trim_tail1, key, exotic=_first(exotic, records))
        adapter = (bwd[::-1] + seq + fwd)[:60]
        matched = match_known_adapter(adapter, known)
        if matched:
            return matched
        if reached_leaf:
            return adapter
    return b""


def _first(exotic, n):
    """`exotic` cut to the listed reads below n (the calls take a list of indexes inside [0, n)); None if none is left"""
    if exotic is None:
        return None
    units = np.asarray(exotic[0], dtype=np.int32)
    units = units[:int(np.searchsorted(units, n))]   # (one offset per listed read: the first len(units) are the kept reads')
    return (units,) + tuple(exotic[1:]) if len(units) else None


def _read_prefix(path: str, read_limit: int = READ_LIMIT, base_limit: int = BASE_LIMIT) -> tuple[bytes, int, int]:
    """the records a loading loop `while (records < read_limit && bases < base_limit)` (:328-343, :88) reads from a plain
    or gzip-compressed FASTQ: (text, records, longest read)"""
    opener = gzip.open if path.endswith(".gz") else open
    out = []
    records = bases = longest = 0
    with opener(path, "rb") as f:
        while records < read_limit and bases < base_limit:
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


def _check_longest(path, longest):
    if longest > abi.MAX_READ_LEN:
        raise ValueError(f"{path}: a read of {longest} bases; the device path holds reads of up to {abi.MAX_READ_LEN}")


class _ParsedPrefix:
    """a file's prefix parsed on the device with an engine of its own: packed rows, the chunk and its line table"""

    def __init__(self, path, text, records, longest, device, lib_path):
        max_len = max(longest, 32)
        self.g = g = engine.GpuEngine(abi.default_params(False, max_len), device=device, lib_path=lib_path)
        self.ptrs = []
        try:
            ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
            cap = records + 2
            t = self._alloc(len(text) + 32)
            g.device_upload(t, text + b"\0" * ((-len(text)) % 16 + 16))
            self.seq, self.qual, self.lens = self._alloc(cap * ss), self._alloc(cap * qs), self._alloc(cap * 2)
            loff, llen = self._alloc(cap * 16), self._alloc(cap * 16)
            info = g.parse_fastq(t, len(text), True, cap, self.seq, self.qual, self.lens, loff, llen)
            if info.first_bad != -1:
                raise ValueError(f"{path}: record {info.first_bad} is not FASTQ the device parser takes")
            self.n = int(info.n_records)
            # records with letters outside ACGTN: their symbols come from the chunk (fastp_gpu_eval_*_x)
            self.exotic = (g.parse_exotic(), t, loff, True) if info.n_exotic else None
        except BaseException:
            self.close()
            raise

    def _alloc(self, nbytes):
        self.ptrs.append(self.g.device_alloc(nbytes))
        return self.ptrs[-1]

    def close(self):
        for p in self.ptrs:
            self.g.device_free(p)
        self.ptrs = []
        self.g.close()


def detect_adapter_in_file(path: str, known_adapters, trim_tail1: int = 0, device: int = 0, lib_path: str | None = None) -> bytes:
    """fastp's adapter auto-detection for one input file (plain or ".gz" FASTQ): reads the prefix the reference's
    Evaluator would load, parses it on the device with an engine of its own and returns `detect_adapter`'s answer.
    Records with letters outside ACGTN are handed on as the parser lists them, so a soft-masked file gets the reference's
    answer; see `detect_adapter` for an answer that holds such a letter itself."""
    text, records, longest = _read_prefix(path)
    _check_longest(path, longest)
    if records < 10000:
        return b""
    p = _ParsedPrefix(path, text, records, longest, device, lib_path)
    try:
        return detect_adapter(p.g, p.seq, p.qual, p.lens, p.n, known_adapters, trim_tail1, exotic=p.exotic)
    finally:
        p.close()


def overrep_in_file(path: str, seq_len: int, device: int = 0, lib_path: str | None = None, max_seqs: int = 1 << 16,
                    text_capacity: int = 1 << 22) -> dict:
    """Evaluator::computeOverRepSeq (evaluator.cpp:78-169) for one input file (plain or ".gz" FASTQ) and the sequence length
    computeSeqLen found: reads the records its loop reads (while fewer than 151 * 10000 bases were seen), parses them on the
    device and returns {sequence bytes: count}, the map Options::overRepSeqs starts from.  Sequences of reads with letters
    outside ACGTN carry those bytes, as the reference's raw substrings do."""
    text, records, longest = _read_prefix(path, read_limit=1 << 62, base_limit=151 * 10000)
    _check_longest(path, longest)
    if records == 0:
        return {}
    p = _ParsedPrefix(path, text, records, longest, device, lib_path)
    try:
        _, seqs = p.g.eval_overrep(p.seq, p.qual, p.lens, p.n, seq_len, max_seqs=max_seqs, text_capacity=text_capacity,
                                   exotic=p.exotic)
        return dict(seqs)
    finally:
        p.close()


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
