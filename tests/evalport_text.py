"""evalport_text.py - TEST INFRASTRUCTURE: the reference's Evaluator loops on the RAW text of reads with letters outside
ACGTN (soft-masked lower case, IUPAC codes, '.'), the checker for fastp_gpu_eval_*_x (tests/test_eval_text.py).

tests/evalport.py and tests/evalport_adapter.py restate the loops of src/evaluator.cpp and src/nucleotidetree.cpp on a
hostloop.parse_fastq batch, whose rows are the file's bytes; what they do with a byte b outside ACGTN is the reference's:
    seq2int (:577-626)                  anything but A T C G -> -1           (evalport.adapter_kmer_counts, port.seq2int)
    checkKnownAdapters (:266-287)       raw != against the adapter           (port.first_match / match_table)
    NucleotideTree::addSeq (:42-55)     only 'N' cuts, child b & 7, a node keeps its creator's byte    (port.NucleotideTree)
    computeOverRepSeq (:99-160)         raw substrings in a map, byte order  (evalport.evaluate_overrep_counts)
This module adds what the text-aware cases need on top: the batch as the PACKED ROWS show it (every such byte an 'A' -
what the kernels answered for before), the list of reads the parser reports, the tree walk on bytes instead of
characters, and the whole adapter decision with the histogram included."""
import numpy as np

import evalport
import evalport_adapter as port
from fastp_amd import hostloop

_IS_ACGTN = np.zeros(256, dtype=bool)
_IS_ACGTN[list(b"ACGTN")] = True


def listed(b) -> np.ndarray:
    """the reads fastp_gpu_parse_exotic lists: those holding a byte outside ACGTN (ascending int32)"""
    inside = np.arange(b.seq.shape[1])[None, :] < np.asarray(b.lens)[:, None]
    return np.flatnonzero((~_IS_ACGTN[b.seq] & inside).any(axis=1)).astype(np.int32)


def as_packed(b):
    """the batch the packed rows describe: a byte outside ACGTN is stored as code 0 without the N flag - an 'A'"""
    inside = np.arange(b.seq.shape[1])[None, :] < np.asarray(b.lens)[:, None]
    seq = np.where(~_IS_ACGTN[b.seq] & inside, np.uint8(ord("A")), b.seq)
    return hostloop.FastqBatch(b.names, b.strands, seq, b.qual, b.lens)


class ByteTree:
    """nucleotidetree.cpp on bytes (evalport_adapter.NucleotideTree keeps characters; the two agree on ASCII)"""

    def __init__(self):
        self.root = {"count": 0, "base": ord("N"), "children": [None] * 8}

    def add_seq(self, seq: bytes):            # :42-55
        cur = self.root
        for ch in seq:
            if ch == ord("N"):
                break
            base = ch & 0x07
            if cur["children"][base] is None:
                cur["children"][base] = {"count": 0, "base": ch, "children": [None] * 8}
            cur["children"][base]["count"] += 1
            cur = cur["children"][base]

    def dominant_path(self, reached_leaf: bool):   # :57-88
        out = bytearray()
        cur = self.root
        while True:
            total = 0
            for i in range(8):
                if cur["children"][i] is not None:
                    total += cur["children"][i]["count"]
            if total < 50:
                break
            has_dominant = False
            for i in range(8):
                c = cur["children"][i]
                if c is None:
                    continue
                if c["count"] / float(total) >= 0.95:
                    has_dominant = True
                    out.append(c["base"])
                    cur = c
                    break
            if not has_dominant:
                reached_leaf = False
                break
        return bytes(out), reached_leaf


def seed_paths(b, seed: int, trim_tail1: int = 0, records=None):
    """getAdapterWithSeed's two scans and walks (:485-520) on the raw reads: (forwardPath, backwardPath as the tree
    returns it, reachedLeaf, hits)"""
    shift_tail = max(1, trim_tail1)
    n = b.n if records is None else records
    reads = [b.seq[i, :int(b.lens[i])].tobytes() for i in range(n)]
    sseq = port.int2seq(seed)        # (the slice compare only saves time: seq2int gives the seed for these ten letters alone)
    hits = 0
    fwd = ByteTree()
    for r in reads:
        pos = 20
        while pos <= len(r) - 10 - shift_tail and pos < 500:
            if r[pos:pos + 10] == sseq and port.seq2int(r, pos) == seed:
                fwd.add_seq(r[pos + 10:pos + 10 + max(0, len(r) - 10 - shift_tail - pos)])
                hits += 1
            pos += 1
    reached_leaf = True
    fpath, reached_leaf = fwd.dominant_path(reached_leaf)
    bwd = ByteTree()
    for r in reads:
        pos = 20
        while pos <= len(r) - 10 - shift_tail and pos < 500:
            if r[pos:pos + 10] == sseq and port.seq2int(r, pos) == seed:
                bwd.add_seq(r[:pos][::-1])
            pos += 1
    bpath, reached_leaf = bwd.dominant_path(reached_leaf)
    return fpath, bpath, reached_leaf, hits


def eval_adapter(b, adapters, trim_tail1: int = 0, seeds=None) -> bytes:
    """evalAdapterAndReadNum's adapter (:356-481) for the batch, histogram included (evalport_adapter.eval_adapter with
    the byte tree above in getAdapterWithSeed).  seeds: a list that receives the keys getAdapterWithSeed was called for"""
    records = port.loaded_records(b)
    if records < 10000:
        return b""
    known = port.check_known_adapters(b.slice(0, records), adapters)[3]
    if len(known) > 8:
        return known
    counts, _ = evalport.adapter_kmer_counts(b, trim_tail1)
    topkeys, total = port.top_keys(counts, [int(k) for k in np.flatnonzero(counts)])
    for key in topkeys:
        if key == 0:
            continue
        count = int(counts[key])
        if count < 10 or count * (1 << 20) < total * 20:
            break
        seq = port.int2seq(key)
        if sum(1 for s in range(len(seq) - 1) if seq[s] != seq[s + 1]) < 3:
            continue
        if seeds is not None:
            seeds.append(key)
        fpath, bpath, reached_leaf, _ = seed_paths(b, key, trim_tail1, records)
        adapter = (bpath[::-1] + seq + fpath)[:60]
        matched = port.match_known_adapter(adapter, adapters)
        if matched:
            return matched
        if reached_leaf:
            return adapter
    return b""


def stats_overrep_report(reads, seeds, seqlen: int, sampling: int = 1) -> dict:
    """what fastp's report prints under "overrepresented_sequences" for the seed set `seeds` (Options::overRepSeqs):
    Stats::statRead's counting loop (stats.cpp:270-288 - a hit skips `step` positions, so overlapping seeds share the
    reads between them) over every `sampling`-th read, then Stats::overRepPassed (:519-533)"""
    counts = {k: 0 for k in seeds}
    steps = [10, 20, 40, 100, min(150, seqlen - 2)]
    for n, r in enumerate(reads):
        if n % sampling:
            continue
        for step in steps:
            i = 0
            while i < len(r) - step:
                sub = r[i:i + step]
                if sub in counts:
                    counts[sub] += 1
                    i += step
                i += 1
    need = {10: 500, 20: 200, 40: 100, 100: 50}
    return {k: c for k, c in counts.items() if sampling * c > need.get(len(k), 20)}
