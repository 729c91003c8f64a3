"""evalport_adapter.py - TEST INFRASTRUCTURE: a literal Python restatement of the adapter decision of the reference's
Evaluator (src/evaluator.cpp: checkKnownAdapters :220-306, the top-10 loop of evalAdapterAndReadNum :399-443,
getAdapterWithSeed :485-539, matchKnownAdapter :541-559) and of NucleotideTree (src/nucleotidetree.cpp:42-88), the
checker for fastp_gpu_eval_known_adapters / fastp_gpu_eval_adapter_seed and fastp_amd/evaluator.py.  Loops are kept
in the reference's order; nothing here is shared with the code under test.  Works on a hostloop.parse_fastq batch."""
import numpy as np


def _reads(b, n=None):
    n = b.n if n is None else n
    return [b.seq[i, :int(b.lens[i])].tobytes() for i in range(n)]


def first_match(r: bytes, adapter: bytes):
    """the loop :266-287 for one (read, adapter), behind its `alen >= rlen` skip (:260): (pos, mismatches) of the first
    fitting position, or None"""
    rlen, alen = len(r), len(adapter)
    if alen >= rlen:
        return None
    for pos in range(0, rlen - 8):
        cmplen = min(rlen - pos, alen)
        allowed = cmplen // 16
        mismatch = 0
        matched = True
        for i in range(cmplen):
            if adapter[i] != r[i + pos]:
                mismatch += 1
                if mismatch > allowed:
                    matched = False
                    break
        if matched:
            return pos, mismatch
    return None


def _first_match_np(rr: np.ndarray, aa: np.ndarray):
    """first_match with all positions compared at once (the same result: the early breaks only save time;
    test_eval_adapter.py holds the two against each other)"""
    rlen, alen = len(rr), len(aa)
    npos = rlen - 8
    if npos <= 0 or alen >= rlen:
        return None
    pad = np.zeros(rlen + alen, dtype=np.uint8)
    pad[:rlen] = rr
    win = np.lib.stride_tricks.sliding_window_view(pad, alen)[:npos]
    cmplen = np.minimum(rlen - np.arange(npos), alen)
    inside = np.arange(alen)[None, :] < cmplen[:, None]
    mismatch = ((win != aa[None, :]) & inside).sum(axis=1)
    ok = np.flatnonzero(mismatch <= cmplen // 16)
    if len(ok) == 0:
        return None
    return int(ok[0]), int(mismatch[ok[0]])


def match_table(b, known, n=None):
    """_first_match_np for every (read, adapter) of the batch, reads of one length taken together:
    {adapter: (pos int32[n], -1 = none; mismatches int32[n])}"""
    n = b.n if n is None else min(n, b.n)
    lens = np.asarray(b.lens[:n]).astype(np.int64)
    out = {a: (np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)) for a in known}
    for rlen in np.unique(lens):
        rlen = int(rlen)
        npos = rlen - 8
        if npos <= 0:
            continue
        rows = np.flatnonzero(lens == rlen)
        for a in known:
            alen = len(a)
            if alen >= rlen:
                continue
            aa = np.frombuffer(a, dtype=np.uint8)
            cmplen = np.minimum(rlen - np.arange(npos), alen)
            inside = np.arange(alen)[None, :] < cmplen[:, None]
            for c0 in range(0, len(rows), 2048):
                sel = rows[c0:c0 + 2048]
                pad = np.zeros((len(sel), rlen + alen), dtype=np.uint8)
                pad[:, :rlen] = b.seq[sel, :rlen]
                win = np.lib.stride_tricks.sliding_window_view(pad, alen, axis=1)[:, :npos]
                mismatch = ((win != aa[None, None, :]) & inside[None]).sum(axis=2)
                ok = mismatch <= (cmplen // 16)[None, :]
                has = ok.any(axis=1)
                first = ok.argmax(axis=1)
                out[a][0][sel[has]] = first[has]
                out[a][1][sel[has]] = mismatch[np.flatnonzero(has), first[has]]
    return out


def check_known_adapters(b, adapters, trace=None):
    """Evaluator::checkKnownAdapters over `adapters` (a list of distinct bytes, any order): returns
    (counts {adapter: n}, mismatches {adapter: n}, checkedReads, the adapter returned or b"").
    trace: a list that receives (read, adapter, "count" | "pruned") per matched pair the loop reached"""
    MAX_CHECK_READS = 100000
    MAX_CHECK_BASES = MAX_CHECK_READS * 1000
    MAX_HIT = 1000
    known = sorted(adapters)            # std::map<string, string>: byte order
    table = match_table(b, known, MAX_CHECK_READS)   # the inner loop :266-287 per (read, adapter): it reads no loop state

    def fitted(i, a):
        return (int(table[a][0][i]), int(table[a][1][i])) if table[a][0][i] >= 0 else None
    counts = {a: 0 for a in known}
    mism = {a: 0 for a in known}
    checked_reads = 0
    checked_bases = 0
    cur_max = 0
    for i in range(b.n):
        rlen = int(b.lens[i])
        checked_reads += 1
        checked_bases += rlen
        if checked_reads > MAX_CHECK_READS or checked_bases > MAX_CHECK_BASES:
            break
        if cur_max > MAX_HIT:
            break
        for a in known:
            if len(a) >= rlen:
                continue
            if cur_max > 20 and counts[a] < cur_max // 10:
                if trace is not None and fitted(i, a) is not None:
                    trace.append((i, a, "pruned"))
                continue
            m = fitted(i, a)
            if m is not None:
                counts[a] += 1
                if cur_max < counts[a]:
                    cur_max = counts[a]
                mism[a] += m[1]
                if trace is not None:
                    trace.append((i, a, "count"))
    adapter = b""
    max_count = 0
    for a in known:
        if counts[a] > max_count:
            adapter = a
            max_count = counts[a]
    if max_count > checked_reads // 50 or (max_count > checked_reads // 200 and mism.get(adapter, 0) < checked_reads):
        return counts, mism, checked_reads, adapter
    return counts, mism, checked_reads, b""


def eligible_key(k: int) -> bool:   # :404-422
    atcg = [0, 0, 0, 0]
    for i in range(10):
        atcg[(k >> (i * 2)) & 3] += 1
    if any(c >= 10 - 4 for c in atcg):
        return False
    if atcg[2] + atcg[3] >= 10 - 2:
        return False
    if k >> 12 == 0xff:
        return False
    return True


def top_keys(counts, keys=None):
    """the insertion loop :399-443 over `counts` (a sequence of 1 << 20): (topkeys[10], total).  `keys`: only these bins are
    visited (ascending) - the loop's result when every other eligible bin holds zero AND the caller accounts for the
    zero bins itself; None visits all 2^20 bins as the reference does"""
    topnum = 10
    topkeys = [0] * topnum
    total = 0
    for k in (range(1 << 20) if keys is None else keys):
        if not eligible_key(k):
            continue
        val = int(counts[k])
        total += val
        for t in range(topnum - 1, -1, -1):
            if val < int(counts[topkeys[t]]):
                if t < topnum - 1:
                    for m in range(topnum - 1, t + 1, -1):
                        topkeys[m] = topkeys[m - 1]
                    topkeys[t + 1] = k
                break
            elif t == 0:
                for m in range(topnum - 1, t, -1):
                    topkeys[m] = topkeys[m - 1]
                topkeys[t] = k
    return topkeys, total


def int2seq(val: int, seqlen: int = 10) -> bytes:   # :561-571
    out = bytearray(b"N" * seqlen)
    for done in range(seqlen):
        out[seqlen - done - 1] = b"ATCG"[val & 3]
        val >>= 2
    return bytes(out)


def seq2int(seq: bytes, pos: int, keylen: int = 10) -> int:   # :577-625 (a pure function of the window)
    key = 0
    for i in range(pos, pos + keylen):
        c = seq[i:i + 1]
        if c not in (b"A", b"T", b"C", b"G"):
            return -1
        key = (key << 2) + b"ATCG".index(c)
    return key


class NucleotideTree:   # nucleotidetree.cpp
    def __init__(self):
        self.root = {"count": 0, "base": "N", "children": [None] * 8}

    def add_seq(self, seq: bytes):
        cur = self.root
        for ch in seq:
            if ch == ord("N"):
                break
            base = ch & 0x07
            if cur["children"][base] is None:
                cur["children"][base] = {"count": 0, "base": chr(ch), "children": [None] * 8}
            cur["children"][base]["count"] += 1
            cur = cur["children"][base]

    def dominant_path(self, reached_leaf: bool):
        out = []
        cur = self.root
        while True:
            total = sum(c["count"] for c in cur["children"] if c is not None)
            if total < 50:
                break
            has_dominant = False
            for c in cur["children"]:
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
        return "".join(out).encode(), reached_leaf


def seed_paths(b, seed: int, trim_tail1: int = 0, records=None):
    """the two scans and walks of getAdapterWithSeed :485-520: (forwardPath, backwardPath as the tree returns it,
    reachedLeaf, hits)"""
    shift_tail = max(1, trim_tail1)
    reads = _reads(b, records)
    sseq = int2seq(seed)
    hits = 0
    fwd = NucleotideTree()
    for r in reads:
        pos = 20
        while pos <= len(r) - 10 - shift_tail and pos < 500:
            if r[pos:pos + 10] == sseq and seq2int(r, pos) == seed:
                fwd.add_seq(r[pos + 10:pos + 10 + max(0, len(r) - 10 - shift_tail - pos)])
                hits += 1
            pos += 1
    reached_leaf = True
    fpath, reached_leaf = fwd.dominant_path(reached_leaf)
    bwd = NucleotideTree()
    for r in reads:
        pos = 20
        while pos <= len(r) - 10 - shift_tail and pos < 500:
            if r[pos:pos + 10] == sseq and seq2int(r, pos) == seed:
                bwd.add_seq(r[:pos][::-1])
            pos += 1
    bpath, reached_leaf = bwd.dominant_path(reached_leaf)
    return fpath, bpath, reached_leaf, hits


def match_known_adapter(seq: bytes, adapters) -> bytes:   # :541-559
    for a in sorted(adapters):
        if len(seq) < len(a):
            continue
        diff = 0
        for i in range(min(len(a), len(seq))):
            if a[i] != seq[i]:
                diff += 1
        if diff == 0:
            return a
    return b""


def get_adapter_with_seed(b, seed: int, adapters, trim_tail1: int = 0, records=None) -> bytes:   # :485-539
    fpath, bpath, reached_leaf, _ = seed_paths(b, seed, trim_tail1, records)
    adapter = bpath[::-1] + int2seq(seed) + fpath
    if len(adapter) > 60:
        adapter = adapter[:60]
    matched = match_known_adapter(adapter, adapters)
    if matched:
        return matched
    return adapter if reached_leaf else b""


def loaded_records(b) -> int:   # the loading loop :328-343
    READ_LIMIT = 256 * 1024
    BASE_LIMIT = 151 * READ_LIMIT
    records = bases = 0
    while records < READ_LIMIT and bases < BASE_LIMIT and records < b.n:
        bases += int(b.lens[records])
        records += 1
    return records


def eval_adapter(b, adapters, counts, trim_tail1: int = 0) -> bytes:
    """evalAdapterAndReadNum's adapter decision (:356-481) given the ten-mer histogram `counts` of the loaded reads
    (tests/evalport.py adapter_kmer_counts restates that loop).  The top-10 loop visits the non-zero bins and ten zero
    ones: a zero bin never displaces a non-zero one, and zero bins among the top ten end the loop below (count < 10)."""
    records = loaded_records(b)
    if records < 10000:
        return b""
    sub = b.slice(0, records)
    known = check_known_adapters(sub, adapters)[3]
    if len(known) > 8:
        return known
    size = 1 << 20
    nz = [int(k) for k in np.flatnonzero(counts)]
    topkeys, total = top_keys(counts, nz)
    for key in topkeys:
        if key == 0:
            continue
        count = int(counts[key])
        if count < 10 or count * size < total * 20:
            break
        seq = int2seq(key)
        diff = sum(1 for s in range(len(seq) - 1) if seq[s] != seq[s + 1])
        if diff < 3:
            continue
        adapter = get_adapter_with_seed(b, key, adapters, trim_tail1, records)
        if adapter:
            return adapter
    return b""
