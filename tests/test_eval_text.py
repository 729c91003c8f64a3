"""The Evaluator pre-pass on samples with letters outside ACGTN (soft-masked lower case, IUPAC codes, '.'): the text-aware
forms fastp_gpu_eval_adapter_kmers_x / _known_adapters_x / _adapter_seed_x / _overrep_x (csrc/fq_eval.h) and what
fastp_amd/evaluator.py builds from them, against the literal restatement of the reference's loops on the raw text
(tests/evalport.py, evalport_adapter.py, evalport_text.py).  Every family runs on the emulator (test_sim_*) and, with the
same cases at the same sizes, on the GPU (test_gpu_*).  All comparisons are exact.

Every case first shows, on the ports alone, that its input DISCRIMINATES: the port's answer on the raw text differs from
its answer on the text the packed rows describe (every byte outside ACGTN an 'A' - evalport_text.as_packed), which is
what the packed-only kernels answer for."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import engines
import evalport
import evalport_adapter as port
import evalport_text as xport
import synth
from fastp_amd import abi, evaluator, hostloop

_CACHE: dict = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _rnd(rng, n) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def _put(s: bytes, at: int, what: bytes) -> bytes:
    return s[:at] + what + s[at + len(what):]


def _lower(s: bytes, a: int, b: int) -> bytes:
    return s[:a] + s[a:b].lower() + s[b:]


def _other(b: int) -> bytes:
    return b"ACGT"[(b"ACGT".index(b) + 2) % 4:][:1]


def _fastq(reads) -> bytes:
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


def _mem(mk):
    import format_util
    return format_util.NumpyMem() if mk is engines.sim_engine else format_util.TorchMem()


class _Rows:
    """FASTQ text -> fastp_gpu_parse_fastq -> packed rows in `mem`, with the chunk, its line table and the parser's list
    of records with letters outside ACGTN kept for the _x calls; beside it the same text decoded on the host"""

    def __init__(self, g, mem, fq, max_len):
        n = fq.count(b"\n") // 4
        self.ss, self.qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
        cap = n + 2
        self.text = mem.upload(fq, (-len(fq)) % 16 + 16)
        self.seq, self.qual = mem.alloc(cap * self.ss), mem.alloc(cap * self.qs)
        self.lens, self.loff, llen = mem.alloc(cap * 2), mem.alloc(cap * 16), mem.alloc(cap * 16)
        mem.sync()
        info = g.parse_fastq(mem.ptr(self.text), len(fq), True, cap, mem.ptr(self.seq), mem.ptr(self.qual), mem.ptr(self.lens),
                             mem.ptr(self.loff), mem.ptr(llen))
        assert info.first_bad == -1 and info.n_records == n
        self.mem, self.n, self.fq = mem, n, fq
        self.units = g.parse_exotic().copy()
        assert info.n_exotic == len(self.units)
        self.b = hostloop.parse_fastq(fq, self.qs)
        assert np.array_equal(self.units, xport.listed(self.b))      # the parser lists exactly the reads the port calls listed

    def ptrs(self):
        m = self.mem
        return m.ptr(self.seq), m.ptr(self.qual), m.ptr(self.lens)

    def exotic(self):
        """the dense form: the chunk and the parser's line_off table"""
        return self.units, self.mem.ptr(self.text), self.mem.ptr(self.loff), True

    def exotic_sparse(self):
        """the other form: one byte offset per listed read"""
        starts, at = [], 0
        for i, line in enumerate(self.fq.split(b"\n")[:-1]):
            if i % 4 == 1:
                starts.append(at)
            at += len(line) + 1
        off = np.array([starts[u] for u in self.units], dtype=np.uint32)
        self._off = self.mem.upload(off.tobytes(), 16)
        self.mem.sync()
        return self.units, self.mem.ptr(self.text), self.mem.ptr(self._off), False


def _reads_rows(g, mem, reads, max_len):
    return _Rows(g, mem, _fastq(reads), max_len)


def _histogram(g, mem, rows, trim, exotic):
    c = mem.alloc(4 << 20)
    mem.sync()
    rec = g.eval_adapter_kmers(*rows.ptrs(), rows.n, trim, mem.ptr(c), exotic=exotic)
    return np.frombuffer(mem.download(c, 4 << 20), dtype=np.uint32), rec


# ---- 1. the ten-mer histogram -----------------------------------------------------------------------------------
FOREIGN = (b"a", b"c", b"g", b"t", b"n", b"R", b".")


def _histogram_reads():
    """reads of 76 with one foreign byte at positions 19, 20 (the first window and the base in front of it), 29, 30 (its far
    edge), and at len - 10 - shift - 1 .. + 1 (the last admitted window's first base and its neighbours) for shift 1 and 3;
    a soft-masked read next to the same text in upper case"""
    rng = np.random.default_rng(211)
    L = 76
    spots = [19, 20, 29, 30] + [L - 10 - sh + d for sh in (1, 3) for d in (-1, 0, 1)] + [L - 1 - 1, L - 3 - 1, L - 3]
    reads = []
    for at in spots:
        for f in FOREIGN:
            r = _rnd(rng, L)
            reads.append(_put(r, at, r[at:at + 1].lower() if f in b"acgt" else f))
    up = _rnd(rng, L)
    reads += [_lower(up, 25, 50), up, up.lower(), up]
    assert len(reads) <= 128
    return reads


def _run_histogram(mk):
    g, mem = mk(abi.default_params(False, 76)), _mem(mk)
    try:
        rows = _reads_rows(g, mem, _histogram_reads(), 76)
        assert 0 < len(rows.units) < rows.n and rows.units[-2] + 1 not in rows.units       # a listed read next to an unlisted one
        for trim in (0, 3):
            want, wrec = _cached(("hist", trim), lambda: evalport.adapter_kmer_counts(rows.b, trim))
            blind = _cached(("hist-packed", trim), lambda: evalport.adapter_kmer_counts(xport.as_packed(rows.b), trim))[0]
            assert not np.array_equal(want, blind) and int(blind.sum()) > int(want.sum())          # discriminates
            got, rec = _histogram(g, mem, rows, trim, rows.exotic())
            assert rec == wrec and np.array_equal(got, want), trim
            got, rec = _histogram(g, mem, rows, trim, rows.exotic_sparse())
            assert np.array_equal(got, want), trim
            plain, _ = _histogram(g, mem, rows, trim, None)
            assert np.array_equal(plain, blind)          # ... and the plain call is the packed rows' answer, as before
    finally:
        g.close()


def test_sim_text_histogram():
    _run_histogram(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_histogram")
def test_gpu_text_histogram():
    _run_histogram(engines.gpu_engine)


# ---- 2. known adapters ------------------------------------------------------------------------------------------
X12, Y12 = b"ACCGTTAGCATG", b"TGGATCCTAGCA"          # X before Y in map order; 12 bases: no mismatch allowed
A32 = b"GATCAGTACCATGACTGACATTGCAGTCAGGA"             # 32 bases: two mismatches allowed over the whole of it
FILL = b"CTCTTCTCCTTCTCTCCT"                          # holds none of them, nor a tail of 9 of any


def _carry(*ads) -> bytes:
    r = FILL[:6]
    for a in ads:
        r += a + FILL[:5]
    return r + FILL[:4]


def _sub(a: bytes, at) -> bytes:
    """regular mismatches: another base at each position"""
    for i in at:
        a = _put(a, i, _other(a[i]))
    return a


def _known_geometry_reads():
    """[(read, adapter, first_match on the raw text, first_match on the packed rows' text)]"""
    a_at = [i for i in range(32) if A32[i:i + 1] == b"A"]
    assert len(a_at) >= 4 and a_at[1] < 20
    f0, f1 = a_at[0], a_at[1]
    cases = []
    # matches only if 'a' were 'A': must not count
    cases.append((_carry(_put(X12, 0, b"a")), X12, None, (6, 0)))
    # a foreign byte inside the cmplen / 16 allowance: counts, and the mismatch is added
    cases.append((_carry(_put(A32, f0, b"R")), A32, (6, 1), (6, 0)))
    cases.append((_carry(_put(_sub(A32, [9]), f0, b"a")), A32, (6, 2), (6, 1)))
    # one foreign byte beyond the allowance
    cases.append((_carry(_put(_sub(A32, [9, 21]), f0, b".")), A32, None, (6, 2)))
    # the shortened compare at the read's end: 20 bases left, one mismatch allowed
    head = FILL + FILL
    cases.append((head + _put(A32[:20], f1, b"n"), A32, (36, 1), (36, 0)))
    cases.append((head + _put(_sub(A32[:20], [3]), f1, b"n"), A32, None, (36, 1)))
    return cases


def _known_replay_reads():
    """the skip rule (curMaxCount > 20, count < curMaxCount / 10) with listed reads among the hits: soft-masked filler
    around an intact adapter still hits; Y's third read comes when curMaxCount is 30 and is skipped.  A read whose X
    has its A's soft-masked does not count - on the packed rows it would, and the skip would come one read earlier"""
    rx, ry = _carry(X12), _carry(Y12)
    rx_l, ry_l = _lower(rx, 0, 5), _lower(ry, 0, 5)
    masked = _carry(X12.replace(b"A", b"a"))
    return [ry, ry_l] + [rx, rx_l] * 10 + [masked] + [rx_l, rx] * 5 + [ry_l, ry]


def _known_equal(g, rows, adapters, want):
    wc, wm, wchecked, wbest = want
    rc, counts, mism, checked, best = g.eval_known_adapters(*rows.ptrs(), rows.n, adapters, exotic=rows.exotic())
    assert rc == 0
    assert [int(x) for x in counts] == [wc[a] for a in adapters]
    assert [int(x) for x in mism] == [wm[a] for a in adapters]
    assert checked == wchecked
    assert (adapters[best] if best >= 0 else b"") == wbest


def _run_known(mk):
    g, mem = mk(abi.default_params(False, 64)), _mem(mk)
    try:
        ads = [Y12, A32, X12]                        # (given in another order than the map's)
        cases = _known_geometry_reads()
        for read, hit, raw, packed in cases:
            assert port.first_match(read, hit) == raw, read
            assert port.first_match(xport.as_packed(hostloop.parse_fastq(_fastq([read]), 64)).seq[0, :len(read)].tobytes(), hit) == packed
            assert raw != packed                                                           # discriminates
            rows = _reads_rows(g, mem, [read], 64)   # alone: n = 1, no pruning - the match kernel's own result
            _known_equal(g, rows, ads, port.check_known_adapters(rows.b, ads))
        rows = _reads_rows(g, mem, [c[0] for c in cases] + [_carry(X12), _carry(A32)], 64)
        want = _cached("known-geometry", lambda: port.check_known_adapters(rows.b, ads))
        assert want[0] == {X12: 1, Y12: 0, A32: 4} and want[1][A32] == 1 + 2 + 1
        assert _cached("known-geometry-packed", lambda: port.check_known_adapters(xport.as_packed(rows.b), ads))[:2] != want[:2]
        _known_equal(g, rows, ads, want)
        # the replay
        reads = _known_replay_reads()
        rows = _reads_rows(g, mem, reads, 64)
        trace = []
        want = _cached("known-replay", lambda: port.check_known_adapters(rows.b, [Y12, X12], trace))
        if trace:
            assert [t for t in trace if t[1] == Y12][-2:] == [(len(reads) - 2, Y12, "pruned"), (len(reads) - 1, Y12, "pruned")]
            assert sum(1 for t in trace if t[1] == X12 and t[2] == "count" and t[0] in rows.units) >= 10   # listed reads among the hits
        assert want[0] == {X12: 30, Y12: 2}
        blind = _cached("known-replay-packed", lambda: port.check_known_adapters(xport.as_packed(rows.b), [Y12, X12]))
        assert blind[0] == {X12: 31, Y12: 2}                                               # discriminates
        _known_equal(g, rows, [Y12, X12], want)
    finally:
        g.close()


def test_sim_text_known_adapters():
    _run_known(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_known_adapters")
def test_gpu_text_known_adapters():
    _run_known(engines.gpu_engine)


# ---- 3. seed walks ----------------------------------------------------------------------------------------------
SEED = b"ACGTTGCAAG"
LEFT = b"CTGACCTAGTCATGGTCCATGCTAG"                  # 25 bases in front of the seed; backward depth d is LEFT[24 - d]
EXT = b"GATCCTTGCAATCGGATACCGTTAGCCTGA"              # 30 bases behind it; forward depth d is EXT[d]
BASE = LEFT + SEED + EXT + b"T"                       # (trim_tail1 0: the last base is not part of the forward sequence)
F0, B0 = 35, 24                                       # forward depth d is BASE[F0 + d], backward depth d is BASE[B0 - d]


def _seed_cases():
    """[(name, reads, check(fwd, bwd, leaf, hits) on the port's result)]; 65 - 130 hits each, so a wavefront is crossed"""
    assert BASE[25:35] == SEED and BASE.count(SEED[:5]) == 1 and len(BASE) == 66
    assert EXT[9:10] == b"A" and EXT[3:4] != b"A" and LEFT[B0 - 3:B0 - 2] != b"A"
    out = []

    def low_at(r, *at):
        for i in at:
            r = _lower(r, i, i + 1)
        return r
    alt = _put(_put(BASE, F0 + 3, _other(BASE[F0 + 3])), B0 - 3, _other(BASE[B0 - 3]))
    low = low_at(BASE, F0 + 3, B0 - 3)
    # a node created by a lower-case byte; its bin reaches 95 % only with the upper-case hits: 5 + 93 of 100
    fl = _lower(EXT, 3, 4)
    bl = _lower(LEFT[::-1], 3, 4)
    out.append(("lower_creates", [low] * 5 + [BASE] * 93 + [alt] * 2,
                lambda f, b, leaf, hits: (f, b, leaf, hits) == (fl, bl, True, 100) or pytest.fail("the creator's byte is lower case")))
    # ... created by the upper-case byte first: the other character
    out.append(("upper_creates", [BASE] + [low] * 5 + [BASE] * 92 + [alt] * 2,
                lambda f, b, leaf, hits: (f, b, leaf, hits) == (EXT, LEFT[::-1], True, 100) or pytest.fail("the creator's byte is upper case")))
    # 'n' goes on (bin 6, printed as it is) where 'N' cuts
    n5 = _put(_put(BASE, F0 + 5, b"n"), B0 - 5, b"n")
    N5 = _put(_put(BASE, F0 + 5, b"N"), B0 - 5, b"N")
    out.append(("n_goes_on", [N5] * 4 + [n5] * 96 + [BASE] * 2,
                lambda f, b, leaf, hits: (f, b, leaf, hits) == (_put(EXT, 5, b"n"), _put(LEFT[::-1], 5, b"n"), True, 102) or pytest.fail("n goes on, N cuts")))
    # dominant bins 0, 2 and 5: H, R, M
    hrm = BASE
    for d, ch in ((2, b"H"), (4, b"R"), (6, b"M")):
        hrm = _put(_put(hrm, F0 + d, ch), B0 - d, ch)
    fw, bw = EXT, LEFT[::-1]
    for d, ch in ((2, b"H"), (4, b"R"), (6, b"M")):
        fw, bw = _put(fw, d, ch), _put(bw, d, ch)
    assert [c & 7 for c in b"HRM"] == [0, 2, 5]
    out.append(("bins_0_2_5", [BASE] * 3 + [hrm] * 97,
                lambda f, b, leaf, hits: (f, b, leaf, hits) == (fw, bw, True, 100) or pytest.fail("H, R and M dominate their depths")))
    # two bins split 94 / 6 at a depth whose base is 'A': on the packed rows the R would be an A and the walk would go on
    split = _put(BASE, F0 + 9, b"R")
    out.append(("split_94_6", [BASE] * 94 + [split] * 6,
                lambda f, b, leaf, hits: (f, b, leaf, hits) == (EXT[:9], LEFT[::-1], False, 100) or pytest.fail("94 of 100 must stop")))
    # hits of one read at two positions, the first soft-masked in the first reads: read 0's first hit creates the nodes
    two = LEFT + SEED + EXT[:12] + SEED + EXT + b"T"
    two_l = _lower(two, F0 + 3, F0 + 4)

    def check_two(f, b, leaf, hits):
        assert hits == 80 and f == fl[:12] and not leaf       # (behind EXT[:12] the two positions' sequences part 40 / 40)
    out.append(("two_hits", [two_l] * 3 + [two] * 37, check_two))
    return out


def _run_seed(mk):
    g, mem = mk(abi.default_params(False, 120)), _mem(mk)
    key = port.seq2int(SEED, 0)
    try:
        for name, reads, check in _seed_cases():
            rows = _reads_rows(g, mem, reads, 120)
            want = _cached(("seed", name), lambda: xport.seed_paths(rows.b, key, 0))
            check(*want)
            assert 65 <= want[3] <= 130
            blind = _cached(("seed-packed", name), lambda: xport.seed_paths(xport.as_packed(rows.b), key, 0))
            assert blind != want, name                                                     # discriminates
            rc, fwd, bwd, leaf, hits = g.eval_adapter_seed(*rows.ptrs(), rows.n, 0, key, exotic=rows.exotic())
            assert (fwd, bwd, leaf, hits) == want, name
    finally:
        g.close()


def test_sim_text_seed_walks():
    _run_seed(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_seed_walks")
def test_gpu_text_seed_walks():
    _run_seed(engines.gpu_engine)


# ---- 4. the substring census ------------------------------------------------------------------------------------
def _census_reads():
    """seq_len 42: steps 10, 20, 40, (100,) 40 - a 40-mer is counted twice per occurrence, as the reference's loop does.
    U (50 bases) 500 times passes every class (500 / 500 / 1000); its twin, soft-masked from base 44 on, 120 times passes
    the 20 and 40 classes with the windows that touch the mask and adds to U's counts with the others"""
    rng = np.random.default_rng(223)
    U = _rnd(rng, 50)
    twin = _lower(U, 44, 50)
    noise = []
    for i in range(60):
        r = _rnd(rng, int(rng.integers(44, 61)))
        if i % 3 == 0:
            r = _put(r, int(rng.integers(0, len(r))), FOREIGN[i % len(FOREIGN)])
        noise.append(r)
    reads = [U] * 500 + [twin] * 120 + noise
    order = np.random.default_rng(5).permutation(len(reads))
    return [reads[i] for i in order], U, twin


def _run_census(mk):
    g, mem = mk(abi.default_params(False, 64)), _mem(mk)
    try:
        reads, U, twin = _census_reads()
        rows = _reads_rows(g, mem, reads, 64)
        want = _cached("census", lambda: evalport.evaluate_overrep_counts(rows.b, 42))
        keys = list(want)
        assert keys == sorted(keys)
        # different keys, neither absorbs the other; a window in front of the mask is one key for both kinds of read
        assert U[:40] == twin[:40] and want[U[:40]] == 2 * 620 and want[U[9:49]] == 2 * 500 and want[twin[9:49]] == 2 * 120
        # a kept long key contains a shorter one, both with foreign bytes, count / count2 < 10: the shorter one is gone
        assert twin[28:48] != U[28:48] and twin[28:48] not in want and twin[28:48] in twin[9:49]
        # byte order: upper case before lower case
        up, low = U[5:45], twin[5:45]
        assert up[:10] == low[:10] and keys.index(up) < keys.index(low)
        blind = _cached("census-packed", lambda: evalport.evaluate_overrep_counts(xport.as_packed(rows.b), 42))
        assert blind != want and twin[9:49] not in blind                                    # discriminates
        rc, got = g.eval_overrep(*rows.ptrs(), rows.n, 42, exotic=rows.exotic())
        assert rc == 0 and got == list(want.items())
        rc, found = g.eval_overrep(*rows.ptrs(), rows.n, 42, max_seqs=2, check=False, exotic=rows.exotic())
        assert rc == abi.E_OVERFLOW and found == len(want)
    finally:
        g.close()


def test_sim_text_census():
    _run_census(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_census")
def test_gpu_text_census():
    _run_census(engines.gpu_engine)


# ---- the 11000-read samples -------------------------------------------------------------------------------------
CUSTOM = b"CTGACCTAGTCAAGGTCCATGCTAGGATCCATGCAAT"      # on nobody's list
LISTED = [synth.ADAPTER_R1, synth.ADAPTER_R2, b"GATCGTCGGACTGTAGAACTCTGAACGTGTAGA", b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGGGTGCCAAGG"]


def _plain_reads(variant):
    """the "listed" and "custom" samples of test_eval_adapter.py: 11000 x 76 single-end, TruSeq behind inserts of ~50, or
    an adapter on nobody's list behind the last 30..44 bases of one amplicon"""
    if variant == "listed":
        d = synth.synth_pairs(11000, L=76, seed=61, paired=False, dup_frac=0.0, insert_mean=50.0, insert_sd=12.0)
        return d["seq1"], d["qual1"], d["len1"], None
    rng = np.random.default_rng(62)
    n, L = 11000, 76
    amp = np.frombuffer(_rnd(rng, 44), dtype=np.uint8)
    tail = np.concatenate([np.frombuffer(CUSTOM, dtype=np.uint8), np.full(L, ord("A"), dtype=np.uint8)])
    seq = np.zeros((n, 80), dtype=np.uint8)
    ins = rng.integers(30, 45, size=n)
    for i in range(n):
        seq[i, :L] = np.concatenate([amp[44 - ins[i]:], tail])[:L]
    err = rng.random((n, L)) < 0.01
    seq[:, :L] = np.where(err, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))], seq[:, :L])
    qual = np.zeros((n, 80), dtype=np.uint8)
    qual[:, :L] = ord("I")
    return seq, qual, np.full(n, L, dtype=np.int32), ins


def _plain_fastq(variant) -> bytes:
    return _cached(("fq", variant), lambda: synth.to_fastq(*_plain_reads(variant)[:3], 1))


def _masked_fastq(variant) -> bytes:
    """12 - 15 % of the reads soft-masked in a stretch inside the insert - somewhere in bases 14 .. 29 of reads whose
    adapter starts at base 30 or later, so the histogram's first windows (from base 20 on) see it; "custom_lower": also the first hit of the seed lower case in the adapter itself, beside the seed's window"""
    def build():
        seq, qual, lens, ins = _plain_reads("listed" if variant == "listed" else "custom")
        seq = seq.copy()
        rng = np.random.default_rng(63)
        if ins is None:      # "listed": where the adapter shows
            head = np.frombuffer(synth.ADAPTER_R1[:10], dtype=np.uint8)
            win = np.lib.stride_tricks.sliding_window_view(seq[:, :76], 10, axis=1)
            found = (win == head).all(axis=2)
            ins = np.where(found.any(axis=1), found.argmax(axis=1), 0)
        share = 0.135 * len(lens) / int(((ins >= 30) & (lens == 76)).sum())
        pick = np.flatnonzero((rng.random(len(lens)) < share) & (ins >= 30) & (lens == 76) & (np.arange(len(lens)) >= 64))
        for i in pick:
            a = int(rng.integers(14, 22))
            seq[i, a:a + int(rng.integers(4, 9))] |= 0x20
        assert 0.12 <= len(pick) / len(lens) <= 0.15
        if variant == "custom_lower":
            seeds = []
            b = hostloop.parse_fastq(_masked_fastq("custom"), abi.qual_stride(76))
            assert xport.eval_adapter(b, LISTED, 0, seeds) and len(seeds) == 1
            s = CUSTOM.find(port.int2seq(seeds[0]))
            assert 0 <= s
            lo = s - 2 if s >= 2 else s + 10       # two adapter bases in front of the seed's window, or the two behind it
            assert lo + 2 <= 16
            at = int(ins[0]) + lo
            seq[0, at:at + 2] |= 0x20
        return synth.to_fastq(seq, qual, lens, 1)
    return _cached(("fq-masked", variant), build)


def _e2e_want(variant):
    fq = _masked_fastq(variant)

    def compute():
        b = hostloop.parse_fastq(fq, abi.qual_stride(76))
        want = xport.eval_adapter(b, LISTED, 0)
        blind_b = xport.as_packed(b)
        # discriminates: the ten-mer histogram always; the answer itself where it carries lower case
        assert not np.array_equal(evalport.adapter_kmer_counts(b, 0)[0], evalport.adapter_kmer_counts(blind_b, 0)[0])
        if variant == "listed":
            assert want == synth.ADAPTER_R1
        elif variant == "custom":
            assert len(want) == 60 and want.endswith(CUSTOM[:16]) and set(want) <= set(b"ACGT")
        else:
            assert len(want) == 60 and want.upper().endswith(CUSTOM[:16]) and want != want.upper()
            assert xport.eval_adapter(blind_b, LISTED, 0) != want
        return want
    return fq, _cached(("e2e", variant), compute)


# ---- 5. n_exotic == 0 and NULL are the plain calls --------------------------------------------------------------
def _run_equivalence(mk):
    g, mem = mk(abi.default_params(False, 76)), _mem(mk)
    try:
        for variant in ("listed", "custom"):
            rows = _Rows(g, mem, _plain_fastq(variant), 76)
            assert len(rows.units) == 0
            p, n = rows.ptrs(), rows.n
            empty = (np.zeros(0, dtype=np.int32), 0, 0, False)
            null = (None, 0, 0, False)
            plain_h, rec = _histogram(g, mem, rows, 0, None)
            assert rec == n and plain_h.sum() > 0
            key = evaluator.top_seeds(plain_h)[0][0]
            few = 3000                               # (the two slow ones on the emulator: the first 3000 reads)
            plain_k = g.eval_known_adapters(*p, few, LISTED)
            plain_s = g.eval_adapter_seed(*p, n, 0, key)
            plain_o = g.eval_overrep(*p, few, 76)
            assert plain_s[4] >= 50 and (variant != "listed" or plain_k[4] == 0) and len(plain_o[1]) > 0
            for x in (empty, null):
                h, r = _histogram(g, mem, rows, 0, x)
                assert r == rec and np.array_equal(h, plain_h)
                k = g.eval_known_adapters(*p, few, LISTED, exotic=x)
                assert [list(map(int, v)) if isinstance(v, np.ndarray) else v for v in k] == \
                       [list(map(int, v)) if isinstance(v, np.ndarray) else v for v in plain_k]
                assert g.eval_adapter_seed(*p, n, 0, key, exotic=x) == plain_s
                assert g.eval_overrep(*p, few, 76, exotic=x) == plain_o
    finally:
        g.close()


def test_sim_text_calls_without_a_list_are_the_plain_calls():
    _run_equivalence(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_calls_without_a_list_are_the_plain_calls")
def test_gpu_text_calls_without_a_list_are_the_plain_calls():
    _run_equivalence(engines.gpu_engine)


# ---- 6. argument checks -----------------------------------------------------------------------------------------
def _run_argument_checks(mk):
    g, mem = mk(abi.default_params(False, 64)), _mem(mk)
    try:
        reads = [_carry(X12), _lower(_carry(X12), 0, 4), _carry(Y12), _lower(_carry(Y12), 0, 4)]
        rows = _reads_rows(g, mem, reads, 64)
        assert list(rows.units) == [1, 3]
        p, n = rows.ptrs(), rows.n
        _, text, loff, _ = rows.exotic()
        counts_dev = mem.alloc(4 << 20, fill=0x5A)
        mem.sync()

        def x_of(units, text=text, off=loff, n_exotic=None):
            u = np.array(units, dtype=np.int32)
            x = abi.EvalText(len(u) if n_exotic is None else n_exotic, 1, u.ctypes.data if len(u) else None, text, off)
            x.keep = u
            return x
        bad = {"descending": x_of([3, 1]), "twice": x_of([1, 1]), "negative": x_of([-1, 1]), "index n": x_of([1, n]),
               "no text": x_of([1, 3], text=None), "no offsets": x_of([1, 3], off=None), "negative count": x_of([1, 3], n_exotic=-1),
               "no list": x_of([], n_exotic=2)}
        lib = g.lib
        VP, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
        XP = C.POINTER(abi.EvalText)
        lib.fastp_gpu_eval_adapter_kmers_x.argtypes = [VP, VP, VP, VP, I32, I32, VP, C.POINTER(I64), XP]
        lib.fastp_gpu_eval_known_adapters_x.argtypes = [VP, VP, VP, VP, I32, C.POINTER(C.c_char_p), I32, VP, VP, C.POINTER(I64), C.POINTER(I32), XP]
        lib.fastp_gpu_eval_adapter_seed_x.argtypes = [VP, VP, VP, VP, I32, I32, C.c_uint32, VP, C.POINTER(I32), VP, C.POINTER(I32),
                                                      C.POINTER(I32), C.POINTER(I64), XP]
        lib.fastp_gpu_eval_overrep_x.argtypes = [VP, VP, VP, VP, I32, I32, C.c_char_p, I64, C.POINTER(I64), C.POINTER(I64), I32, C.POINTER(I32), XP]
        for fn in (lib.fastp_gpu_eval_adapter_kmers_x, lib.fastp_gpu_eval_known_adapters_x, lib.fastp_gpu_eval_adapter_seed_x, lib.fastp_gpu_eval_overrep_x):
            fn.restype = C.c_int
        ads = (C.c_char_p * 2)(X12, Y12)

        def calls(x):
            """the four calls with every output preset to a pattern: [(name, rc, outputs as bytes)]"""
            xr = C.byref(x)
            out = []
            rec = I64(-7)
            rc = lib.fastp_gpu_eval_adapter_kmers_x(g.h, *p, n, 0, mem.ptr(counts_dev), C.byref(rec), xr)
            out.append(("kmers", rc, bytes(rec) + mem.download(counts_dev, 4 << 20)))
            cnt, mis, chk, best = (I32 * 2)(-7, -7), (I32 * 2)(-7, -7), I64(-7), I32(-7)
            rc = lib.fastp_gpu_eval_known_adapters_x(g.h, *p, n, ads, 2, C.addressof(cnt), C.addressof(mis), C.byref(chk), C.byref(best), xr)
            out.append(("known", rc, bytes(cnt) + bytes(mis) + bytes(chk) + bytes(best)))
            fwd, bwd = C.create_string_buffer(b"\x5a" * 511), C.create_string_buffer(b"\x5a" * 511)
            i32 = [I32(-7) for _ in range(3)]
            hits = I64(-7)
            rc = lib.fastp_gpu_eval_adapter_seed_x(g.h, *p, n, 0, 5, fwd, C.byref(i32[0]), bwd, C.byref(i32[1]), C.byref(i32[2]), C.byref(hits), xr)
            out.append(("seed", rc, fwd.raw + bwd.raw + b"".join(bytes(v) for v in i32) + bytes(hits)))
            text_out = C.create_string_buffer(b"\x5a" * 255)
            off, cnt64, ns = (I64 * 5)(*[-7] * 5), (I64 * 4)(*[-7] * 4), I32(-7)
            rc = lib.fastp_gpu_eval_overrep_x(g.h, *p, n, 30, text_out, 256, off, cnt64, 4, C.byref(ns), xr)
            out.append(("overrep", rc, text_out.raw + bytes(off) + bytes(cnt64) + bytes(ns)))
            return out
        untouched = None
        for what, x in bad.items():
            res = calls(x)
            assert [rc for _, rc, _ in res] == [abi.E_INVALID] * 4, what
            blobs = [blob for _, _, blob in res]
            untouched = untouched or blobs
            assert blobs == untouched, what                  # the preset patterns, every time
        good = calls(x_of([1, 3]))
        assert [rc for _, rc, _ in good] == [0] * 4 and all(a != b for a, b in zip([blob for _, _, blob in good], untouched))
    finally:
        g.close()


def test_sim_text_argument_checks():
    _run_argument_checks(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_argument_checks")
def test_gpu_text_argument_checks():
    _run_argument_checks(engines.gpu_engine)


# ---- 7. detect_adapter end to end -------------------------------------------------------------------------------
def _run_e2e(mk):
    g, mem = mk(abi.default_params(False, 76)), _mem(mk)
    try:
        for variant in ("listed", "custom", "custom_lower"):
            fq, want = _e2e_want(variant)
            rows = _Rows(g, mem, fq, 76)
            assert rows.n == 11000 and 0.12 <= len(rows.units) / rows.n <= 0.15
            got = evaluator.detect_adapter(g, *rows.ptrs(), rows.n, LISTED[::-1], 0, exotic=rows.exotic())
            assert got == want, variant
    finally:
        g.close()


def test_sim_text_detect_adapter_end_to_end():
    _run_e2e(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_text_detect_adapter_end_to_end")
def test_gpu_text_detect_adapter_end_to_end():
    _run_e2e(engines.gpu_engine)


# ---- 8. files, and the reference itself -------------------------------------------------------------------------
def test_sim_text_detect_adapter_in_file(tmp_path):
    """a plain and a gzip-compressed soft-masked file through detect_adapter_in_file and overrep_in_file on the emulator"""
    fq, want = _e2e_want("custom_lower")
    plain, gz = tmp_path / "in.fq", tmp_path / "in.fq.gz"
    plain.write_bytes(fq)
    gz.write_bytes(gzip.compress(fq, 1))
    lib = engines.build_sim()
    assert evaluator.detect_adapter_in_file(str(plain), LISTED, lib_path=lib) == want
    assert evaluator.detect_adapter_in_file(str(gz), LISTED, lib_path=lib) == want
    b = hostloop.parse_fastq(fq, abi.qual_stride(76))
    census = _cached("file-census", lambda: evalport.evaluate_overrep_counts(b, 76))
    assert any(k != k.upper() for k in census)
    assert census != _cached("file-census-packed", lambda: evalport.evaluate_overrep_counts(xport.as_packed(b), 76))   # discriminates
    assert evaluator.overrep_in_file(str(gz), 76, lib_path=lib) == census


REF = os.path.join(engines.ROOT, "oracle", "_ref", "fastp_ref")
REF_LIST = "/root/reference/src/knownadapters.h"


@pytest.mark.parametrize("variant", ["listed", "custom", "custom_lower"])
def test_text_in_file_equals_reference(variant, tmp_path):
    """fastp_ref's own Evaluator (single-end, -w 1, -p, its compiled-in list) on a soft-masked file == detect_adapter_in_file
    and overrep_in_file on the emulator (run here, where the reference's sources are: no GPU test).  The report prints the Evaluator's seeds with STATS' counts, the ones over Stats'
    own thresholds only, and a seed's count there depends on which other seeds there are (a hit skips the positions behind
    it): so the keys and counts the report prints are held against Stats' loop run over overrep_in_file's seed set
    (evalport_text.stats_overrep_report) - a seed too many or too few moves them."""
    if not (os.path.exists(REF) and os.path.exists(REF_LIST)):
        pytest.skip("no reference binary / source tree here")
    with open(REF_LIST, "rb") as f:
        known = sorted(set(re.findall(rb'knownAdapters\["([ACGT]+)"\]', f.read())))
    assert len(known) > 200
    fq, _ = _e2e_want(variant)
    path = tmp_path / "in.fq"
    path.write_bytes(fq)
    js = tmp_path / "ref.json"
    run = subprocess.run([REF, "-i", str(path), "-o", str(tmp_path / "out.fq"), "-j", str(js), "-h", str(tmp_path / "ref.html"), "-w", "1", "-p", "-P", "1"],
                         capture_output=True)
    lib = engines.build_sim()
    got = evaluator.detect_adapter_in_file(str(path), known, lib_path=lib)
    if variant == "custom_lower":
        # the reference detects the adapter with its lower-case letters, prints it, and then refuses to go on with it
        # (options.cpp:375-381) - there is no report; what it detected is the line behind the announcement
        err = run.stderr.split(b"\n")
        assert run.returncode != 0 and b"can only have bases in {A, T, C, G}" in run.stderr
        assert got != got.upper() and got == err[err.index(b"Detecting adapter sequence for read1...") + 1]
        return
    assert run.returncode == 0, run.stderr[-500:]
    rep = json.loads(js.read_text())
    ref = rep.get("adapter_cutting", {}).get("read1_adapter_sequence", "unspecified").encode()
    assert (got or b"unspecified") == ref and got != b""
    printed = {k.encode(): v for k, v in rep["read1_before_filtering"]["overrepresented_sequences"].items()}
    seeds = evaluator.overrep_in_file(str(path), 76, lib_path=lib)
    reads = fq.split(b"\n")[1::4]
    assert printed == xport.stats_overrep_report(reads, seeds, 76) and set(printed) <= set(seeds)
    # (TruSeq behind random inserts: a hundred overlapping seeds share the reads and none reaches Stats' thresholds)
    assert (len(printed) > 0) == (variant != "listed")
    assert variant == "listed" or any(k != k.upper() for k in seeds)       # seeds that carry the mask
