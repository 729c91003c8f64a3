"""The Evaluator pre-pass's known-adapter check and seed extension on the device (fastp_gpu_eval_known_adapters,
fastp_gpu_eval_adapter_seed; csrc/fq_eval.h) and fastp_amd/evaluator.py against tests/evalport_adapter.py, the literal
restatement of the reference's loops.  Every family runs on the emulator (test_sim_*) and, with the same cases at the
same sizes, on the GPU (test_gpu_*).  All comparisons are exact.  Every case first shows, on the port's output alone,
that it does what it was built for.

One check the reference's rule has cannot be reached through reads: the second arm of the final decision asks for
mismatches[best] < checkedReads, and a hit adds at most alen / 16 <= 16 mismatches while that arm is only looked at when
count <= checkedReads / 50 - so mismatches <= 16 * count < checkedReads always.  The decision cases cover both sides
of `count > checked / 50` and of `count > checked / 200`."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import engines
import evalport
import evalport_adapter as port
import synth
from fastp_amd import abi, evaluator, hostloop

TRUSEQ = [synth.ADAPTER_R1, synth.ADAPTER_R2]
_PORT_CACHE: dict = {}


def _rnd(rng, n) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def _mutate(s: bytes, at) -> bytes:
    out = bytearray(s)
    for i in at:
        out[i] = b"ACGT"[(b"ACGT".index(out[i]) + 1) % 4]
    return bytes(out)


def _fastq(reads) -> bytes:
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


class _Rows:
    """reads -> FASTQ text -> fastp_gpu_parse_fastq -> packed rows in `mem`, beside the same batch decoded on the host"""

    def __init__(self, g, mem, reads, max_len):
        fq = _fastq(reads)
        self.ss, self.qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
        cap = len(reads) + 2
        t = mem.upload(fq, (-len(fq)) % 16 + 16)
        self.seq, self.qual = mem.alloc(cap * self.ss), mem.alloc(cap * self.qs)
        self.lens, loff, llen = mem.alloc(cap * 2), mem.alloc(cap * 16), mem.alloc(cap * 16)
        mem.sync()
        info = g.parse_fastq(mem.ptr(t), len(fq), True, cap, mem.ptr(self.seq), mem.ptr(self.qual), mem.ptr(self.lens),
                             mem.ptr(loff), mem.ptr(llen))
        assert info.first_bad == -1 and info.n_records == len(reads)
        self.mem, self.n = mem, len(reads)
        self.b = hostloop.parse_fastq(fq, self.qs)

    def ptrs(self, first=0):
        m = self.mem
        return m.ptr(self.seq) + first * self.ss, m.ptr(self.qual) + first * self.qs, m.ptr(self.lens) + first * 2


class _Engines:
    """one engine per max_len for a family of cases"""

    def __init__(self, mk):
        self.mk, self.by_len = mk, {}

    def get(self, max_len):
        if max_len not in self.by_len:
            self.by_len[max_len] = self.mk(abi.default_params(False, max_len))
        return self.by_len[max_len]

    def close(self):
        for g in self.by_len.values():
            g.close()


def _mem(mk):
    import format_util
    return format_util.NumpyMem() if mk is engines.sim_engine else format_util.TorchMem()


def _known_equal(g, rows, adapters, key=None, per_read=False):
    """the whole batch through fastp_gpu_eval_known_adapters == the port; per_read: also each read alone (n = 1: the
    replay cannot prune, so counts / mismatches are the match kernel's result for every (read, adapter))"""
    want = _PORT_CACHE.get(key) if key else None
    if want is None:
        want = port.check_known_adapters(rows.b, adapters)
        if key:
            _PORT_CACHE[key] = want
    wc, wm, wchecked, wbest = want
    rc, counts, mism, checked, best = g.eval_known_adapters(*rows.ptrs(), rows.n, adapters)
    assert rc == 0
    assert [int(x) for x in counts] == [wc[a] for a in adapters]
    assert [int(x) for x in mism] == [wm[a] for a in adapters]
    assert checked == wchecked
    assert (adapters[best] if best >= 0 else b"") == wbest
    if per_read:
        anp = [np.frombuffer(a, dtype=np.uint8) for a in adapters]
        for i in range(rows.n):
            rr = rows.b.seq[i, :int(rows.b.lens[i])]
            exp = [port._first_match_np(rr, a) if len(a) < len(rr) else None for a in anp]
            rc, counts, mism, checked, best = g.eval_known_adapters(*rows.ptrs(i), 1, adapters)
            assert rc == 0 and checked == 1
            assert [int(x) for x in counts] == [0 if e is None else 1 for e in exp], i
            assert [int(x) for x in mism] == [0 if e is None else e[1] for e in exp], i
    return want


def test_port_position_scan_equals_literal_loop():
    """evalport_adapter._first_match_np (all positions at once) == first_match (the loop as the reference writes it)"""
    rng = np.random.default_rng(7)
    seen, pairs = set(), []
    for _ in range(400):
        rlen, alen = int(rng.integers(0, 60)), int(rng.integers(1, 40))
        a = _rnd(rng, alen)
        r = bytearray(_rnd(rng, rlen))
        if rlen > alen and rng.random() < 0.7:
            at = int(rng.integers(0, max(1, rlen - 4)))
            ins = _mutate(a, rng.integers(0, alen, size=int(rng.integers(0, 3))))
            r[at:at + alen] = ins[:rlen - at]
            r = r[:rlen]
        if rlen and rng.random() < 0.2:
            r[int(rng.integers(0, rlen))] = ord("N")
        got = port._first_match_np(np.frombuffer(bytes(r), dtype=np.uint8), np.frombuffer(a, dtype=np.uint8))
        assert got == port.first_match(bytes(r), a)
        seen.add(got is None)
        pairs.append((bytes(r), a))
    assert seen == {True, False}
    # ... and match_table (reads of one length at once), which check_known_adapters looks its matches up in
    b = hostloop.parse_fastq(_fastq([r for r, _ in pairs]), 64)
    ads = sorted({a for _, a in pairs[:12]})
    table = port.match_table(b, ads)
    for i, (r, _) in enumerate(pairs):
        for a in ads:
            want = port.first_match(r, a)
            assert (int(table[a][0][i]), int(table[a][1][i])) == (want if want is not None else (-1, 0))


# ---- a. match geometry ------------------------------------------------------------------------------------------
def _geometry_cases():
    """[(name, reads, adapters, max_len)]; the built-for assertions run here, on evalport_adapter.first_match"""
    rng = np.random.default_rng(101)
    fm = port.first_match
    out = []
    # reads of 0, 8, 9 and 10 bases: 9 is the first length with a position
    a5 = b"GATTC"
    reads = [b"", a5 + b"ACG", a5 + b"ACGT", b"C" + a5 + b"ACGT", b"CA" + a5 + b"ACG", b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"]
    assert [len(r) for r in reads[:5]] == [0, 8, 9, 10, 10]
    assert fm(reads[1], a5) is None and fm(reads[2], a5) == (0, 0) and fm(reads[3], a5) == (1, 0) and fm(reads[4], a5) is None
    assert fm(reads[5], b"A") is None and fm(reads[5], a5) is None          # an all-N read
    out.append(("short_reads", reads, [a5, b"A", b"ACGTTGCA"], 64))
    # rlen == alen (no result) and alen + 1
    a20 = _rnd(rng, 20)
    reads = [a20, a20 + b"C", b"G" + a20]
    assert fm(reads[0], a20) is None and fm(reads[1], a20) == (0, 0) and fm(reads[2], a20) == (1, 0)
    out.append(("rlen_alen", reads, [a20], 64))
    # adapter lengths at word edges and at steps of cmplen / 16: contained whole with 0, exactly L / 16 and L / 16 + 1 mismatches
    ads, reads = [], []
    for L in (1, 15, 16, 17, 19, 31, 32, 33, 63, 64, 65, 119, 256):
        a = _rnd(rng, L) if L > 1 else b"G"
        ads.append(a)
        pre, post = (_rnd(rng, 30), _rnd(rng, 10)) if L > 1 else (b"ACTACTTACA" * 3, b"ACTACTTACA")
        allow = L // 16
        r0 = pre + a + post
        assert fm(r0, a) == (30, 0)
        reads.append(r0)
        if L > 1:
            at = [int(x) for x in rng.choice(L, size=allow + 1, replace=False)]
            r1, r2 = pre + _mutate(a, at[:allow]) + post, pre + _mutate(a, at) + post
            assert fm(r1, a) == (30, allow)
            m2 = fm(r2, a)
            assert m2 is None or m2[0] != 30
            reads += [r1, r2]
    out.append(("adapter_lengths", reads, ads[::-1], 512))    # (given in another order than the map's)
    # pos 0, pos rlen - 9 with cmplen 9, every tail overlap from 9 up; reads of up to 512 bases
    t = synth.ADAPTER_R1
    reads = [t + _rnd(rng, 20)]
    assert fm(reads[0], t) == (0, 0)
    for k in range(9, len(t)):
        r = _rnd(rng, 60 - k) + t[:k]
        assert fm(r, t) == (60 - k, 0)
        reads.append(r)
    r = _rnd(rng, 60 - 8) + t[:8]
    assert fm(r, t) is None                                  # an overlap of 8 has no position
    reads.append(r)
    for L in (511, 512):
        r = _rnd(rng, L - 9) + t[:9]
        assert fm(r, t) == (L - 9, 0)
        reads.append(r)
        r = _rnd(rng, L - 40) + _mutate(t, [3, 17]) + _rnd(rng, 40 - len(t))
        assert fm(r, t) == (L - 40, 2)
        reads.append(r)
    out.append(("tails_and_long_reads", reads, [synth.ADAPTER_R2, t], 512))
    # two fitting positions, the second with fewer mismatches: the first wins, with its own count
    a32 = _rnd(rng, 32)
    r = _rnd(rng, 12) + _mutate(a32, [4, 20]) + _rnd(rng, 7) + a32 + _rnd(rng, 9)
    assert fm(r, a32) == (12, 2)
    reads = [r]
    # an N inside the otherwise first window moves the match to the later one
    a15 = _rnd(rng, 15)
    n15 = bytearray(a15)
    n15[5] = ord("N")
    r = _rnd(rng, 11) + bytes(n15) + _rnd(rng, 6) + a15 + _rnd(rng, 10)
    assert fm(r, a15) == (11 + 15 + 6, 0) and fm(r.replace(b"N", a15[5:6]), a15) == (11, 0)
    reads.append(r)
    # first match in the second and in the third tile of 64 positions; a match in tile 1 that fits again in tile 2
    for at in (64, 70, 127, 128, 150):
        r = _rnd(rng, at) + a32 + _rnd(rng, 30)
        assert fm(r, a32) == (at, 0)
        reads.append(r)
    r = _rnd(rng, 10) + _mutate(a32, [9]) + _rnd(rng, 38) + a32 + _rnd(rng, 20)
    assert fm(r, a32) == (10, 1) and fm(r[64:], a32) == (80 - 64, 0)
    reads.append(r)
    out.append(("order_n_tiles", reads, [a15, a32], 256))
    # 1, 32, 33, 64, 65, 234, 256 and 257 adapters of 19..119 bases, shuffled; a few reads carry some of them
    pool = []
    while len(pool) < 257:
        a = _rnd(rng, int(rng.integers(19, 120)))
        if a not in pool:
            pool.append(a)
    for na in (1, 32, 33, 64, 65, 234, 256, 257):
        ads = pool[:na]
        reads = []
        for k in range(10):
            a = ads[int(rng.integers(0, na))] if k < 8 else ads[na - 1]    # (the last one: the last bit of the last word)
            at = int(rng.integers(0, 60))
            reads.append((_rnd(rng, at) + a + _rnd(rng, 130))[:130])
        reads.append(_rnd(rng, 130))
        assert fm(reads[9], ads[na - 1]) is not None
        out.append((f"adapters_{na}", reads, ads, 150))
    return out


def _run_geometry(mk):
    eng, mem = _Engines(mk), _mem(mk)
    unsorted = False
    try:
        for name, reads, adapters, max_len in _geometry_cases():
            g = eng.get(max_len)
            rows = _Rows(g, mem, reads, max_len)
            unsorted |= adapters != sorted(adapters)
            _known_equal(g, rows, adapters, per_read=True)
        assert unsorted          # lists in another order than the map's: every result above is indexed as the caller's list
    finally:
        eng.close()


def test_sim_known_adapters_match_geometry():
    _run_geometry(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_known_adapters_match_geometry")
def test_gpu_known_adapters_match_geometry():
    _run_geometry(engines.gpu_engine)


# ---- b. replay rules --------------------------------------------------------------------------------------------
X12, Y12 = b"ACCGTTAGCATG", b"TGGATCCTAGCA"          # X before Y in map order; 12 bases: no mismatch allowed
FILL = b"CTCTTCTCCTTCTCTCCT"                          # holds neither, nor a tail of 9 of either


def _carry(*ads) -> bytes:
    r = FILL[:6]
    for a in ads:
        r += a + FILL[:5]
    return r + FILL[:4]


def _replay_cases():
    """[(name, reads, adapters, cache key or None, check(port result, trace))]"""
    fm = port.first_match
    rx, ry, rxy, r0 = _carry(X12), _carry(Y12), _carry(X12, Y12), _carry() + FILL
    assert fm(rx, X12) and not fm(rx, Y12) and fm(ry, Y12) and not fm(ry, X12) and fm(rxy, X12) and fm(rxy, Y12)
    assert not fm(r0, X12) and not fm(r0, Y12)
    out = []

    def last_is(what):
        def check(res, trace, n):
            assert [t for t in trace if t[0] == n - 1 and t[1] == Y12] == [(n - 1, Y12, what)]
        return check
    # curMaxCount 20 -> 21: `curMaxCount > 20`
    out.append(("prune_at_20", [rx] * 20 + [ry], last_is("count")))
    out.append(("prune_at_21", [rx] * 21 + [ry], last_is("pruned")))
    # count[Y] = 2 against curMaxCount / 10 at 29, 30, 31
    out.append(("tenth_at_29", [ry] * 2 + [rx] * 29 + [ry], last_is("count")))
    out.append(("tenth_at_30", [ry] * 2 + [rx] * 30 + [ry], last_is("pruned")))
    out.append(("tenth_at_31", [ry] * 2 + [rx] * 31 + [ry], last_is("pruned")))
    # X (earlier in map order) takes curMaxCount to 21 inside the last read and prunes Y of the same read ...
    out.append(("prune_inside_read", [ry] + [rx] * 20 + [rxy], last_is("pruned")))

    # ... and with the roles swapped the later one cannot prune the earlier one
    def control(res, trace, n):
        assert [t for t in trace if t[0] == n - 1] == [(n - 1, X12, "count"), (n - 1, Y12, "count")] and res[0][Y12] == 21
    out.append(("prune_inside_read_control", [rx] + [ry] * 20 + [rxy], control))

    # the exit at curMaxCount > 1000
    def exit_1000(res, trace, n):
        assert res[2] == 1002 and res[0][X12] == 1001 and res[3] == X12
    out.append(("exit_after_1000_hits", [rx] * 1100, exit_1000))
    # the final decision: count against checked / 50 and checked / 200 (1000 reads: 20 and 5)
    for hits, accepted in ((21, True), (20, True), (6, True), (5, False)):
        def decision(res, trace, n, hits=hits, accepted=accepted):
            assert res[2] == 1000 and res[0][X12] == hits and res[3] == (X12 if accepted else b"")
        out.append((f"decision_{hits}_of_1000", ([rx] + [r0] * 9) * hits + [r0] * (1000 - 10 * hits), decision))

    # a tie on the largest count: the first in map order
    def tie(res, trace, n):
        assert res[0][X12] == res[0][Y12] == 7 and res[3] == X12
    out.append(("tie", [ry, rx, r0] * 7 + [r0] * 79, tie))
    return out


def _read_limit_case():
    """100,001 reads of 12 bases, two adapters of 10: the loop leaves AT read 100,000 - counted, not looked at"""
    rng = np.random.default_rng(5)
    xa, ya = b"ACCGTTAGCA", b"TGGATCCTAG"
    codes = rng.integers(0, 4, size=(100001, 12))
    arr = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    arr[::200, :10] = np.frombuffer(xa, dtype=np.uint8)
    arr[100000, :10] = np.frombuffer(xa, dtype=np.uint8)
    return [bytes(r) for r in arr], [ya, xa]


def _run_replay(mk):
    eng, mem = _Engines(mk), _mem(mk)
    try:
        g = eng.get(64)
        ads = [Y12, X12]
        for name, reads, check in _replay_cases():
            rows = _Rows(g, mem, reads, 64)
            trace = []
            res = port.check_known_adapters(rows.b, ads, trace)
            check(res, trace, len(reads))
            _PORT_CACHE[("replay", name)] = res
            _known_equal(g, rows, ads, key=("replay", name))
        reads, ads = _read_limit_case()
        rows = _Rows(g, mem, reads, 64)
        res = _known_equal(g, rows, ads, key=("replay", "read_limit"))
        assert res[2] == 100001 and port.first_match(reads[100000], ads[1]) == (0, 0)
        head = hostloop.FastqBatch(rows.b.names[:100000], None, rows.b.seq[:100000], None, rows.b.lens[:100000])
        key = ("replay", "read_limit_head")
        if key not in _PORT_CACHE:
            _PORT_CACHE[key] = port.check_known_adapters(head, ads)
        assert _PORT_CACHE[key][0] == res[0] and 500 <= res[0][ads[1]] < 1000     # the last read's match is not in it
    finally:
        eng.close()


def test_sim_known_adapters_replay_rules():
    _run_replay(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_known_adapters_replay_rules")
def test_gpu_known_adapters_replay_rules():
    _run_replay(engines.gpu_engine)


# ---- c. argument checks -----------------------------------------------------------------------------------------
def _run_argument_checks(mk):
    g, mem = mk(abi.default_params(False, 64)), _mem(mk)
    try:
        rows = _Rows(g, mem, [_carry(X12)] * 3, 64)
        p = rows.ptrs()

        def rc_of(ads, n=3):
            return g.eval_known_adapters(*p, n, ads, check=False)
        assert rc_of([X12])[0] == 0
        assert rc_of([X12, b""])[0] == abi.E_INVALID
        assert rc_of([X12, b"acgt" * 3])[0] == abi.E_INVALID
        assert rc_of([b"ACGTNACGTACG"])[0] == abi.E_INVALID
        assert rc_of([X12, Y12, X12])[0] == abi.E_INVALID
        assert rc_of([b"A" * 256])[0] == 0 and rc_of([b"A" * 257])[0] == abi.E_UNSUPPORTED
        many = []
        for i in range(1025):
            many.append(bytes(b"ACGT"[(i >> (2 * k)) & 3] for k in range(6)) + b"ACGTAC")
        assert len(set(many)) == 1025
        assert rc_of(many[:1024])[0] == 0 and rc_of(many)[0] == abi.E_UNSUPPORTED
        rc, counts, mism, checked, best = rc_of([])
        assert (rc, len(counts), checked, best) == (0, 0, 3, -1)
        rc, counts, mism, checked, best = rc_of([X12], n=0)
        assert (rc, list(counts), checked, best) == (0, [0], 0, -1)
        # NULL pointers, straight at the C ABI
        fn = g.lib.fastp_gpu_eval_known_adapters
        arr = (C.c_char_p * 1)(X12)
        cnt, mis = (C.c_int32 * 1)(), (C.c_int32 * 1)()
        chk, best = C.c_int64(), C.c_int32()
        good = [g.h, p[0], p[1], p[2], 3, arr, 1, C.addressof(cnt), C.addressof(mis), C.byref(chk), C.byref(best)]
        assert fn(*good) == 0 and cnt[0] == 3
        for k in (0, 1, 2, 3, 5, 7, 8, 9, 10):
            bad = list(good)
            bad[k] = None
            assert fn(*bad) == abi.E_INVALID, k
        assert g.eval_adapter_seed(*p, 3, 0, 1 << 20, check=False)[0] == abi.E_INVALID
        fs = g.lib.fastp_gpu_eval_adapter_seed
        buf = [C.create_string_buffer(512) for _ in range(2)]
        i32 = [C.c_int32() for _ in range(3)]
        i64 = C.c_int64()
        good = [g.h, p[0], p[1], p[2], 3, 0, 5, buf[0], C.byref(i32[0]), buf[1], C.byref(i32[1]), C.byref(i32[2]), C.byref(i64)]
        assert fs(*good) == 0
        for k in (0, 1, 2, 3, 7, 8, 9, 10, 11, 12):
            bad = list(good)
            bad[k] = None
            assert fs(*bad) == abi.E_INVALID, k
    finally:
        g.close()


def test_sim_eval_adapter_argument_checks():
    _run_argument_checks(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_eval_adapter_argument_checks")
def test_gpu_eval_adapter_argument_checks():
    _run_argument_checks(engines.gpu_engine)


# ---- d. seed hits and walks -------------------------------------------------------------------------------------
SEED = b"ACGTTGCAAG"


def _seed_cases():
    """[(name, reads, max_len, trim_tail1, seed key, check(fwd, bwd, leaf, hits))] - check runs on the port's result"""
    rng = np.random.default_rng(31)
    key = port.seq2int(SEED, 0)
    assert port.int2seq(key) == SEED
    left, ext = _rnd(rng, 25), _rnd(rng, 30)
    while SEED[:4] in left + ext:
        left, ext = _rnd(rng, 25), _rnd(rng, 30)
    base = left + SEED + ext + b"T"          # forward sequence with trim_tail1 0: ext
    noise = [_rnd(rng, 66) for _ in range(30)]
    out = []

    def other(b):
        return b"ACGT"[(b"ACGT".index(b) + 2) % 4:][:1]
    for h in (49, 50, 51):
        def check(f, bw, leaf, hits, h=h):
            assert hits == h and leaf and (f, bw) == ((ext, left[::-1]) if h >= 50 else (b"", b""))   # (backward: to the read's start)
        out.append((f"hits_{h}", [base] * h + noise, 80, 0, key, check))
    # trim_tail1 3: three bases fewer at the far end
    out.append(("trim_tail_3", [base] * 60 + noise, 80, 3, key, lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (ext[:-2], left[::-1], True, 60) or pytest.fail("trim_tail1 3")))
    # 95 of 100 go on, 94 of 100 and (the third case) 57 of 60
    alt = base[:40] + other(base[40:41]) + base[41:]
    out.append(("ratio_95_of_100", [base] * 95 + [alt] * 5 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, leaf, hits) == (ext, True, 100) or pytest.fail("95 of 100 must go on")))
    out.append(("ratio_94_of_100", [base] * 94 + [alt] * 6 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (ext[:5], left[::-1], False, 100) or pytest.fail("94 of 100 must stop")))
    out.append(("ratio_57_of_60", [base] * 57 + [alt] * 3 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, leaf, hits) == (ext, True, 60) or pytest.fail("57 of 60 must go on")))
    # hits at pos 20 and at rlen - 10 - shiftTail (an empty forward sequence), the latter with both trims
    at20 = left[:20] + SEED + ext + b"T"
    out.append(("pos_20_and_19", [at20] * 55 + [left[:19] + SEED + ext + b"T"] * 55 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (ext, left[:20][::-1], True, 55) or pytest.fail("pos 19 is not searched")))
    for trim in (0, 3):
        st = max(1, trim)
        lastpos = left + ext + SEED + b"T" * st
        tooclose = left + ext + b"A" + SEED + b"T" * (st - 1)
        assert len(lastpos) - 10 - st == 55

        def check(f, bw, leaf, hits):
            assert hits == 60 and f == b"" and bw == (left + ext)[::-1] and leaf
        out.append((f"last_pos_trim{trim}", [lastpos] * 60 + [tooclose] * 60 + noise, 80, trim, key, check))
    # a read with two hits
    two = left + SEED + ext[:12] + SEED + ext + b"T"
    out.append(("two_hits", [two] * 30 + noise, 120, 0, key,
                lambda f, bw, leaf, hits: hits == 60 and f[:12] == ext[:12] or pytest.fail("two hits per read")))
    # N at extension depth 0 / deeper: those sequences end there
    n0 = base[:35] + b"N" + base[36:]
    n3 = base[:38] + b"N" + base[39:]
    out.append(("n_in_extension", [base] * 50 + [n0] * 20 + [n3] * 20 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, leaf, hits) == (ext, True, 90) or pytest.fail("N ends a sequence")))
    out.append(("n_cuts_below_50", [base] * 40 + [n3] * 20 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, leaf, hits) == (ext[:3], True, 60) or pytest.fail("N at depth 3")))
    # a seed that never occurs; a seed window with an N
    nseed = base[:28] + b"N" + base[29:]
    out.append(("absent_and_n_in_seed", [nseed] * 70 + noise, 80, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (b"", b"", True, 0) or pytest.fail("no hit")))
    # 512 bases: pos 499 is searched, pos 500 is not
    l499, l500 = _rnd(rng, 499), _rnd(rng, 500)
    while SEED[:5] in l499 + l500:
        l499, l500 = _rnd(rng, 499), _rnd(rng, 500)
    out.append(("pos_499_500", [l499 + SEED + b"CAT", l500 + SEED + b"CA"] * 55, 512, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (b"CA", l499[::-1], True, 55) or pytest.fail("MAX_SEARCH_LENGTH")))
    # more hits than one workgroup has lanes
    out.append(("hits_3000", [base] * 2850 + [alt] * 150, 80, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (ext, left[::-1], True, 3000) or pytest.fail("3000 hits")))
    # reached_leaf cleared by the backward walk only
    bsplit = left[:24] + other(left[24:25]) + SEED + ext + b"T"
    out.append(("leaf_cleared_backward", [base] * 40 + [bsplit] * 40, 80, 0, key,
                lambda f, bw, leaf, hits: (f, bw, leaf, hits) == (ext, b"", False, 80) or pytest.fail("backward walk")))
    return out


def _run_seed(mk):
    eng, mem = _Engines(mk), _mem(mk)
    try:
        for name, reads, max_len, trim, key, check in _seed_cases():
            g = eng.get(max_len)
            rows = _Rows(g, mem, reads, max_len)
            ck = ("seed", name)
            if ck not in _PORT_CACHE:
                _PORT_CACHE[ck] = port.seed_paths(rows.b, key, trim)
            want = _PORT_CACHE[ck]
            check(*want)
            rc, fwd, bwd, leaf, hits = g.eval_adapter_seed(*rows.ptrs(), rows.n, trim, key)
            assert (fwd, bwd, leaf, hits) == want, name
            if name == "absent_and_n_in_seed":
                rc, fwd, bwd, leaf, hits = g.eval_adapter_seed(*rows.ptrs(), rows.n, trim, port.seq2int(b"GGGGGGGGGG", 0))
                assert (fwd, bwd, leaf, hits) == (b"", b"", True, 0) == port.seed_paths(rows.b, (1 << 20) - 1, trim)
    finally:
        eng.close()


def test_sim_adapter_seed_hits_and_walks():
    _run_seed(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_adapter_seed_hits_and_walks")
def test_gpu_adapter_seed_hits_and_walks():
    _run_seed(engines.gpu_engine)


# ---- e. detect_adapter end to end -------------------------------------------------------------------------------
CUSTOM = b"CTGACCTAGTCAAGGTCCATGCTAGGATCCATGCAAT"      # on nobody's list (tests/test_ref_binding.py uses it the same way)
LISTED = TRUSEQ + [b"GATCGTCGGACTGTAGAACTCTGAACGTGTAGA", b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGGGTGCCAAGG"]


def _e2e_reads(variant):
    kw = dict(L=76, seed=61, paired=False, dup_frac=0.0)
    if variant == "listed":
        return synth.synth_pairs(11000, insert_mean=50.0, insert_sd=12.0, **kw)
    if variant == "few":
        return synth.synth_pairs(9000, insert_mean=50.0, insert_sd=12.0, **kw)
    if variant == "none":
        return synth.synth_pairs(11000, insert_mean=300.0, insert_sd=20.0, insert_min=150, **kw)
    # "custom": an adapter on nobody's list behind an amplicon.  The k-mer path only answers where the bases in front of
    # the adapter agree too (a walk that meets a split clears reachedLeaf, evaluator.cpp:532-537): inserts are the last
    # 30..44 bases of one 44-base sequence, so the backward walk runs on until the longest inserts thin out below 50
    rng = np.random.default_rng(62)
    n, L = 11000, 76
    amp = np.frombuffer(_rnd(rng, 44), dtype=np.uint8)
    tail = np.concatenate([np.frombuffer(CUSTOM, dtype=np.uint8), np.full(L, ord("A"), dtype=np.uint8)])
    seq = np.zeros((n, 80), dtype=np.uint8)
    for i, ins in enumerate(rng.integers(30, 45, size=n)):
        seq[i, :L] = np.concatenate([amp[44 - ins:], tail])[:L]
    err = rng.random((n, L)) < 0.01
    seq[:, :L] = np.where(err, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))], seq[:, :L])
    qual = np.zeros((n, 80), dtype=np.uint8)
    qual[:, :L] = ord("I")
    return {"seq1": seq, "qual1": qual, "len1": np.full(n, L, dtype=np.int32)}


def _e2e_fastq(variant) -> bytes:
    d = _e2e_reads(variant)
    return synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1)


def _e2e_want(variant, fq):
    key = ("e2e", variant)
    if key not in _PORT_CACHE:
        b = hostloop.parse_fastq(fq, abi.qual_stride(76))
        counts, _ = evalport.adapter_kmer_counts(b, 0)
        _PORT_CACHE[key] = port.eval_adapter(b, LISTED, counts, 0)
    return _PORT_CACHE[key]


def _check_e2e_want(variant, want):
    if variant == "listed":
        assert want == synth.ADAPTER_R1
    elif variant == "custom":
        assert len(want) == 60 and want not in LISTED and want.endswith(CUSTOM[:16])    # the longest insert, 44, and the cut at 60
    else:
        assert want == b""


def _run_e2e(mk):
    g, mem = mk(abi.default_params(False, 76)), _mem(mk)
    try:
        for variant in ("listed", "custom", "none", "few"):
            fq = _e2e_fastq(variant)
            want = _e2e_want(variant, fq)
            _check_e2e_want(variant, want)
            n = fq.count(b"\n") // 4
            ss, qs = abi.seq_stride(76), abi.qual_stride(76)
            t = mem.upload(fq, (-len(fq)) % 16 + 16)
            seq, qual, lens = mem.alloc((n + 2) * ss), mem.alloc((n + 2) * qs), mem.alloc((n + 2) * 2)
            loff, llen = mem.alloc((n + 2) * 16), mem.alloc((n + 2) * 16)
            mem.sync()
            info = g.parse_fastq(mem.ptr(t), len(fq), True, n + 2, mem.ptr(seq), mem.ptr(qual), mem.ptr(lens), mem.ptr(loff), mem.ptr(llen))
            assert info.n_records == n
            got = evaluator.detect_adapter(g, mem.ptr(seq), mem.ptr(qual), mem.ptr(lens), n, LISTED[::-1], 0)
            assert got == want, variant
    finally:
        g.close()


def test_sim_detect_adapter_end_to_end():
    _run_e2e(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_detect_adapter_end_to_end")
def test_gpu_detect_adapter_end_to_end():
    _run_e2e(engines.gpu_engine)


def test_top_seeds_equal_the_insertion_loop():
    """evaluator.top_seeds == the literal loop of evaluator.cpp:399-443 on hand-made histograms: ties, ineligible bins
    holding the largest counts, fewer than ten non-zero bins, an empty histogram"""
    rng = np.random.default_rng(9)
    elig = [k for k in rng.integers(1, 1 << 20, size=4000) if port.eligible_key(int(k))]
    inel = [k for k in rng.integers(1, 1 << 20, size=4000) if not port.eligible_key(int(k))]
    assert len(elig) > 100 and len(inel) > 100
    hists = []
    c = np.zeros(1 << 20, dtype=np.uint32)
    hists.append(c.copy())                                   # nothing
    c[elig[:4]] = [50, 50, 7, 50]
    hists.append(c.copy())                                   # fewer than ten, a tie of three
    c[elig[4:40]] = rng.integers(1, 6, size=36) * 100        # many ties
    c[inel[:30]] = 100000                                    # low-complexity / GC-rich / GGGG bins on top
    c[0] = 0
    hists.append(c.copy())
    c[elig[40:60]] = 300
    hists.append(c.copy())                                   # the tie runs across the tenth place
    for i, h in enumerate(hists):
        # (the loop over all 2^20 bins for two of them; for the others over the bins that hold something and a thousand that do not)
        visit = None if i in (1, 2) else sorted(set(np.flatnonzero(h).tolist()) | set(int(k) for k in elig[-1000:]))
        want_keys, want_total = port.top_keys(h, visit)
        got_keys, got_total = evaluator.top_seeds(h)
        assert got_total == want_total
        nz = [k for k in want_keys if h[k] > 0]
        assert got_keys[:len(nz)] == nz                      # (zero bins end the caller's loop: count < 10)
        assert all(h[k] == 0 for k in got_keys[len(nz):])
    assert evaluator.int2seq(port.seq2int(SEED, 0)) == SEED == port.int2seq(port.seq2int(SEED, 0))
    assert evaluator.match_known_adapter(CUSTOM, LISTED) == b"" == port.match_known_adapter(CUSTOM, LISTED)
    seq = synth.ADAPTER_R1 + b"ACGT"
    assert evaluator.match_known_adapter(seq, LISTED[::-1]) == synth.ADAPTER_R1 == port.match_known_adapter(seq, LISTED)


def test_load_adapter_list(tmp_path):
    p = tmp_path / "a.txt"
    p.write_bytes(b"# known\nACGTAC\n\nacgtac\nTTGACA\n")
    assert evaluator.load_adapter_list(str(p)) == [b"ACGTAC", b"TTGACA"]
    p = tmp_path / "a.fa"
    p.write_bytes(b">one\nACGT\nAC\n>two\nTTGACA\n>one again\nACGTAC\n")
    assert evaluator.load_adapter_list(str(p)) == [b"ACGTAC", b"TTGACA"]


def test_sim_detect_adapter_in_file(tmp_path):
    """a plain and a gzip-compressed file through detect_adapter_in_file on the emulator"""
    import gzip
    fq = _e2e_fastq("listed")
    want = _e2e_want("listed", fq)
    _check_e2e_want("listed", want)
    plain, gz = tmp_path / "in.fq", tmp_path / "in.fq.gz"
    plain.write_bytes(fq)
    gz.write_bytes(gzip.compress(fq, 1))
    lib = engines.build_sim()
    assert evaluator.detect_adapter_in_file(str(plain), LISTED, lib_path=lib) == want
    assert evaluator.detect_adapter_in_file(str(gz), LISTED, lib_path=lib) == want


# ---- f. the reference itself ------------------------------------------------------------------------------------
REF = os.path.join(engines.ROOT, "oracle", "_ref", "fastp_ref")
REF_LIST = "/root/reference/src/knownadapters.h"


@pytest.mark.parametrize("variant", ["listed", "custom", "none"])
def test_detect_adapter_in_file_equals_reference(variant, tmp_path):
    """fastp_ref's own auto-detection (single-end, its compiled-in list) == detect_adapter_in_file on the emulator with the
    list read from the reference's header at test time"""
    if not (os.path.exists(REF) and os.path.exists(REF_LIST)):
        pytest.skip("no reference binary / source tree here")
    with open(REF_LIST, "rb") as f:
        known = sorted(set(re.findall(rb'knownAdapters\["([ACGT]+)"\]', f.read())))
    assert len(known) > 200
    fq = _e2e_fastq(variant)
    path = tmp_path / "in.fq"
    path.write_bytes(fq)
    js = tmp_path / "ref.json"
    subprocess.run([REF, "-i", str(path), "-o", str(tmp_path / "out.fq"), "-j", str(js), "-h", str(tmp_path / "ref.html"), "-w", "1"],
                   check=True, capture_output=True)
    # (without an adapter the report has no "adapter_cutting" section: adapter trimming is off for the run)
    ref = json.loads(js.read_text()).get("adapter_cutting", {}).get("read1_adapter_sequence", "unspecified").encode()
    got = evaluator.detect_adapter_in_file(str(path), known, lib_path=engines.build_sim())
    assert (got or b"unspecified") == ref
    assert (variant == "none") == (got == b"")
