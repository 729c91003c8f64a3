"""Hand-built units for the text kernel (fastp_amd/csrc/fq_text.h) and the lane / tile kernels beside it: every family puts
the events of one step of the worker loop on the scan steps 63 / 64 / 65 (127 / 128 / 129 where the read is long enough) - the last
step of a block of 64 lanes, the first of the next one, and one further - or makes a value survive from an earlier block.

A family is (params, reads, expectations).  Every unit states the outcome it was built for (`Units.add(..., len1=..)`), and
`reached()` - plain Python over the records an engine returned - says which units missed theirs.  tests/test_text_edges.py
asserts that on the oracle's result before it compares any device route: a unit whose edge the reference never reaches tests
nothing, whatever agrees with whatever.

Constructions that cannot reach their edge in the reference, and are therefore NOT built (the reason beside each):
  * trimPolyG breaking by `mismatch > (i + 1) / 8` at step 63 / 64 / 65: from step 47 on (i + 1) / 8 is at least 6, so the
    `mismatch > 5` rule always breaks the walk first (polyx.cpp:27-33); the ratio rule can only fire below step 47.
  * cut_right with NO base under the minimum behind the first failing window: a window whose sum is below w * (33 + q) holds a
    base below 33 + q, and it starts below l - tail - w, so that base lies below l - 1 (filter.cpp:150-160).
  * a one-gap overlap accepted at a POSITIVE offset shows in no record and no counter (the pair record carries the ungapped
    analysis, a positive offset trims nothing, correction skips a gapped overlap): the units use negative offsets.
"""
import numpy as np

from fastp_amd import abi
import cases

RS_NULL, RS_ADAPTER, RS_ADAPTER_OV, RS_CORRECTED, RS_MERGED, RS_POLYX = 0x01, 0x04, 0x08, 0x10, 0x20, 0x40
TEXT_WAVES = 8   # fq_text.h: wavefronts (= units at a time) per workgroup of the text kernel
LENGTHS = (0, 1, 4, 5, 63, 64, 65)   # every family keeps units of these lengths, and of max_len
_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N"}
_OTHER = {"A": "C", "C": "A", "G": "T", "T": "G", "N": "A"}   # a substitution that is never the complement either


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[k] for k in rng.integers(0, len(letters), size=n))


def sub(s, positions):
    s = list(s)
    for p in positions:
        s[p] = _OTHER[s[p]]
    return "".join(s)


class Units:
    """reads as strings + phred lists; what each unit was built for"""

    def __init__(self, L, paired):
        self.L, self.paired = L, paired
        self.rows, self.expect, self.names = [], [], []

    def add(self, name, s1, q1=40, s2=None, q2=40, **expect):
        assert expect, f"{name}: a unit states what it was built for"
        assert len(s1) <= self.L and (s2 is None or len(s2) <= self.L), name
        assert (s2 is not None) == self.paired, name
        q1 = [q1] * len(s1) if np.isscalar(q1) else list(q1)
        q2 = None if s2 is None else ([q2] * len(s2) if np.isscalar(q2) else list(q2))
        assert len(q1) == len(s1) and (s2 is None or len(q2) == len(s2)), name
        self.rows.append((s1, q1, s2, q2))
        self.expect.append(expect)
        self.names.append(name)
        return len(self.rows) - 1

    def arrays(self):
        n, stride = len(self.rows), (self.L + 7) // 8 * 8
        d = {}
        for tag, ks, kq in (("1", 0, 1), ("2", 2, 3)) if self.paired else (("1", 0, 1),):
            seq, qual, lens = np.zeros((n, stride), np.uint8), np.zeros((n, stride), np.uint8), np.zeros(n, np.int32)
            for i, row in enumerate(self.rows):
                s, q = row[ks], row[kq]
                lens[i] = len(s)
                seq[i, :len(s)] = np.frombuffer(s.encode(), np.uint8)
                qual[i, :len(s)] = np.asarray(q, np.uint8) + 33
            d["seq" + tag], d["qual" + tag], d["len" + tag] = seq, qual, lens
        return d


class Family:
    def __init__(self, name, params, units, flags, edge=(60, 69), counters=None, files=None, umi=None):
        self.name, self.params, self.paired, self.L = name, params, units.paired, units.L
        self.flags = [str(x) for x in flags] + ["-l", "1"]   # the reference's command line for the same options (-l 1: length_required)
        self.files, self.umi = files, umi                    # files beside the input (--adapter_fasta); the host's UMI name editing
        self.d, self.expect, self.names = units.arrays(), units.expect, units.names
        self.n = len(units.rows)
        self.edge = edge           # the stretch of read 1 a soft variant rewrites: it crosses the family's edge position
        self.counters = counters   # f(counters, layout) -> list of problems: outcomes that only show in the counter block

    def tiled(self, reps):
        """the same family `reps` times over (only the reads: the copies state no outcome of their own)"""
        import copy
        t = copy.copy(self)
        t.d = {key: np.concatenate([v] * reps) for key, v in self.d.items()}
        t.n = self.n * reps
        return t

    def args(self, d=None):
        d = d or self.d
        return (d["seq1"], d["qual1"], d["len1"]) + ((d["seq2"], d["qual2"], d["len2"]) if self.paired else ())


def reached(fam, res, events=None):
    """the units (name: what was wanted, what came) whose stated outcome the records do not show; [] = every edge was reached"""
    r1, r2, pr, corr = res
    miss = []
    ncorr = np.bincount((corr["read"] // (2 if fam.paired else 1)).astype(np.int64), minlength=fam.n) if len(corr) else np.zeros(fam.n, int)
    for u, (name, exp) in enumerate(zip(fam.names, fam.expect)):
        got = {}
        for key in exp:
            m = key[-1]
            r = r2 if m == "2" else r1
            if key in ("len1", "len2"):
                got[key] = int(r["len"][u])
            elif key in ("front1", "front2"):
                got[key] = int(r["front"][u])
            elif key in ("code1", "code2"):
                got[key] = int(r["code"][u])
            elif key in ("null1", "null2"):
                got[key] = int(bool(r["flags"][u] & RS_NULL))
            elif key in ("apos1", "apos2"):
                got[key] = int(r["adapter_pos"][u]) if r["flags"][u] & (RS_ADAPTER | RS_ADAPTER_OV) else None
            elif key in ("polyx1", "polyx2"):
                got[key] = int(bool(r["flags"][u] & RS_POLYX))
            elif key == "offset":   # None: no overlap
                got[key] = int(pr["ov_offset"][u]) if pr["flags"][u] & 1 else None
            elif key == "ov_len":
                got[key] = int(pr["ov_len"][u])
            elif key == "diff":
                got[key] = int(pr["ov_diff"][u])
            elif key == "ov_trim":   # adapters trimmed by the (possibly one-gap) overlap analysis
                got[key] = int(bool(r1["flags"][u] & RS_ADAPTER_OV))
            elif key == "ncorr":
                got[key] = int(ncorr[u])
            elif key == "merged":   # length of the merged read; None: not merged
                got[key] = int(r1["reserved"][u]) + int(r2["reserved"][u]) if r1["flags"][u] & RS_MERGED else None
            elif key == "exact_end":   # --overlapped_out: end of the exact overlap in read 1; None: the exact analysis found none
                got[key] = int(r1["reserved"][u] & 0x7FFF) if r1["reserved"][u] & 0x8000 else None
            elif key == "events":
                got[key] = int(np.count_nonzero(events["read"] == u)) if events is not None else None
            else:
                raise KeyError(key)
        if got != exp:
            miss.append((u, name, exp, got))
    return miss


def soften(fam, units, how="lower"):
    """the family with a stretch across its edge position rewritten in the given units: lower case, an IUPAC letter or '.'
    (letters outside ACGTN: only those units are listed for the text kernel).  A read shorter than the stretch gets its last
    base rewritten; an empty read 1 makes read 2 (or nothing) carry it."""
    d = {k: v.copy() for k, v in fam.d.items()}
    lo, hi = fam.edge
    for k, u in enumerate(units):
        tag = "1"
        if d["len1"][u] == 0 and fam.paired:
            tag = "2"
        n = int(d["len" + tag][u])
        if n == 0:
            continue
        a, b = (lo, min(hi, n)) if lo < n else (n - 1, n)
        kind = how if how != "mixed" else ("lower", "iupac", "dot")[k % 3]
        if kind == "lower":
            d["seq" + tag][u, a:b] |= 0x20
        elif kind == "iupac":
            d["seq" + tag][u, a:b] = np.frombuffer(b"RYKMSWBDHV", np.uint8)[np.arange(b - a) % 10]
        else:
            d["seq" + tag][u, (a + b) // 2] = ord(".")
    return d


def listed(fam, d):
    """units of d that hold a letter outside ACGTN (what the packer lists for the text kernel)"""
    ok = np.zeros(256, bool)
    ok[[0] + [ord(c) for c in "ACGTN"]] = True
    bad = ~ok[d["seq1"]].all(axis=1)
    if fam.paired:
        bad |= ~ok[d["seq2"]].all(axis=1)
    return np.flatnonzero(bad)


def text_tables_in_lds(params, device_lds=160 * 1024):
    """launch_text's inequality (fastp_gpu.hip): Stats' per-base tables of a workgroup sit in LDS beside the wavefronts' texts
    when both fit min(150 KiB, the device's LDS); otherwise every lane adds to the counter block with global atomics.
    Returns (in LDS?, dynamic LDS bytes of the launch)."""
    ml = (params.max_len + 8 + 7) & ~7
    text = TEXT_WAVES * (9 * ml + 3 * 264)
    slots = 2 if not params.paired else 3 if params.merge else 4
    tables = slots * (34 * abi.cycles_for(params) + 1024 + 128) * 4
    fits = tables + text <= min(150 * 1024, device_lds)
    return fits, text + (tables if fits else 0)


def _se(L, **kw):
    p = abi.default_params(False, L)
    p.adapter_enabled = 0
    p.adapter_seq_r1 = None
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pe(L, **kw):
    p = abi.default_params(True, L)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _length_units(U, rng, expect, letters="ACGT", also=()):
    """the lengths every family keeps; expect(n) -> what a plain read of n bases comes to under the family's options"""
    for n in LENGTHS + tuple(also) + (U.L,):
        s = rand_seq(rng, n, letters)
        if U.paired:
            U.add(f"len{n}", s, 40, rand_seq(rng, n, letters), 40, **expect(n))
        else:
            U.add(f"len{n}", s, 40, **expect(n))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Filter::trimAndCut (filter.cpp:68-207).  Qualities are EXACTLY the threshold (a window of them is "at" it) or below it,
# so where the first window at / below the threshold starts is where the builder puts it, for every window size.
def cut_front(L, w, f=0, t=0, umi=0):
    """-f f -t t, a UMI of `umi` bases in front (front > 0 when the scan starts), --cut_front window w at Q20.  The scan's
    positions count from the read behind the UMI; its blocks start at f."""
    rng = np.random.default_rng(100 + L + w + f)
    p = _se(L, cut_front=1, cut_front_window=w, cut_front_quality=20, trim_front1=f, trim_tail1=t, umi_len1=umi, length_required=1)
    U = Units(L, False)
    l = L - umi
    hi = l - t - w            # the loop tests starts f .. hi - 1

    def unit(name, s, nrun):
        """first window at the threshold starts at s (s = hi: none does); nrun N's from where the cut lands (-1: to the end)"""
        q = [2] * l
        q[s:] = [20] * (l - s)
        if s >= hi:               # no window at the threshold inside the loop: the last tested one still holds a low base
            q = [20] * l
            q[hi - 1 + w - 1] = 2 if hi > f else 20
            q[:max(hi - 1, 0)] = [2] * max(hi - 1, 0)
            s = hi
        land = s + w - 1 if s > 0 else 0
        seq = list(rand_seq(rng, l))
        end = l if nrun < 0 else min(l, land + nrun)
        seq[land:end] = "N" * (end - land)
        front = end
        exp = dict(null1=1) if (l - front - t <= 0 or front >= l - 1) else dict(null1=0, front1=umi + front, len1=l - front - t)
        U.add(name, rand_seq(rng, umi) + "".join(seq), [40] * umi + q, **exp)

    for s in sorted({f, f + 63, f + 64, f + 65, f + 127, f + 128, f + 129, hi - 1, hi}):
        if f <= s <= hi:
            unit(f"s{s}", s, 0)
            unit(f"s{s}_n3", s, 3)
    if f + 64 < hi:
        # the N run behind the cut: first_up(land, l) starts a block of its own where the cut lands; the run ends on its last
        # step, on the first steps of the next block and well inside it, with real bases behind it (the run to the end gives NULL,
        # and so would a scan that gave up after one block)
        for nrun in (63, 64, 65, 70):
            assert (f + w - 1 if f > 0 else 0) + nrun < l - t - 1
            unit(f"s{f}_nrun{nrun}_ends_in_next_block", f, nrun)
        unit("s63_nrun_to_end", f + 63, -1)
        unit("s0_nrun_to_end", f, -1)
    for n in LENGTHS:           # short reads: the window does not fit (NULL) or the whole read is at the threshold
        ln = n - umi
        if ln < 0:   # shorter than its UMI: Read::trimFront leaves one base (none of an empty read), nothing fits behind -f
            U.add(f"len{n}", rand_seq(rng, n), [40] * n, null1=1)
            continue
        exp = dict(null1=1) if ln - f - t - w <= 0 else dict(null1=0, front1=umi + f + (w - 1 if f > 0 else 0), len1=ln - t - f - (w - 1 if f > 0 else 0))
        if exp.get("len1", 1) <= 0 or (not exp["null1"] and exp["front1"] - umi >= ln - 1):
            exp = dict(null1=1)
        U.add(f"len{n}", rand_seq(rng, n), [40] * umi + [20] * ln, **exp)
    flags = ["-G", "-A", "--cut_front", "--cut_front_window_size", w, "--cut_front_mean_quality", 20, "-f", f, "-t", t]
    if umi:
        flags += ["-U", "--umi_loc", "read1", "--umi_len", umi]
    return Family(f"cut_front_L{L}_w{w}_f{f}", p, U, flags, edge=(umi + f + 60, umi + f + 69), umi=("read1", umi) if umi else None)


def cut_right(L, w, f=0, t=0):
    """--cut_right window w at Q20: the first window below the threshold starts at s; the first base under the minimum is the
    low base that failed it, at s + w - 1 (w = 70: a block further on)"""
    rng = np.random.default_rng(200 + L + w + f)
    p = _se(L, cut_right=1, cut_right_window=w, cut_right_quality=20, trim_front1=f, trim_tail1=t, length_required=1)
    U = Units(L, False)
    hi = L - t - w
    for s in sorted({f, f + 63, f + 64, f + 65, f + 127, f + 128, f + 129, hi - 1}):
        if not f <= s < hi:
            continue
        q = [20] * L
        q[s + w - 1] = 19
        exp = dict(null1=1) if s + w - 1 - f <= 0 else dict(null1=0, front1=f, len1=s + w - 1 - f)
        U.add(f"s{s}", rand_seq(rng, L), q, **exp)
        if w > 1:   # the low base further inside the window that fails first: a lower sum, the same first low base
            q = [20] * L
            q[s + w - 1] = 2
            q[s + w:s + w + 3] = [2] * len(q[s + w:s + w + 3])
            U.add(f"s{s}_deep", rand_seq(rng, L), q, **exp)
    U.add("none_fails", rand_seq(rng, L), [20] * L, null1=0, front1=f, len1=L - f - t)
    for n in LENGTHS:
        exp = dict(null1=1) if n - f - t - w <= 0 else dict(null1=0, front1=f, len1=n - f - t)
        if not exp["null1"] and f >= n - 1:
            exp = dict(null1=1)
        U.add(f"len{n}", rand_seq(rng, n), [20] * n, **exp)
    flags = ["-G", "-A", "--cut_right", "--cut_right_window_size", w, "--cut_right_mean_quality", 20, "-f", f, "-t", t]
    return Family(f"cut_right_L{L}_w{w}_f{f}", p, U, flags, edge=(f + 60, f + 69))


def cut_tail(L, w, f=0, t=0):
    """--cut_tail window w at Q20: counted from the tail, the first window at the threshold ends at e = hi - 63 / 64 / 65 ..
    (hi = l - tail - 1); N's in front of where the cut lands go as well"""
    rng = np.random.default_rng(300 + L + w + f)
    p = _se(L, cut_tail=1, cut_tail_window=w, cut_tail_quality=20, trim_front1=f, trim_tail1=t, length_required=1)
    U = Units(L, False)
    hi, lo = L - t - 1, f + w

    def unit(name, e, nrun):
        q = [20] * L
        q[e + 1:] = [2] * (L - e - 1)
        if e < lo:   # all windows fail: first_down returns lo - 1
            q = [20] * L
            q[lo - 1:] = [2] * (L - lo + 1)
            q[:f] = [20] * f
            e = lo - 1
        tt = e - w + 1 if e < L - 1 else e
        seq = list(rand_seq(rng, L))
        a = max(0, tt - nrun + 1) if nrun >= 0 else 0
        seq[a:tt + 1] = "N" * (tt + 1 - a)
        last = a - 1
        rlen = last - f + 1
        exp = dict(null1=1) if (rlen <= 0 or f >= L - 1) else dict(null1=0, front1=f, len1=rlen)
        U.add(name, "".join(seq), q, **exp)

    for e in sorted({hi, hi - 1, hi - 63, hi - 64, hi - 65, hi - 127, hi - 128, hi - 129, lo, lo - 1}):
        if lo - 1 <= e <= hi:
            unit(f"e{e}", e, 0)
            unit(f"e{e}_n3", e, 3)
    if L >= 136:
        # N's in front of the cut: first_down(0, t) starts a block of its own where the cut lands; the run ends on its last step,
        # on the first steps of the next block and well inside it, with real bases before it
        for nrun in (63, 64, 65, 70):
            assert (hi - w + 1 if hi < L - 1 else hi) - nrun > f
            unit(f"e{hi}_nrun{nrun}_ends_in_next_block", hi, nrun)
    unit("e63_nrun_to_front", hi - 63, -1)
    for n in LENGTHS:
        if n - f - t - w <= 0 or f >= n - 1:
            exp = dict(null1=1)
        else:   # every window at the threshold: the first one from the tail ends at n - t - 1
            e = n - t - 1
            tt = e - w + 1 if e < n - 1 else e
            exp = dict(null1=1) if tt - f + 1 <= 0 else dict(null1=0, front1=f, len1=tt - f + 1)
        U.add(f"len{n}", rand_seq(rng, n), [20] * n, **exp)
    flags = ["-G", "-A", "--cut_tail", "--cut_tail_window_size", w, "--cut_tail_mean_quality", 20, "-f", f, "-t", t]
    return Family(f"cut_tail_L{L}_w{w}_f{f}", p, U, flags, edge=(max(0, hi - 69), max(9, hi - 60)))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. PolyX::trimPolyG (polyx.cpp:16-42).  Step i of the walk looks at base rlen - 1 - i.
def _tail_read(rng, L, steps, body="ACT"):
    """a read of L bases whose tail, read backwards, is `steps` (step 0 = the last base); the rest from `body`"""
    return rand_seq(rng, L - len(steps), body) + "".join(reversed(steps))


def poly_g(L, min_len=10):
    rng = np.random.default_rng(400 + L + min_len)
    p = _se(L, poly_g=1, poly_g_min_len=min_len, length_required=1)
    U = Units(L, False)
    for B in (63, 64, 65, 127, 128, 129):
        if B + 2 > L:
            continue
        # five mismatches where (i + 1) / 8 allows them, the sixth at step B: the walk breaks there by `mismatch > 5`
        steps = ["G"] * (B + 1)
        for i in (7, 15, 23, 31, 39, B):
            steps[i] = "A"
        U.add(f"sixth_at_{B}", _tail_read(rng, L, steps), **(dict(len1=L - B) if B >= min_len else dict(len1=L)))
        # the block the walk breaks in holds no G in front of the break; the last G is in the block before (steps 64 k - 1)
        blk = B // 64 * 64
        if blk and B - blk <= 1:
            steps = ["G"] * (B + 1)
            mism = [7, 15, 23, 31, 39][:5 - (B - blk)] + list(range(blk, B + 1))
            for i in mism:
                steps[i] = "T"
            U.add(f"no_g_in_breaking_block_{B}", _tail_read(rng, L, steps), **(dict(len1=L - blk) if B >= min_len else dict(len1=L)))
    for n in (64, 65, 128):   # the walk runs out: every base goes
        if n <= L:
            U.add(f"all_g_{n}", "G" * n, len1=0 if n >= min_len else n)
    _length_units(U, rng, lambda n: dict(len1=n), letters="ACT")
    return Family(f"poly_g_L{L}_min{min_len}", p, U, ["-A", "-g", "--poly_g_min_len", min_len], edge=(L - 69, L - 60))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. PolyX::trimPolyX (polyx.cpp:49-116)
def poly_x(L):
    rng = np.random.default_rng(500 + L)
    p = _se(L, poly_x=1, poly_x_min_len=10, length_required=1)
    U = Units(L, False)
    for B in (63, 64, 65, 127, 128, 129):
        if B + 2 > L:
            continue
        for x, y, z in (("A", "T", "C"), ("C", "G", "A"), ("T", "G", "A")):
            # a poly-x tail, five other letters where cmp / 8 allows them, the sixth at step B: the walk breaks there, the
            # search back for x stops one step earlier
            steps = [x] * (B + 1)
            for i in (7, 15, 23, 31, 39, B):
                steps[i] = z
            U.add(f"{x}_sixth_at_{B}", _tail_read(rng, L, steps, body=z + y), len1=L - B, polyx1=1)
            # N counts for all four bases: an N tail with five x and five y; then y, then x at step B.  With the breaking step
            # counted x ties with y and wins (the first of A, T, C, G); without it y wins and the search back stops at B - 1
            steps = ["N"] * (B + 1)
            for k, i in enumerate((7, 15, 23, 31, 39)):
                steps[i], steps[i + 1] = x, y
            steps[B - 1], steps[B] = y, x
            U.add(f"{x}{y}_tie_broken_by_step_{B}", _tail_read(rng, L, steps, body=z), len1=L - B - 1, polyx1=1)
        # lower case in the tail matches nothing: the sixth foreign byte breaks the walk like any other letter
        steps = ["A"] * (B + 1)
        for i in (7, 15, 23, 31, 39, B):
            steps[i] = "a"
        U.add(f"lower_case_sixth_at_{B}", _tail_read(rng, L, steps, body="CG"), len1=L - B, polyx1=1)
    # the search back for the poly base crosses a block: three A, an N run, then C G T C G T: A is six short at step 75 and
    # still the most counted; the last A at or below step 75 is step 2
    steps = ["A"] * 3 + ["N"] * 67 + list("CGTCGT")
    U.add("search_back_across_a_block", _tail_read(rng, L, steps, body="CGT") if L >= 76 else "ACGT", **(dict(len1=L - 3, polyx1=1) if L >= 76 else dict(len1=4)))
    for n in (64, 65, 128):
        if n <= L:
            U.add(f"all_n_{n}", "N" * n, len1=n, polyx1=1)   # every count ties: A, and no A to be found: pos = -1, nothing goes
    _length_units(U, rng, lambda n: dict(len1=n, polyx1=0), letters="ACGT")
    return Family(f"poly_x_L{L}", p, U, ["-A", "-G", "-x", "--poly_x_min_len", 10], edge=(L - 69, L - 60))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. OverlapAnalysis::analyze (overlapanalysis.cpp:17-146).  Limit: min(5, (int)(overlap_len * 10 / 100.0)).
def _limit(ol, diff_limit=5, pct=10):
    return min(diff_limit, int(ol * (pct / 100.0)))


def analyze(L, allow_gap=1, overlapped_out=1, merge=0):
    """forward offsets (read 1 runs `o` bases ahead of rc(read 2)) and reverse ones (the insert is k bases shorter than read 2:
    both reads run into random 'adapter')"""
    rng = np.random.default_rng(600 + L)
    p = _pe(L, overlap_diff_percent_limit=10, allow_gap_overlap_trimming=allow_gap, overlapped_out=overlapped_out, merge=merge,
            correction=merge, length_required=1)
    U = Units(L, True)

    def forward(name, o, l1, l2, diffs=(), frag=None, lower=(), **exp):
        """r1 = F[:l1], rc(r2) = F[o : o + l2]; substitutions at overlap positions `diffs` of read 1"""
        F = frag or rand_seq(rng, o + l2)
        if not overlapped_out:
            exp.pop("exact_end", None)
        r1, r2 = F[:l1], rc(F[o:o + l2])
        r1 = sub(r1, [o + i for i in diffs])
        if lower:   # read 1 soft-masked there, read 2 the complement in lower case: complement() gives the CAPITAL, a difference
            r1 = "".join(c.lower() if i - o in lower else c for i, c in enumerate(r1))
            r2 = "".join(c.lower() if (l2 - 1 - i) in lower else c for i, c in enumerate(r2))
        U.add(name, r1, 40, r2, 40, **exp)

    def reverse(name, k, l, diffs=(), r1_edit=None, **exp):
        """insert of l - k bases in reads of l: r1 = F + tail, r2 = rc(F) + tail; rc(r2)[k:] = F"""
        F = rand_seq(rng, l - k)
        if merge and exp.get("offset") is not None:   # merge mode's own analysis comes after the adapters went: F against F
            exp.update(offset=0, ov_len=l - k, diff=len(diffs))
        r1 = sub(F, diffs) + rand_seq(rng, k)
        if r1_edit:
            r1 = r1_edit(r1)
        U.add(name, r1[:l], 40, rc(F) + rand_seq(rng, k), 40, **exp)

    for o in (63, 64, 65, 127, 128):   # accepted at candidate o: the last lane of a trip, the first of the next, one further
        if L - o < 30:
            continue
        ol = L - o
        forward(f"fwd_{o}", o, L, L, offset=o, ov_len=ol, diff=0, len1=L, exact_end=L)
        forward(f"fwd_{o}_diffs_at_limit", o, L, L, diffs=range(2, 2 + _limit(ol)), offset=o, ov_len=ol, diff=_limit(ol), exact_end=None)
        reverse(f"rev_{o}", o, L, offset=-o, ov_len=ol, diff=0, len1=ol, len2=ol, ov_trim=1)
    # two acceptable offsets: a periodic insert matches at every offset of the same residue; the lowest wins
    if L >= 136:
        for per, o, name in ((10, 23, "one_trip"), (50, 70, "two_trips"), (64, 65, "lanes_1_and_65")):
            unit = rand_seq(rng, per)
            frag = (unit * (2 * L // per + 2))[:o + L]
            forward(f"fwd_two_offsets_{name}", o, L, L, frag=frag, offset=o % per, ov_len=L - o % per, diff=0)
            # the reverse direction: the insert is periodic, so candidates k, k + per, .. all match; k is tried first
            k = {10: 23, 50: 30, 64: 65}[per]
            ins = (unit * (L // per + 2))[:L - k]
            exp = dict(offset=0, ov_len=L - k, diff=0, len1=L - k) if merge else dict(offset=-k, ov_len=L - k, diff=0, len1=L - k)
            U.add(f"rev_two_offsets_{name}", ins + rand_seq(rng, k), 40, rc(ins) + rand_seq(rng, k), 40, **exp)
    # overlap_len at the requirement, and on both sides of the complete-compare prefix
    # (the loops run `while offset < len1 - overlapRequire`: the shortest overlap ever tried is the requirement + 1)
    for ol in (31, 50, 51):
        o = L - ol
        forward(f"fwd_ol{ol}", o, L, L, offset=o, ov_len=ol, diff=0)
        forward(f"fwd_ol{ol}_one_above", o, L, L, diffs=range(1, 2 + _limit(ol)), offset=None)
    forward("fwd_ol30_is_never_tried", L - 30, L, L, offset=None)
    # (int)(39 * 10 / 100.0) = 3: three differences pass, four do not
    forward("fwd_ol39_three", L - 39, L, L, diffs=(3, 17, 30), offset=L - 39, ov_len=39, diff=3)
    forward("fwd_ol39_four", L - 39, L, L, diffs=(3, 17, 30, 36), offset=None)
    # the first 50 positions decide; the rest is only counted
    o, ol = 8, L - 8
    forward("first50_at_limit", o, L, L, diffs=(0, 10, 20, 30, 49), offset=o, ov_len=ol, diff=5)
    forward("first50_one_above", o, L, L, diffs=(0, 10, 20, 30, 40, 49), offset=None)
    forward("above_only_behind_50", o, L, L, diffs=(0, 10, 20, 50, 55, 63), offset=o, ov_len=ol, diff=6)
    forward("all_behind_50", o, L, L, diffs=tuple(range(50, 64)), offset=o, ov_len=ol, diff=14)
    # raw bytes: soft-masked bases of read 1 against complemented lower case of read 2 differ
    forward("lower_case_at_limit", o, L, L, lower=(5, 15, 25, 35, 45), offset=o, ov_len=ol, diff=5)
    forward("lower_case_one_above", o, L, L, lower=(5, 15, 25, 35, 45, 48), offset=None)
    if allow_gap:
        # one-gap accept (synth.indel_overlap_pairs): the ungapped scan rejects (limit + 1 differences, the last two positions among
        # them), Matcher::diffWithOneInsertion accepts with the split at the end.  At reverse candidate k in the second trip.
        for k in (64, 65):
            if L - k < 40:
                continue
            ol = 40
            l = k + ol
            body = tuple(range(4, 4 + 6 * (_limit(ol) - 1), 6))

            def ends(r, ol=ol):   # the last two overlap positions differ, the last one also from its left neighbour's partner
                x = next(c for c in "ACGT" if c not in (r[ol - 1], r[ol - 2]))   # (either read can be the one with the insertion)
                return r[:ol - 2] + x + x + r[ol:]
            reverse(f"gap_accept_rev_{k}", k, l, diffs=body, r1_edit=ends, offset=None, ov_trim=1, len1=ol, len2=ol)
            reverse(f"gap_reject_rev_{k}", k, l, diffs=body + (1,), r1_edit=ends, offset=None, ov_trim=0, len1=l)
            # a REAL inserted base in read 1: the best split is clean, but the unsplit prefix is far above the limit - the
            # reference says no (matcher.cpp:88-97)
            reverse(f"gap_real_insertion_rev_{k}", k, l, r1_edit=lambda r: r[:12] + _OTHER[r[12]] + r[12:], offset=None, ov_trim=0, len1=l)
    for n in LENGTHS + (L,):
        s = rand_seq(rng, n)
        exp = dict(offset=0, ov_len=n, diff=0) if n >= 30 else dict(offset=None)
        U.add(f"len{n}", s, 40, rc(s), 40, **exp)
    flags = ["-G", "--overlap_diff_percent_limit", 10]
    flags += ["--allow_gap_overlap_trimming"] if allow_gap else []
    flags += ["--overlapped_out", "@TMP@/overlapped.fq"] if overlapped_out else []
    flags += ["-m", "-c", "--merged_out", "@TMP@/merged.fq"] if merge else []
    return Family(f"analyze_L{L}_gap{allow_gap}_ovl{overlapped_out}_m{merge}", p, U, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. AdapterTrimmer::trimBySequence (adaptertrimmer.cpp:64-157): lane = position + 4 for adapters of 16 bases and more
def by_sequence(L, adapter, tag):
    rng = np.random.default_rng(700 + L + len(adapter))
    p = _se(L, adapter_enabled=1, adapter_seq_r1=adapter.encode(), length_required=1)
    U = Units(L, False)
    alen = len(adapter)
    start = -4 if alen >= 16 else -3 if alen >= 12 else -2 if alen >= 8 else 0
    avoid = adapter[:4]

    def prefix(n):   # random bases that do not hold the adapter's first four (a four-base hit needs no more at the read's end)
        while True:
            s = rand_seq(rng, n)
            if avoid not in s + adapter[:3]:
                return s

    for pos in (59, 60, 61, 123, 124, 125):
        if pos + 4 > L:
            continue
        s = (prefix(pos) + adapter + "A" * L)[:L]
        U.add(f"hit_at_{pos}", s, apos1=pos, len1=pos)
        if alen >= 16:   # one difference per eight bases compared is allowed
            s = (prefix(pos) + sub(adapter, (2,)) + "A" * L)[:L]
            if min(L - pos, alen) >= 8:
                U.add(f"hit_at_{pos}_one_diff", s, apos1=pos, len1=pos)
    for sh in range(1, 5):
        if alen - sh < 4:
            continue
        s = (adapter[sh:] + "C" + prefix(L))[:L]
        U.add(f"hit_at_minus_{sh}", s, **(dict(apos1=-sh, len1=0) if -sh >= start else dict(apos1=None, len1=L)))
    for n in (4, 5, min(alen - 1, L), min(alen, L)):   # reads shorter than the adapter that begin with it (4 bases: position 0 is not tried)
        U.add(f"short_{n}", adapter[:n], **(dict(apos1=0, len1=0) if n > 4 else dict(apos1=None, len1=n)))
    # (a one-base read is compared with the adapter's fifth base at position -4 and goes if it equals it)
    _length_units(U, rng, lambda n: dict(apos1=None, len1=n), letters="T")
    return Family(f"by_sequence_L{L}_{tag}", p, U, ["-G", "-a", adapter], edge=(56, 65))


def by_sequence_insertion(L=136):
    """the two one-insertion loops (adaptertrimmer.cpp:105-135) compare the read FROM ITS START whatever position they are at;
    the position only shortens the compared length.  The read starts with m clean adapter bases around one extra (loop 1) or
    one missing (loop 2) base and goes on with bases that differ from the adapter under either alignment, so a position is
    accepted once the compared length has shrunk to what the clean part allows: 64 and above here (the 131-base adapter)."""
    ad = cases.LONG_MIXED
    p = _se(L, adapter_enabled=1, adapter_seq_r1=ad.encode(), length_required=1)
    U = Units(L, False)

    def wrong(i):   # a base that equals none of the adapter's bases an alignment could put against read position i
        near = {ad[j] for j in (i - 1, i, i + 1) if 0 <= j < len(ad)}
        return next(c for c in "ACGT" if c not in near)

    for pos in (64, 65, 70):
        for kind in ("read_has_one_more", "read_has_one_less"):
            # compared length at `pos`: loop 1 min(rlen - pos - 1, alen), loop 2 min(rlen - pos, alen - 1); its limit c / 8 - 1.
            # `clean` compared positions agree and every further one differs: c is accepted, and c + 1 (one position earlier) is
            # not as long as its limit is the same, (c + 1) % 8 != 0
            c = min(70, L - pos - 1)
            assert (c + 1) % 8
            rlen = pos + c + (1 if kind == "read_has_one_more" else 0)
            clean = c - (c // 8 - 1)
            if kind == "read_has_one_more":
                head = ad[:5] + wrong(5) + ad[5:clean]
            else:
                head = ad[:5] + ad[6:clean + 1]
            s = head + "".join(wrong(i) for i in range(len(head), rlen))
            U.add(f"{kind}_at_{pos}", s[:rlen], apos1=pos, len1=pos)
    _length_units(U, np.random.default_rng(750), lambda n: dict(apos1=None, len1=n), letters="T")
    return Family(f"by_sequence_insertion_L{L}", p, U, ["-G", "-a", ad], edge=(100, 110))


def by_fasta(L=136):
    """--adapter_fasta: two contigs hit the same read, the second one in front of the first one's cut"""
    rng = np.random.default_rng(800 + L)
    X, Y = "CTGTCTCTTATACACATCT", "TGGAATTCTCGGGTGCCAAGG"
    Z = "GTTGTTTGTTGTTTGTTGTT"   # -a: hits nothing here (without it the reference would look for a single-end adapter itself)
    p = abi.set_adapter_fasta(_se(L, adapter_enabled=1, adapter_seq_r1=Z.encode(), length_required=1), [X.encode(), Y.encode()])
    U = Units(L, False)
    body = lambda n: rand_seq(rng, n, "AC")
    for pos in (59, 60, 61):
        U.add(f"two_contigs_{pos}", body(pos) + Y + body(100 - pos - len(Y)) + X + body(L - 100 - len(X)), len1=pos, events=2)
        U.add(f"first_contig_{pos}", body(pos) + X + body(L - pos - len(X)), len1=pos, events=1)
        U.add(f"second_contig_{pos}", body(pos) + Y + body(L - pos - len(Y)), len1=pos, events=1)
    # (a one-base read is compared with the contig's fifth base at position -4 and goes if it equals it: G equals neither)
    _length_units(U, rng, lambda n: dict(len1=n, events=0), letters="G")
    fasta = f">x\n{X}\n>y\n{Y}\n".encode()
    return Family(f"by_fasta_L{L}", p, U, ["-G", "-a", Z, "--adapter_fasta", "@TMP@/adapters.fa"], edge=(56, 65), files={"adapters.fa": fasta})


# ---------------------------------------------------------------------------------------------------------------------------
# 6. BaseCorrector, Stats::statRead, the merged read
def correct_merge(L, merge=1, include_unmerged=0):
    rng = np.random.default_rng(900 + L)
    p = _pe(L, correction=1, merge=merge, merge_include_unmerged=include_unmerged, length_required=1)
    U = Units(L, True)
    o = 10
    ol = L - o
    for at in ((63, 64, 65), (127, 128, 129), (0, 63, 64, ol - 1)):
        at = tuple(i for i in at if i < ol)
        if len(at) < 2:
            continue
        for fix in (1, 2):   # which read is corrected: the other one is good (Q40) where this one is bad (Q10)
            F = rand_seq(rng, o + L)
            r1, r2 = sub(F[:L], [o + i for i in at]), rc(F[o:o + L])
            q1, q2 = [40] * L, [40] * L
            for i in at:
                (q1 if fix == 1 else q2)[o + i if fix == 1 else L - 1 - i] = 10
            exp = dict(offset=o, ov_len=ol, ncorr=len(at))
            if merge:
                exp["merged"] = L + o
            U.add(f"correct_read{fix}_at_{'_'.join(map(str, at))}", r1, q1, r2, q2, **exp)
    # a merged read longer than max_len: Stats' cycles run past the read length
    for o2 in (L - 36, L - 63, L - 64, L - 65):
        F = rand_seq(rng, o2 + L)
        exp = dict(offset=o2, ov_len=L - o2, merged=L + o2) if merge else dict(offset=o2, ov_len=L - o2)
        U.add(f"merged_{L + o2}", F[:L], 40, rc(F[o2:]), 40, **exp)
    # a foreign letter at 60 .. 68: the 5-mer window's restart crosses the block edge (these units are listed for the text kernel)
    for pos in range(60, 69):
        F = rand_seq(rng, L + 20)
        r1 = F[:pos] + "R" + F[pos + 1:L]
        U.add(f"foreign_at_{pos}", r1, 40, rc(F[20:L + 20]), 40, offset=20, ov_len=L - 20, diff=1)
    for n in LENGTHS + (L,):
        s = rand_seq(rng, n)
        exp = dict(offset=0, ov_len=n, diff=0) if n >= 30 else dict(offset=None)
        U.add(f"len{n}", s, 40, rc(s), 40, **exp)

    def counters(ctr, lay):
        """5-mers of read 1 before filtering: position i >= 4 counts iff the letters i - 4 .. i are all ACGT"""
        want = 0
        for s1, _, _, _ in U.rows:
            want += sum(1 for i in range(4, len(s1)) if all(c in "ACGT" for c in s1[i - 4:i + 1]))
        got = int(ctr[lay.stats[0] + lay.st_kmer:lay.stats[0] + lay.st_kmer + 1024].sum())
        return [] if got == want else [f"5-mers of read 1 before filtering: {got}, built for {want}"]

    flags = ["-G", "-c"] + (["-m", "--merged_out", "@TMP@/merged.fq"] if merge else []) + (["--include_unmerged"] if include_unmerged else [])
    return Family(f"correct_merge_L{L}_m{merge}{include_unmerged}", p, U, flags, counters=counters)


# name -> builder.  Each family runs at the smallest max_len that holds it: 72 one block edge, 136 two, 200 the overlap candidates
# of the third trip.  (The names are the tests' parameter ids and the fixtures' file names.)
_SHORT = {n: cases.ADAPTER_R1[:n] for n in (7, 8, 11, 12, 15, 16)}
FAMILIES = {
    "cut_front_w1": lambda: cut_front(72, 1),
    "cut_front_w4": lambda: cut_front(136, 4),
    "cut_front_w40_umi_ft": lambda: cut_front(136, 40, f=3, t=2, umi=5),
    "cut_right_w1": lambda: cut_right(72, 1),
    "cut_right_w4_ft": lambda: cut_right(136, 4, f=3, t=2),
    "cut_right_w40": lambda: cut_right(136, 40),
    "cut_right_w70": lambda: cut_right(136, 70),
    "cut_tail_w1": lambda: cut_tail(72, 1),
    "cut_tail_w4_ft": lambda: cut_tail(136, 4, f=3, t=2),
    "cut_tail_w40": lambda: cut_tail(136, 40),
    "poly_g_72": lambda: poly_g(72),
    "poly_g_136": lambda: poly_g(136),
    "poly_g_136_min65": lambda: poly_g(136, 65),
    "poly_x_72": lambda: poly_x(72),
    "poly_x_136": lambda: poly_x(136),
    "analyze_72": lambda: analyze(72),
    "analyze_136": lambda: analyze(136),
    "analyze_200": lambda: analyze(200),
    # (--merge with --overlapped_out: the first context of a process with these options pays the runtime's one-time cost of that
    # kernel, 3 to 18 s on the GPU; behind tests/test_gpu_parity.py's pe_merge_overlapped_out the family takes 0.03 s)
    "analyze_136_merge": lambda: analyze(136, allow_gap=0, overlapped_out=1, merge=1),
    "analyze_136_plain": lambda: analyze(136, allow_gap=0, overlapped_out=0),
    "by_sequence_r1": lambda: by_sequence(136, cases.ADAPTER_R1, "r1"),
    "by_sequence_long": lambda: by_sequence(136, cases.LONG_MIXED, "long"),
    **{f"by_sequence_a{n}": (lambda a=a, n=n: by_sequence(72, a, f"a{n}")) for n, a in _SHORT.items()},
    "by_sequence_insertion": lambda: by_sequence_insertion(136),
    "by_fasta": lambda: by_fasta(136),
    "correct_136": lambda: correct_merge(136, merge=0),
    "correct_merge_136": lambda: correct_merge(136),
    "correct_merge_136_unmerged": lambda: correct_merge(136, include_unmerged=1),
    "correct_merge_200_global_atomics": lambda: correct_merge(200),
}
# the plan each family's options are meant for (fastp_gpu_plan): the lane kernel where nothing asks for more than it covers - windows
# of up to 8 bases, adapters of up to 64, no one-gap overlap, no --overlapped_out; the other families pin the tile kernels
PLAN = {name: "lane" for name in FAMILIES}
PLAN.update(cut_front_w40_umi_ft="fused", cut_right_w40="split", cut_right_w70="split", cut_tail_w40="split", analyze_72="split",
            analyze_136="split", analyze_200="split", analyze_136_merge="fused", by_sequence_long="split", by_sequence_insertion="split")
_BUILT = {}


def family(name):
    if name not in _BUILT:
        _BUILT[name] = FAMILIES[name]()
    return _BUILT[name]


def fastq(fam, d=None):
    """the family as FASTQ text (read 1, read 2 or None)"""
    import synth
    d = d or fam.d
    return (synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1),
            synth.to_fastq(d["seq2"], d["qual2"], d["len2"], 2) if fam.paired else None)
