"""Hand-built seeds and reads for tests/test_overrep_kernels.py (the overrepresentation kernels, fq_device.h ovr_*).

Generators only: no expected value is computed here - every expected counter comes from oraclelib.Oracle.  The one piece
of the engine restated below is the seed table's build (fq_host.cpp, "overrepresentation analysis seeds -> hash tables";
constants from fq_types.h), and it is used only to CHOOSE inputs: seeds that collide into probe chains and across the
table's wrap-around, and read windows that are no seeds but land on an occupied first slot."""
import numpy as np

import synth
from fastp_amd import abi

HASH_MUL = 0x01000193   # OVR_HASH_MUL
SALT_MUL = 0x9E3779B1   # OVR_SALT_MUL
M32 = 0xFFFFFFFF
ACGT = b"ACGT"
_SYM = {ord("A"): 0, ord("T"): 1, ord("C"): 2, ord("G"): 3, ord("N"): 4}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def steps_for(eval_len):
    """stats.cpp:273"""
    return [10, 20, 40, 100, min(150, eval_len - 2)]


def live_steps(eval_len):
    return sorted({s for s in steps_for(eval_len) if s > 0})


# ---- the table build, restated to choose inputs -------------------------------------------------------------------
def seed_key(s: bytes) -> int:
    h = 0
    for b in s:
        h = (h * HASH_MUL + _SYM.get(b, b) + 1) & M32
    return h ^ ((len(s) * SALT_MUL) & M32)


def table_slots(n_seeds):
    slots = 16
    while slots < n_seeds * 4:
        slots <<= 1
    return slots


def build_table(seeds):
    """-> (slots, ids [slots] (seed index + 1, 0 = empty), home slot per seed, final slot per seed)"""
    slots = table_slots(len(seeds))
    ids = [0] * slots
    home, final = [], []
    for i, s in enumerate(seeds):
        sl = ((seed_key(s) * SALT_MUL) & M32) & (slots - 1)
        home.append(sl)
        while ids[sl]:
            sl = (sl + 1) & (slots - 1)
        ids[sl] = i + 1
        final.append(sl)
    return slots, ids, home, final


def table_facts(seeds):
    """longest probe (slots looked at until a listed seed is found) and the seeds displaced past the wrap-around"""
    slots, ids, home, final = build_table(seeds)
    probe = [((f - h) & (slots - 1)) + 1 for h, f in zip(home, final)]
    return {"slots": slots, "longest_probe": max(probe), "wrapped": sum(1 for h, f in zip(home, final) if f < h)}


def _home_of_codes(codes, slots):
    """home slots of 10-mers given as engine codes (A0 T1 C2 G3) [n, 10], vectorised"""
    h = np.zeros(len(codes), dtype=np.uint64)
    for k in range(codes.shape[1]):
        h = (h * np.uint64(HASH_MUL) + codes[:, k].astype(np.uint64) + np.uint64(1)) & np.uint64(M32)
    key = h ^ np.uint64((codes.shape[1] * SALT_MUL) & M32)
    return ((key * np.uint64(SALT_MUL)) & np.uint64(M32)) & np.uint64(slots - 1)


_ATCG = np.frombuffer(b"ATCG", dtype=np.uint8)


def probing_list(rng, n_seeds=300, n_decoys=60):
    """A seed list (10-mers, in table order - NOT sorted) whose table holds a probe chain of three in its middle, a chain
    that starts in the last slot and continues at slots 0 and 1, and a seed whose home is slot 0 displaced behind them;
    and decoys: 10-mers that are no seeds but whose first slot is the head of one of these chains, so that the probe
    walks the whole chain (across the wrap-around) before it finds the empty slot."""
    slots = table_slots(n_seeds)
    codes = np.unique(rng.integers(0, 4, size=(200000, 10), dtype=np.uint8), axis=0)
    rng.shuffle(codes)
    home = _home_of_codes(codes, slots).astype(np.int64)
    text = _ATCG[codes]
    mid = slots // 2 + 5
    pick = []
    for h, k in ((slots - 1, 3), (0, 1), (mid, 3)):     # inserted first, in this order: their slots are certain
        pick += list(np.flatnonzero(home == h)[:k])
    assert len(pick) == 7
    used = set(pick)
    heads = {slots - 1, 0, 1, 2, mid, mid + 1, mid + 2}
    decoys = [i for i in np.flatnonzero(np.isin(home, [slots - 1, 0, mid])) if i not in used][:n_decoys]
    used |= set(decoys)
    # filler whose home is none of the chains' slots, so the chains stay as built
    fill = [int(i) for i in np.flatnonzero(~np.isin(home, list(heads)))[:n_seeds + len(used)] if i not in used][:n_seeds - len(pick)]
    seeds = [text[i].tobytes() for i in pick + fill]
    return seeds, [text[i].tobytes() for i in decoys]


def occupied_first_slot(seeds, windows):
    """how many of `windows` (10-mers) are no seeds but hash to an occupied first slot"""
    slots, ids, _, _ = build_table(seeds)
    listed = set(seeds)
    return sum(1 for w in windows if w not in listed and ids[((seed_key(w) * SALT_MUL) & M32) & (slots - 1)])


# ---- seeds ------------------------------------------------------------------------------------------------------
def rand_seq(rng, n, alphabet=ACGT):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)])


def with_n(s, at=1, k=1):
    """a seed that random ACGT text cannot hold by accident: k N from position `at`"""
    at = min(at, len(s) - 1)
    k = min(k, len(s) - at)
    return s[:at] + b"N" * k + s[at + k:]


def seed_list(rng, eval_len, count=0):
    """-> (seeds sorted as Options::overRepSeqs is, the structured ones among them): every step length of the context,
    seeds with an N, a 10-mer that is a prefix of a listed 20-mer that is a prefix of a listed 40-mer, filler 10-mers
    up to `count`"""
    core = []
    for s in live_steps(eval_len):
        if s == 1:
            core += [b"A", b"N"]
            continue
        core += [rand_seq(rng, s), with_n(rand_seq(rng, s), at=int(rng.integers(0, s)))]
    p40 = rand_seq(rng, 40)
    core += [p40, p40[:20], p40[:10]]
    core = sorted(set(core))
    seeds = set(core)
    while len(seeds) < count:
        seeds |= {rand_seq(rng, 10) for _ in range(count - len(seeds))}
    return sorted(seeds), core


# ---- reads ------------------------------------------------------------------------------------------------------
def rows(reads, max_len, quals=None):
    """list of bytes -> ASCII rows [n, stride] + lengths; quality constant 'I' unless given per read"""
    stride = (max_len + 7) // 8 * 8
    n = len(reads)
    seq = np.zeros((n, stride), dtype=np.uint8)
    qual = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(reads):
        assert len(r) <= max_len
        seq[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        qual[i, :len(r)] = np.frombuffer(quals[i], dtype=np.uint8) if quals is not None else ord("I")
        lens[i] = len(r)
    return seq, qual, lens


def as_batch(reads1, reads2, max_len, quals1=None, quals2=None):
    d = {}
    d["seq1"], d["qual1"], d["len1"] = rows(reads1, max_len, quals1)
    if reads2 is not None:
        assert len(reads2) == len(reads1)
        d["seq2"], d["qual2"], d["len2"] = rows(reads2, max_len, quals2)
    return d


def seed_reads(seeds, n, L, rng, favoured=(), cut_frac=0.3, min_len=0):
    """reads that are concatenations of seeds with gaps of 0 to 3 random bases; a share is cut to a random length"""
    fit = [s for s in seeds if len(s) <= L]
    fav = [s for s in favoured if len(s) <= L]
    out = []
    for _ in range(n):
        r = rand_seq(rng, int(rng.integers(0, 4)))
        while len(r) < L:
            pool = fav if fav and rng.random() < 0.25 else fit
            r += pool[int(rng.integers(0, len(pool)))] + rand_seq(rng, int(rng.integers(0, 4)))
        r = r[:L]
        if rng.random() < cut_frac:
            r = r[:int(rng.integers(min_len, L + 1))]
        out.append(r)
    return out


def _place(rng, rl, plants):
    """random ACGT text of rl bases with the (position, bytes) plants written over it"""
    r = bytearray(rand_seq(rng, rl))
    for at, s in plants:
        assert 0 <= at and at + len(s) <= rl, (at, len(s), rl)
        r[at:at + len(s)] = s
    return bytes(r)


def _near_misses(s):
    """one base changed at the first, a middle and the last position"""
    out = []
    for at in sorted({0, len(s) // 2, len(s) - 1}):
        c = s[at:at + 1]
        out.append(s[:at] + (b"A" if c != b"A" else b"C") + s[at + 1:])
    return out


def _marker(rng, s, taken):
    """a marker seed: N N at its second and third base (no other seed holds that, the background no N at all) - N N N in
    a marker shorter than 10, which the longer markers then cannot hold either - and two or more bases away from every
    earlier marker, so that no marker's near-miss is another marker"""
    for _ in range(1000):
        m = with_n(rand_seq(rng, s), k=2 if s >= 10 else 3)
        if all(len(t) != s or sum(a != b for a, b in zip(t, m)) >= 2 for t in taken):
            taken.append(m)
            return m
    raise AssertionError("no room for another marker")


def planted(rng, max_len, eval_len):
    """One mate's hit-rule reads.  -> (reads, seeds, marks); marks = {"last": seed indices planted ONLY at len - step - 1
    (the last window examined), "never": seed indices planted ONLY at len - step (never examined)}.  Every marker seed
    holds an N and the background is plain ACGT, so a marker is nowhere by accident.  Per step length s, with read
    lengths max_len .. max_len - 3 (the four sizes of a walk's last trip):
      a seed at 0; at len - s - 1; at len - s; at every position 0..7 (each slide of a trip, twice over); twice back to
      back at a gap of 0 (the second copy is skipped) and of 1 (counted); at >= eval_len, eval_len - 1 and
      eval_len - s + 1 (the clip of `dist`); the near-misses of each; the nested 10 / 20 / 40-mer prefixes at one place."""
    seeds, core = seed_list(rng, eval_len)
    seeds = list(seeds)
    reads, last, never, markers = [], [], [], []

    def add_seed(s):
        if s in seeds:
            return None
        seeds.append(s)
        return len(seeds) - 1

    for s in live_steps(eval_len):
        if s >= max_len:
            continue
        listed = [q for q in core if len(q) == s]
        a = listed[0]
        for rl in range(max_len, max(max_len - 4, s), -1):
            reads.append(_place(rng, rl, [(0, a)]))
            if s >= 10 or (s >= 5 and rl >= max_len - 1):   # (a 5-mer has room for four markers)
                lm, nm = _marker(rng, s, markers), _marker(rng, s, markers)
                il, inv = add_seed(lm), add_seed(nm)
                if il is not None and inv is not None:
                    last.append(il)
                    never.append(inv)
                    reads.append(_place(rng, rl, [(rl - s - 1, lm)]))
                    reads.append(_place(rng, rl, [(rl - s, nm)]))
                    reads += [_place(rng, rl, [(rl - s - 1, x)]) for x in _near_misses(lm)]
        rl = max_len
        for at in range(8):
            if at + s <= rl:
                reads.append(_place(rng, rl, [(at, listed[-1])]))
        for gap in (0, 1):
            for at in (0, 3):
                if at + 2 * s + gap <= rl:
                    reads.append(_place(rng, rl, [(at, a), (at + s + gap, a)]))
        for at in (eval_len, eval_len + 2, eval_len - 1, eval_len - s + 1, eval_len - s):
            if 0 <= at and at + s <= rl:
                reads.append(_place(rng, rl, [(at, a)]))
        reads += [_place(rng, rl, [(min(2, rl - s), x)]) for x in _near_misses(a)]
    p40 = next(q for q in core if len(q) == 40 and q[:20] in core and q[:10] in core)
    for at in (0, 5, max_len - 41, max_len - 40):
        if 0 <= at and at + 40 <= max_len:
            reads.append(_place(rng, max_len, [(at, p40)]))
    reads += seed_reads([q for q in core if b"N" not in q], 12, max_len, rng, cut_frac=0.5)   # (no marker, no N: those stay where they were planted)
    return reads, seeds, {"last": last, "never": never, "core": core}


# ---- merge-mode pairs that really merge -------------------------------------------------------------------------
def rc(s):
    return s.translate(_COMP)[::-1]


JOIN, POST_ONLY, PRE_ONLY, PLAIN = range(4)


def merge_pairs(rng, n, L, kinds, join, post_only, pre_only, plain_seeds):
    """Pairs whose read 2 is the reverse complement of a common fragment, inserts L + 20 .. 2L - 30 (overlaps L - 20 .. 30).
    kinds[i] says what unit i carries:
      JOIN       the 20-mer `join` across the join of the r1 part and the rc(r2') tail of the merged read (neither mate
                 holds it whole)
      POST_ONLY  `post_only` inside the overlap; read 1 has one base of it wrong at quality '#', which -c corrects from
                 read 2: only the corrected read holds the seed
      PRE_ONLY   read 1 holds `pre_only` inside the overlap, one base of it against read 2 at quality '#': the corrected
                 read no longer holds it
      PLAIN      seeds of plain_seeds strewn over the fragment, no mismatch
    -> batch dict"""
    r1s, r2s, q1s = [], [], []
    for i in range(n):
        k = kinds[i]
        # (an overlap of exactly overlap_require is never found - the scan stops one offset short, overlapanalysis.cpp:27 - so a
        # pair of 2L - 30 stays unmerged and uncorrected: the units whose point is the correction stop one short of it)
        ins = int(rng.integers(L + 20, 2 * L - 30 + (0 if k in (POST_ONLY, PRE_ONLY) else 1)))
        F = bytearray(rand_seq(rng, ins))
        q1 = bytearray(b"I" * L)
        err = None
        if k == JOIN:
            F[L - 10:L + 10] = join
        elif k in (POST_ONLY, PRE_ONLY):
            at = int(rng.integers(ins - L, L - 20 + 1))          # inside the overlap [ins - L, L)
            sd = post_only if k == POST_ONLY else pre_only
            e = at + 7
            if k == POST_ONLY:
                F[at:at + 20] = sd
                err = (e, b"A" if F[e:e + 1] != b"A" else b"C")  # read 1 differs from the fragment here
            else:
                F[at:at + 20] = sd
                good = b"A" if sd[7:8] != b"A" else b"C"         # the fragment (and read 2) differ from the seed here
                F[e:e + 1] = good
                err = (e, sd[7:8])
        else:
            at = int(rng.integers(0, 8))
            while at + 10 <= ins:
                s = plain_seeds[int(rng.integers(0, len(plain_seeds)))]
                if at + len(s) <= ins:
                    F[at:at + len(s)] = s
                at += len(s) + int(rng.integers(0, 30))
        F = bytes(F)
        r1 = bytearray(F[:L])
        if err is not None:
            r1[err[0]:err[0] + 1] = err[1]
            q1[err[0]] = ord("#")
        r1s.append(bytes(r1))
        q1s.append(bytes(q1))
        r2s.append(rc(F)[:L])
    return as_batch(r1s, r2s, L, quals1=q1s)


def exotic_seeds(d, units, mate="1", k=4):
    """10-mers cut from reads of `units` around a letter outside ACGTN: seeds that carry such a byte"""
    out = []
    for i in units:
        L = int(d["len" + mate][i])
        row = d["seq" + mate][i, :L]
        bad = np.flatnonzero(~np.isin(row, np.frombuffer(b"ACGTN", dtype=np.uint8)))
        if len(bad) and L >= 10:
            a = min(max(0, int(bad[0]) - 3), L - 10)
            out.append(row[a:a + 10].tobytes())
        if len(out) >= k:
            break
    return out


def add_exotic_to(d, a, b, seed, paired=True):
    """synth.add_exotic over units [a, b) in place"""
    synth.add_exotic({k: v[a:b] for k, v in d.items()}, seed=seed, read_frac=0.7, paired=paired)


def fail_a_third(d, rng, paired, min_len):
    """in place: about a third of the units fail a filter - a mate shorter than length_required, or more N than n_base_limit"""
    n = len(d["len1"])
    for i in np.flatnonzero(rng.random(n) < 0.34):
        m = "2" if paired and rng.random() < 0.5 else "1"
        L = int(d["len" + m][i])
        if rng.random() < 0.5 or L < 12:
            cut = int(rng.integers(0, min_len))
            d["len" + m][i] = min(L, cut)
            d["seq" + m][i, cut:] = 0
            d["qual" + m][i, cut:] = 0
        else:
            d["seq" + m][i, rng.choice(L, size=7, replace=False)] = ord("N")
    return d


def cut_windows(d, mate, rng, k=30, w=10):
    """k windows of w bases cut from full-length reads of one mate: seeds that the reads hold as they are"""
    full = np.flatnonzero(d["len" + mate] >= w)
    return sorted({d["seq" + mate][i, a:a + w].tobytes() for i in rng.choice(full, size=k)
                   for a in [int(rng.integers(0, int(d["len" + mate][i]) - w + 1))]})


def plant_duplicates(d, rng, frac=0.5):
    n = len(d["len1"])
    if n < 2:
        return d
    dst = rng.choice(np.arange(1, n), size=max(1, int(n * frac)), replace=False)
    src = (rng.random(len(dst)) * dst).astype(np.int64)
    for k in d:
        d[k][dst] = d[k][src]
    return d


def hits(co, lay, slot):
    """the overrepresentation counts of one Stats object from a counter block"""
    a = int(lay.overrep_count[slot])
    return co[a:a + int(lay.n_overrep[slot])]


def params(paired, max_len, seeds1, seeds2, eval_len, sampling, **opts):
    p = abi.default_params(paired, max_len)
    p.adapter_enabled = 0
    p.n_base_limit = 5
    if not paired:
        p.adapter_seq_r1 = None
    for k, v in opts.items():
        setattr(p, k, v)
    return abi.set_overrep(p, seeds1, seeds2 if paired else [], eval_len, eval_len if paired else 0, sampling)
