"""The adapter census (fastp_gpu_adapter_census, csrc/fq_census.h): FilterResult::mAdapter1 / mAdapter2 counted on the
device.  Expected maps never come from the code under test: they are hostloop.AdapterMaps replayed by
hostloop.apply_results over the same records (the literal port of src/filterresult.cpp:115-180, pinned to the reference by
the goldens), or the reference's own JSON in tests/golden.  Maps are compared as whole dicts.

Every family is one list of cases, run as test_sim_* on the emulator and as its test_gpu_* twin on the device.

1. goldens   every golden family whose reference JSON lists an adapter string (testdata_pe, 8 pairs, has the section but
             trims no read: both its maps are empty, so it cannot be told from a census that does nothing and is left out)
2. edges     hand-built records and text, no engine run
3. caps      the 5000 / 20000 thresholds, crossed inside a call and reached exactly at a call boundary
4. quirk #8  the pair form's early return
5. collisions FASTP_GPU_DEBUG_CENSUS_HASH_BITS=4
6. the launch split does not matter"""
import functools

import numpy as np
import pytest

import cases
import census_util as U
import engines
import golden_util
import refjson
from fastp_amd import abi, hostloop

RF_A, RF_OV = abi.RF_ADAPTER, abi.RF_ADAPTER_OV
A1, A2 = cases.ADAPTER_R1.encode(), cases.ADAPTER_R2.encode()


def _params(paired, max_len=152, fasta=None):
    p = abi.default_params(paired, max_len)
    p.adapter_seq_r1 = A1
    p.adapter_seq_r2 = A2 if paired else None
    if fasta:
        abi.set_adapter_fasta(p, fasta)
    return p


def _map_order(d):
    return sorted(d, key=lambda k: (len(k), k))


def _assert_maps(name, eng, amaps):
    g1, g2 = U.maps_of(eng)
    assert g1 == amaps.a1, f"{name}: map 1 differs: {_diff(g1, amaps.a1)}"
    assert g2 == amaps.a2, f"{name}: map 2 differs: {_diff(g2, amaps.a2)}"
    assert list(g1) == _map_order(g1) and list(g2) == _map_order(g2), f"{name}: entries not in the reference's map order"


def _diff(got, exp):
    keys = [k for k in set(got) | set(exp) if got.get(k) != exp.get(k)]
    return [(k, got.get(k), exp.get(k)) for k in sorted(keys)[:6]] + [f"{len(keys)} keys differ, sizes {len(got)} / {len(exp)}"]


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------
def _golden_families():
    out = []
    for name in golden_util.names():
        ac = golden_util.load(name)[2]["json"].get("adapter_cutting")
        if ac and (ac.get("read1_adapter_counts") or ac.get("read2_adapter_counts")):
            out.append(name)
    return out


GOLDEN = _golden_families()
# Families in which a string handed to a map holds a base that BaseCorrector edited (checked on the expected side).  pe_correction
# is not one and cannot be: without -a every string of a pair comes from trimByOverlapAnalysis and lies behind the overlapped
# region, and BaseCorrector only edits inside it - 0 of its 639 corrections fall into a string, 97 into the kept part of a
# mate that also hands a string over (asserted below).  With -a / --adapter_sequence_r2 a string can start inside the region:
# 5 of 904 corrections in pe_exotic_dedup_adapters, 6 of 3001 in pe_overrep_correction.
CORRECTED_IN_STRING = ("pe_exotic_dedup_adapters", "pe_overrep_correction")


def check_golden(name, make_engine):
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    umi = golden_util.umi_for(name)
    b1 = hostloop.parse_fastq(fq1)
    b2 = hostloop.parse_fastq(fq2, b1.seq.shape[1]) if fq2 is not None else None
    if b2 is not None and b2.seq.shape[1] != b1.seq.shape[1]:
        st = max(b1.seq.shape[1], b2.seq.shape[1])
        b1, b2 = hostloop.parse_fastq(fq1, st), hostloop.parse_fastq(fq2, st)
    paired = b2 is not None
    outs, amaps = hostloop.Outputs(paired, True, False, False), hostloop.AdapterMaps()
    n = b1.n if not paired else min(b1.n, b2.n)
    corrected_in_string = corrected_mate = 0
    eng = make_engine(params)
    try:
        for a in range(0, n, 1000):
            e = min(n, a + 1000)
            p1, p2 = b1.slice(a, e), (b2.slice(a, e) if paired else None)
            if paired:
                r1, r2, pr, corr = eng.process(p1.seq, p1.qual, p1.lens, p2.seq, p2.qual, p2.lens)
            else:
                r1, r2, pr, corr = eng.process(p1.seq, p1.qual, p1.lens)
            ev = eng.last_adapter_events
            hostloop.apply_results(params, p1, p2, r1, r2, pr, corr, outs, amaps, umi, adapter_events=ev)
            for c in corr:   # (expected side) a corrected base inside a string that is handed to a map
                rd, pos = int(c["read"]), int(c["pos"])
                rr = (r2 if rd & 1 else r1)[rd >> 1] if paired else r1[rd]
                ov = paired and (r1[rd >> 1]["flags"] & RF_OV)
                lo = int(rr["front"]) + int(rr["adapter_pos"])
                counted = (ov or (rr["flags"] & RF_A)) and rr["adapter_len"]
                corrected_mate += bool(counted)
                if counted and rr["adapter_pos"] >= 0 and lo <= pos < lo + int(rr["adapter_len"]):
                    corrected_in_string += 1
            seqs = [[b.seq[i, :int(b.lens[i])].tobytes() for i in range(b.n)] for b in ((p1, p2) if paired else (p1,))]
            U.census(eng, seqs[0], r1, seqs[1] if paired else None, r2, corrections=corr, events=ev if len(ev) else None)
        ctr = eng.counters()
        assert amaps.a1 or amaps.a2, f"{name}: the expected maps are empty"
        if name == "pe_correction":
            assert corrected_mate > 0, "pe_correction: no adapter string comes from a mate BaseCorrector edited"
        if name in CORRECTED_IN_STRING:
            assert corrected_in_string > 0, f"{name}: no adapter string holds a corrected base"
        _assert_maps(name, eng, amaps)
        cm = hostloop.AdapterMaps()
        cm.a1, cm.a2 = U.maps_of(eng)
        rep = refjson.build(ctr, eng.layout, params, cm)
    finally:
        eng.close()
    golden_util.check_against_golden(name, outs, rep, meta)


@pytest.mark.parametrize("name", GOLDEN)
def test_sim_census_goldens(name):
    check_golden(name, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_goldens")
@pytest.mark.parametrize("name", GOLDEN)
def test_gpu_census_goldens(name):
    check_golden(name, engines.gpu_engine)


# ---- 2. edges -----------------------------------------------------------------------------------------------------------
LINE = 70
READS = [b"ACGTTGCAAGCTTAGGCATCGATCGGATTACAGCTAGCTAGGATCCGATATCGCGCTTAAGGCCTAGTCAGT",
         b"TTTTTTTTTTTTGGGGGGGGGGGGACACACACACACACGTGTGTGTGTAAAAAAAAAAAACCCCCCCCCCTG",
         b"GATTACAGATTACAGATTACAGATTACAcgtnRYKMacgtGATTACAGATTACA..GATTACAGATTACAGA"]
READS = [r[:LINE] for r in READS]
assert all(len(r) == LINE for r in READS)


def _edge_mate(kind, i, mate):
    """(sequence line, record) of one mate of unit i"""
    seq = READS[(i + mate) % 3]
    front = (i * 7 + mate) % 4
    lens = (1, 2, 63, 64, 65, LINE)
    if kind == 0:     # nothing trimmed
        return seq, U.record(0, LINE)
    if kind == 1:     # a piece of the line: lengths 1, 2, 63, 64, 65 and the whole line
        ln = lens[(i // 8) % 6]
        fr = 0 if ln == LINE else min(front, LINE - ln)
        return seq, U.record(fr, 10, RF_A, (LINE - ln - fr) if ln < 63 else 0, ln)
    if kind == 2:     # adapter_pos < 0: the head of the adapter sequence (a length past its end is clamped)
        return seq, U.record(front, 5, RF_A, -3, (5, 33, 40)[(i // 8) % 3])
    if kind == 3:     # runs past the end of the line: clamped
        return seq, U.record(front, 5, RF_A, LINE - front - 9, 20)
    if kind == 4:     # starts at the end of the line, or past it: empty, ignored
        return seq, U.record(front, 5, RF_A, LINE - front + (i // 8) % 2 * 3, 6)
    if kind == 5:     # the flag without a length (what an --adapter_fasta trim alone leaves)
        return seq, U.record(front, 5, RF_A, 4, 0)
    raise AssertionError(kind)


def build_edges(n, paired, shift=0):
    rows = [[], []]
    seqs = [[], []]
    for i in range(n):
        k = i + n + shift
        pair_form = paired and k % 5 == 0
        for m in range(2 if paired else 1):
            kind = (k // (1 if m == 0 else 3)) % 6
            if pair_form and kind in (0, 5):
                kind = 1 if m else 4    # an empty read 1 string in a pair form still lets read 2's count
            s, r = _edge_mate(kind, k, m)
            if pair_form:
                r["flags"] |= RF_A | (RF_OV if m == 0 else 0)
            seqs[m].append(s)
            rows[m].append(r)
    return seqs[0], U.records(rows[0]), (seqs[1] if paired else None), (U.records(rows[1]) if paired else None)


EDGE_N = (1, 63, 64, 65, 255, 256, 257)
EDGES = {f"{'pe' if pe else 'se'}_{n}": (n, pe) for pe in (False, True) for n in EDGE_N}


@functools.lru_cache(maxsize=None)
def _edge_expected(name):
    n, paired = EDGES[name]
    amaps = hostloop.AdapterMaps()
    calls = [build_edges(n, paired, sh) for sh in ((0, 1, 2, 3, 4, 5, 6, 7) if n == 1 else (0,))]
    for c in calls:
        U.replay(_params(paired), amaps, *c)
    if n >= 63:   # the case holds what it was built for
        lens = {len(k) for k in amaps.a1}
        assert {1, 2, 63, 64, 65, LINE} <= lens and len(A1) in lens, sorted(lens)
    return calls, amaps


def check_edges(name, make_engine):
    n, paired = EDGES[name]
    calls, amaps = _edge_expected(name)
    eng = make_engine(_params(paired))
    try:
        for k, c in enumerate(calls):
            U.census(eng, *c, interleaved=paired and k % 2 == 1)
        _assert_maps(name, eng, amaps)
        if paired and n >= 63:   # two mates pointing into one text; and fastp_gpu_reset starts from empty maps
            eng.reset()
            assert U.maps_of(eng) == ({}, {})
            U.census(eng, *calls[0], interleaved=True)
            _assert_maps(name + " interleaved", eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(EDGES))
def test_sim_census_edges(name):
    check_edges(name, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_edges")
@pytest.mark.parametrize("name", list(EDGES))
def test_gpu_census_edges(name):
    check_edges(name, engines.gpu_engine)


FASTA = cases.FASTA_LIST


def _event(read, pos, ln, adapter):
    e = np.zeros(1, dtype=abi.ADAPTER_EVENT_DTYPE)
    e["read"], e["pos"], e["len"], e["adapter"] = read, pos, ln, adapter
    return e[0]


def build_fasta(paired):
    """units with --adapter_fasta events: one unit with three events given out of `adapter` order, an event with
    adapter_pos < 0 (the head of the FASTA entry), events of both mates, next to an ordinary trim of the same read"""
    n = 5
    seqs = [[READS[i % 3] for i in range(n)], [READS[(i + 1) % 3] for i in range(n)]]
    rows = [[U.record(0, LINE) for _ in range(n)] for _ in range(2)]
    rows[0][1] = U.record(2, 30, RF_A, 40, 12)      # -a's trim first, then the unit's events
    rows[0][2] = U.record(1, 30, RF_A, 0, 0)        # the flag from an --adapter_fasta trim alone
    key = (lambda u, m: 2 * u + m) if paired else (lambda u, m: u)
    ev = [_event(key(2, 0), 50, 9, 4), _event(key(2, 0), 30, 25, 0), _event(key(2, 0), 58, 30, 2),   # out of order; the last is clamped
          _event(key(1, 0), -2, 11, 3), _event(key(4, 0), 20, 8, 1), _event(key(0, 0), 69, 5, 1)]
    if paired:
        rows[1][3] = U.record(0, 30, RF_A, 33, 7)
        ev += [_event(key(2, 1), 10, 9, 3), _event(key(2, 1), 44, 6, 1), _event(key(3, 1), -1, 40, 0), _event(key(4, 1), 20, 8, 1)]
    ev = np.array(ev, dtype=abi.ADAPTER_EVENT_DTYPE)
    return seqs[0], U.records(rows[0]), (seqs[1] if paired else None), (U.records(rows[1]) if paired else None), ev


def check_fasta(paired, make_engine):
    s1, r1, s2, r2, ev = build_fasta(paired)
    p = _params(paired, fasta=FASTA)
    amaps = hostloop.AdapterMaps()
    for _ in range(2):
        U.replay(p, amaps, s1, r1, s2, r2, events=ev)
    assert FASTA[3][:11] in amaps.a1 and amaps.a1[READS[2][1 + 50:1 + 59]] == 2
    eng = make_engine(p)
    try:
        U.census(eng, s1, r1, s2, r2, events=ev)
        U.census(eng, s1, r1, s2, r2, events=ev[::-1].copy(), interleaved=paired)   # the list's order carries nothing
        _assert_maps("fasta", eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_sim_census_fasta_events(paired):
    check_fasta(paired, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_fasta_events")
@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_gpu_census_fasta_events(paired):
    check_fasta(paired, engines.gpu_engine)


def check_overflow(make_engine):
    """a list whose counter ran past its capacity: E_OVERFLOW, and the maps stay as they were"""
    s1, r1, s2, r2, ev = build_fasta(True)
    p = _params(True, fasta=FASTA)
    corr = np.zeros(4, dtype=abi.CORRECTION_DTYPE)
    corr["read"], corr["pos"], corr["base"], corr["qual"] = [2, 2, 3, 5], [41, 45, 3, 9], ord("N"), ord("#")
    amaps = hostloop.AdapterMaps()
    U.replay(p, amaps, s1, r1, s2, r2, corrections=corr, events=ev)
    assert any(b"N" in k for k in amaps.a1), "the corrected bases are inside a counted string"
    eng = make_engine(p)
    try:
        U.census(eng, s1, r1, s2, r2, corrections=corr, events=ev)
        _assert_maps("before", eng, amaps)
        assert U.census(eng, s1, r1, s2, r2, corrections=corr, events=ev, n_corr=5, check=False) == abi.E_OVERFLOW
        assert U.census(eng, s1, r1, s2, r2, corrections=corr, events=ev, n_events=len(ev) + 1, check=False) == abi.E_OVERFLOW
        assert U.census(eng, s1, r1, s2, r2, corrections=corr, events=ev, n_corr=1 << 30, corr_capacity=2, check=False) == abi.E_OVERFLOW
        _assert_maps("after the refused calls", eng, amaps)
    finally:
        eng.close()


def test_sim_census_list_overflow():
    check_overflow(engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_list_overflow")
def test_gpu_census_list_overflow():
    check_overflow(engines.gpu_engine)


# ---- 3. caps ------------------------------------------------------------------------------------------------------------
PAD = b"GATCCGTA" * 8


def _loaded_keys(count, salt):
    """`count` distinct keys: the index in base 4 over ten letters, then a tail"""
    out = {}
    for i in range(count):
        v, s = i, bytearray()
        for _ in range(10):
            s.append(b"ACGT"[v & 3])
            v >>= 2
        out[bytes(s) + (b"TGCA", b"GTAC")[salt]] = 1 + i % 3
    return out


class KeySource:
    """strings for the cap cases: ordinary and low-complexity keys that are new, keys the map already holds, length-1 strings and
    the len / 2 boundary of lowComplexity (diff = len / 2 - 1: low complexity; diff = len / 2: not)"""
    BOUNDARY = [b"AAAACGTT", b"AAACGTAA", b"CCCCCGTAA", b"CCCCGTACC", b"GGGT", b"GGTA", b"TT", b"TG", b"AAA", b"AAC"]

    def __init__(self, rng, loaded):
        self.rng, self.loaded, self.n_ord, self.n_lc = rng, list(loaded), 0, 0

    def ordinary(self):
        self.n_ord += 1
        v, s = self.n_ord, bytearray(b"TC")
        for _ in range(9):
            s += (b"AG", b"CT", b"GA", b"TC")[v & 3]
            v >>= 2
        return bytes(s) + bytes(self.rng.choice(list(b"ACGT"), size=int(self.rng.integers(0, 12))).astype(np.uint8))

    def low_complexity(self):
        self.n_lc += 1
        k, m = 2 + self.n_lc % 37, 2 + self.n_lc // 37
        return b"ACGT"[self.n_lc % 4:][:1] * k + b"CGTA"[self.n_lc % 4:][:1] * m

    def existing(self):
        return self.loaded[int(self.rng.integers(0, len(self.loaded)))]


def _unit(a1, a2, pair_form):
    """a pair whose reads start with the strings a1 / a2 (b'' = nothing trimmed)"""
    recs = []
    for a in (a1, a2):
        recs.append(U.record(0, 20, (RF_A if a or pair_form else 0), 0, len(a)))
    if pair_form:
        recs[0]["flags"] |= RF_OV
    return (a1 + PAD)[:max(len(a1), 40)], recs[0], (a2 + PAD)[:max(len(a2), 40)], recs[1]


def _calls_from_units(calls):
    out = []
    for units in calls:
        out.append(([u[0] for u in units], U.records([u[1] for u in units]), [u[2] for u in units], U.records([u[3] for u in units])))
    return out


def build_caps(base, first_call_new, seed):
    """load `base` keys per map, then three calls of PE units.  first_call_new None: call 1 is a few hundred mixed units and
    crosses the threshold inside the call.  first_call_new = k: call 1 brings exactly k new keys per map (and hits), so the
    map's size is base + k at the call boundary."""
    rng = np.random.default_rng(seed)
    load = [_loaded_keys(base, 0), _loaded_keys(base, 1)]
    src = [KeySource(rng, load[0]), KeySource(rng, load[1])]
    twice = [s.low_complexity() for s in src]      # low complexity, first seen just before the threshold, and again after it
    late = [s.low_complexity() for s in src]       # low complexity, first seen after it: refused every time
    bound = KeySource.BOUNDARY + [b"A", b"C", b"G", b"T"]

    def mixed(count, first):
        units = []
        for i in range(count):
            pick = []
            for m in (0, 1):
                x = rng.random()
                if first and i == 3 or i in (count // 2, count - 2):
                    a = twice[m]
                elif i in (count // 3, count - 5):
                    a = late[m]
                elif x < 0.30:
                    a = src[m].ordinary()
                elif x < 0.55:
                    a = src[m].low_complexity()
                elif x < 0.70:
                    a = src[m].existing()
                elif x < 0.85:
                    a = bound[int(rng.integers(0, len(bound)))]
                elif x < 0.93 and units:
                    a = units[int(rng.integers(0, len(units)))][0 if m == 0 else 2][:int(rng.integers(4, 30))]
                else:
                    a = b""
                pick.append(a)
            units.append(_unit(pick[0], pick[1], rng.random() < 0.5))
        return units

    calls = []
    if first_call_new is None:
        calls.append(mixed(300, True))
    else:
        units = []
        # (below 5000 every new key is admitted, low complexity or not; above it the new keys are ordinary ones)
        news = [[(src[m].low_complexity() if k % 2 and base < 5000 else src[m].ordinary()) for k in range(first_call_new)] for m in (0, 1)]
        for k in range(first_call_new):
            units.append(_unit(news[0][k], news[1][k], False))
            units.append(_unit(src[0].existing(), news[1][k], k % 2 == 0))
            units.append(_unit(news[0][k], src[1].existing(), True))
        calls.append(units)
    calls.append(mixed(257, first_call_new is not None))
    calls.append(mixed(200, False))
    return load, _calls_from_units(calls), twice, late


CAPS = {"5000_inside": (4990, None), "5000_at_boundary": (4990, 10), "5001_at_boundary": (4990, 11),
        "20000_inside": (19990, None), "20000_at_boundary": (19990, 10), "20001_at_boundary": (19990, 11)}


@functools.lru_cache(maxsize=None)
def _caps_expected(name):
    base, k = CAPS[name]
    load, calls, twice, late = build_caps(base, k, 40 + list(CAPS).index(name))
    amaps = hostloop.AdapterMaps()
    amaps.a1, amaps.a2 = dict(load[0]), dict(load[1])
    sizes = []
    p = _params(True)
    for c in calls:
        U.replay(p, amaps, *c)
        sizes.append((len(amaps.a1), len(amaps.a2)))
    # the case does what it was built for (all on the expected side)
    cap = 5000 if base < 5000 else 20000
    if k is not None:
        assert sizes[0] == (base + k, base + k), sizes
    else:
        assert sizes[0][0] > cap and sizes[0][1] > cap, sizes
    assert sizes[-1][0] > cap and sizes[-1][1] > cap, sizes
    if base < 5000:
        for m, mp in enumerate((amaps.a1, amaps.a2)):
            if k is None:
                assert mp.get(twice[m], 0) >= 2, "the low-complexity key seen before the threshold keeps counting after it"
            assert late[m] not in mp
        new_ordinary = [x for x in amaps.a1 if x not in load[0] and not hostloop.AdapterMaps._low_complexity(x)]
        assert len(amaps.a1) - base > 60 and len(new_ordinary) > 50, "ordinary keys keep being admitted past 5000"
    else:
        assert len(amaps.a1) == 20001 and len(amaps.a2) == 20001, sizes
    return load, calls, amaps


def check_caps(name, make_engine):
    load, calls, amaps = _caps_expected(name)
    eng = make_engine(_params(True))
    try:
        eng.load_adapter_counts(False, load[0])
        eng.load_adapter_counts(True, load[1])
        assert U.maps_of(eng) == (load[0], load[1])
        for c in calls:
            U.census(eng, *c)
        _assert_maps(name, eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(CAPS))
def test_sim_census_caps(name):
    check_caps(name, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_caps")
@pytest.mark.parametrize("name", list(CAPS))
def test_gpu_census_caps(name):
    check_caps(name, engines.gpu_engine)


# ---- 4. quirk #8 --------------------------------------------------------------------------------------------------------
QUIRK = {"low_complexity_past_5000": 5003, "anything_past_20000": 20001}


@functools.lru_cache(maxsize=None)
def _quirk_expected(name):
    base = QUIRK[name]
    load = [_loaded_keys(base, 0), _loaded_keys(base if base < 20000 else 5003, 1)]
    old2 = next(iter(load[1]))
    refused = (lambda i: b"A" * (5 + i) + b"C" * 3) if base < 20000 else (lambda i: b"TCAGCTGACTGA" + b"AG" * (1 + i))
    units = [_unit(refused(0), b"TGCATGCAGTCA", True),      # a1 refused, a2 a new key: not counted
             _unit(refused(1), old2, True),                 # a1 refused, a2 an existing key: not counted
             _unit(b"", b"GACTGACTTGCA", True),             # an empty a1: a2 is counted
             _unit(b"", old2, True),
             _unit(next(iter(load[0])), b"CATGCATGACGT", True),   # a1 an existing key: a2 is counted
             _unit(refused(0), b"TGCATGCAGTCA", False),     # the single forms of the first unit: read 2's string counts
             _unit(refused(2), b"GACTGACTTGCA", True)]
    calls = _calls_from_units([units, units[:3]])
    amaps, naive = hostloop.AdapterMaps(), hostloop.AdapterMaps()
    amaps.a1, amaps.a2 = dict(load[0]), dict(load[1])
    naive.a1, naive.a2 = dict(load[0]), dict(load[1])
    p = _params(True)
    for c in calls:
        U.replay(p, amaps, *c)
    for units_ in (units, units[:3]):   # the naive count: per map, every string on its own
        for s1, rr1, s2, rr2 in units_:
            naive.add_single(s1[:int(rr1["adapter_len"])], False)
            naive.add_single(s2[:int(rr2["adapter_len"])], True)
    assert naive.a1 == amaps.a1 and naive.a2 != amaps.a2, "the early return must change map 2 on this input"
    assert amaps.a2[old2] == load[1][old2] + 1 and amaps.a2[b"TGCATGCAGTCA"] == 1 and amaps.a2[b"GACTGACTTGCA"] == 2
    return load, calls, amaps


def check_quirk(name, make_engine):
    load, calls, amaps = _quirk_expected(name)
    eng = make_engine(_params(True))
    try:
        eng.load_adapter_counts(False, load[0])
        eng.load_adapter_counts(True, load[1])
        for c in calls:
            U.census(eng, *c)
        _assert_maps(name, eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(QUIRK))
def test_sim_census_pair_form_early_return(name):
    check_quirk(name, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_pair_form_early_return")
@pytest.mark.parametrize("name", list(QUIRK))
def test_gpu_census_pair_form_early_return(name):
    check_quirk(name, engines.gpu_engine)


# ---- 5. collisions ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _collision_expected():
    rng = np.random.default_rng(77)
    pool = [bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(1, 40))).astype(np.uint8)) for _ in range(60)]
    pool = list(dict.fromkeys(pool))[:40]
    assert len(pool) == 40
    picks = [pool[k % 40] for k in range(40)] + [pool[int(rng.integers(0, 40))] for _ in range(260)]   # 300 items, 40 distinct strings
    units = [_unit(picks[k], b"", False) for k in range(300)]
    calls = _calls_from_units([units[:180], units[180:]])
    amaps = hostloop.AdapterMaps()
    for c in calls:
        U.replay(_params(True), amaps, *c)
    assert len(amaps.a1) == 40 and sum(amaps.a1.values()) == 300
    return calls, amaps


COLLISIONS = ["40_strings_300_items", "5000_inside", "20000_inside"]


def check_collisions(name, make_engine, monkeypatch):
    monkeypatch.setenv("FASTP_GPU_DEBUG_CENSUS_HASH_BITS", "4")   # read when the context is created
    if name in CAPS:
        return check_caps(name, make_engine)
    calls, amaps = _collision_expected()
    eng = make_engine(_params(True))
    try:
        for c in calls:
            U.census(eng, *c)
        _assert_maps(name, eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("name", COLLISIONS)
def test_sim_census_hash_collisions(name, monkeypatch):
    check_collisions(name, engines.sim_engine, monkeypatch)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_hash_collisions")
@pytest.mark.parametrize("name", COLLISIONS)
def test_gpu_census_hash_collisions(name, monkeypatch):
    check_collisions(name, engines.gpu_engine, monkeypatch)


# ---- 6. the launch split ------------------------------------------------------------------------------------------------
SPLIT_UNITS = 2000
SPLITS = {"one_call": SPLIT_UNITS, "calls_of_1": 1, "calls_of_64": 64, "calls_of_257": 257}


@functools.lru_cache(maxsize=None)
def _split_expected():
    rng = np.random.default_rng(5)
    src = [KeySource(rng, [b"ACGTACGTAC"]), KeySource(rng, [b"TGCATGCATG"])]
    pools = [[s.ordinary() for _ in range(150)] + [s.low_complexity() for _ in range(100)] + KeySource.BOUNDARY for s in src]
    units = []
    for _ in range(SPLIT_UNITS):
        a = [pools[m][int(rng.integers(0, len(pools[m])))] if rng.random() < 0.8 else b"" for m in (0, 1)]
        units.append(_unit(a[0], a[1], rng.random() < 0.5))
    # start above 5000 so that refusals (and with them quirk #8) depend on what came before
    load = [_loaded_keys(5001, 0), _loaded_keys(4900, 1)]
    amaps = hostloop.AdapterMaps()
    amaps.a1, amaps.a2 = dict(load[0]), dict(load[1])
    U.replay(_params(True), amaps, *_calls_from_units([units])[0])
    assert len(amaps.a2) > 5001 and len(amaps.a1) > 5100
    return load, units, amaps


def check_split(name, make_engine):
    load, units, amaps = _split_expected()
    step = SPLITS[name]
    eng = make_engine(_params(True))
    try:
        eng.load_adapter_counts(False, load[0])
        eng.load_adapter_counts(True, load[1])
        for a in range(0, SPLIT_UNITS, step):
            U.census(eng, *_calls_from_units([units[a:a + step]])[0])
        _assert_maps(name, eng, amaps)
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(SPLITS))
def test_sim_census_launch_split(name):
    check_split(name, engines.sim_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_census_launch_split")
@pytest.mark.parametrize("name", list(SPLITS))
def test_gpu_census_launch_split(name):
    check_split(name, engines.gpu_engine)


# ---- 7. the file loop and the binding -----------------------------------------------------------------------------------
# (name, max_len the stream starts with): the last one starts below its late reads' length and re-plans
STREAM_GOLDENS = {"pe_adapter_seq": 152, "se_adapter_fasta": 152, "pe_correction": 152, "pe_late_long_reads": 100}


def _stream_files(tmp_path, fq1, fq2):
    import os
    paths = []
    for k, fq in enumerate((fq1, fq2)):
        paths.append(None)
        if fq is not None:
            paths[k] = os.path.join(str(tmp_path), f"in{k + 1}.fq")
            with open(paths[k], "wb") as f:
                f.write(fq)
    return paths


def check_stream(name, lib, tmp_path, chunk_bytes, monkeypatch):
    import streamlib
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=STREAM_GOLDENS[name], fq1=fq1, fq2=fq2)
    p1, p2 = _stream_files(tmp_path, fq1, fq2)
    umi = golden_util.umi_for(name)
    want = ("out1", "out2", "failed")
    off = streamlib.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=chunk_bytes, umi=umi)
    monkeypatch.setenv("FASTP_GPU_STREAM_ADAPTERS", "device")
    on = streamlib.run_files(lib, params, p1, p2, str(tmp_path), want=want, chunk_bytes=chunk_bytes, umi=umi)
    monkeypatch.delenv("FASTP_GPU_STREAM_ADAPTERS")
    assert off[3].a1 or off[3].a2, f"{name}: the host replay's maps are empty"
    assert on[3].a1 == off[3].a1 and on[3].a2 == off[3].a2, f"{name}: {_diff(on[3].a1, off[3].a1)} {_diff(on[3].a2, off[3].a2)}"
    assert on[0] == off[0] and np.array_equal(on[1], off[1]), f"{name}: outputs or counters differ with the census on"
    assert on[4].replans == off[4].replans and (on[4].replans >= 1) == (name == "pe_late_long_reads")
    assert on[4].chunks >= 2
    golden_util.check_against_golden(name, streamlib.as_outputs(on[0], fq2 is not None), streamlib.report(on[1], on[2], params, on[3]), meta)
    # the setter, the accessors and the filled host object
    outs, ctr, lay, amaps, st, info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=True, chunk_bytes=chunk_bytes, umi=umi)
    assert info["set_rc"] == 0 and info["entries"] == [amaps.a1, amaps.a2] == [off[3].a1, off[3].a2]
    assert all(list(d) == _map_order(d) for d in info["entries"])
    assert outs == {k: off[0][k] for k in outs}


@pytest.mark.parametrize("name", list(STREAM_GOLDENS))
def test_sim_stream_census_equals_host_replay(name, tmp_path, monkeypatch):
    from fastp_amd import engine
    check_stream(name, engine.load_library(engines.build_sim()), tmp_path, 60000, monkeypatch)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_census_equals_host_replay")
@pytest.mark.parametrize("name", list(STREAM_GOLDENS))
def test_gpu_stream_census_equals_host_replay(name, tmp_path, monkeypatch):
    from fastp_amd import engine
    check_stream(name, engine.load_library(), tmp_path, 100000, monkeypatch)


def check_stream_switches(lib, tmp_path, monkeypatch):
    import streamlib
    name = "pe_adapter_seq"
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    p1, p2 = _stream_files(tmp_path, fq1, fq2)
    ref = streamlib.run_files(lib, params, p1, p2, str(tmp_path), chunk_bytes=60000)[3]
    # without a host object the maps are still there; without the census they are not
    info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=True, chunk_bytes=60000, with_host=False)[5]
    assert info["entries"] == [ref.a1, ref.a2]
    info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=None, chunk_bytes=60000, with_host=False)[5]
    assert info["entries"] == [{}, {}]
    monkeypatch.setenv("FASTP_GPU_STREAM_ADAPTERS", "device")
    info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=None, chunk_bytes=60000, with_host=False)[5]
    assert info["entries"] == [ref.a1, ref.a2]          # the variable alone chose the device
    info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=False, chunk_bytes=60000)[5]
    assert info["entries"] == [ref.a1, ref.a2]          # the setter overrides it: the host object's maps
    monkeypatch.setenv("FASTP_GPU_STREAM_ADAPTERS", "1")
    assert U.stream_run(lib, params, p1, p2, str(tmp_path), chunk_bytes=60000, with_host=False)[5]["entries"] == [ref.a1, ref.a2]
    monkeypatch.setenv("FASTP_GPU_STREAM_ADAPTERS", "host")
    assert U.stream_run(lib, params, p1, p2, str(tmp_path), chunk_bytes=60000, with_host=False)[5]["entries"] == [{}, {}]
    monkeypatch.setenv("FASTP_GPU_STREAM_ADAPTERS", "bogus")
    with pytest.raises(streamlib.StreamError) as e:
        streamlib.run_files(lib, params, p1, p2, str(tmp_path), chunk_bytes=60000)
    assert e.value.code == abi.E_INVALID
    monkeypatch.delenv("FASTP_GPU_STREAM_ADAPTERS")
    info = U.stream_run(lib, params, p1, p2, str(tmp_path), census=True, chunk_bytes=60000, late_setter=True)[5]
    assert info["late_rc"] == abi.E_INVALID


def test_sim_stream_census_switches(tmp_path, monkeypatch):
    from fastp_amd import engine
    check_stream_switches(engine.load_library(engines.build_sim()), tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_stream_census_switches")
def test_gpu_stream_census_switches(tmp_path, monkeypatch):
    from fastp_amd import engine
    check_stream_switches(engine.load_library(), tmp_path, monkeypatch)


# the patched reference with the maps counted on the device: every value of fastp's own JSON equals fastp_ref -w 1's
CENSUS_ENV = {"FASTP_GPU_STREAM_ADAPTERS": "device"}
CENSUS_BINDING_CASES = ["pe_adapter_seq", "pe_adapter_fasta"]


@pytest.mark.parametrize("name", CENSUS_BINDING_CASES)
def test_patched_reference_census_on_emulator(name, tmp_path):
    import os

    import test_ref_binding as rb
    if not rb._ensure_built() or not os.path.exists(rb.REF_SIM):
        pytest.skip("reference binaries not built")
    rb._check(name, rb.REF_SIM, 600, tmp_path, seed=61, extra_env=CENSUS_ENV)


@pytest.mark.gpu
@pytest.mark.twin("test_patched_reference_census_on_emulator")
@pytest.mark.parametrize("name", CENSUS_BINDING_CASES)
def test_gpu_patched_reference_census(name, tmp_path):
    import os

    import test_ref_binding as rb
    if not (os.path.exists(rb.REF) and os.path.exists(rb.REF_GPU)):
        pytest.skip("oracle/_ref binaries did not travel to this box")
    rb._check(name, rb.REF_GPU, 3000, tmp_path, seed=62, threads=3, extra_env=CENSUS_ENV)


# ---- 8. the pipeline (torch tensors of a GPU: -m gpu only) --------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pe_adapter_seq", "se_adapter_cut"])
def test_gpu_pipeline_adapter_counts(name, tmp_path):
    import os

    from fastp_amd.pipeline import FastqPipeline
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    paired = fq2 is not None
    p1, p2 = _stream_files(tmp_path, fq1, fq2)
    # the golden's replay: the engine's records through hostloop.apply_results
    eng = engines.gpu_engine(params)
    try:
        import driver
        _, _, rep = driver.run_engine(eng, params, fq1, fq2, umi=golden_util.umi_for(name))
    finally:
        eng.close()
    files = {}
    for tag, census in (("plain", False), ("census", True)):
        out = {k: os.path.join(str(tmp_path), f"{tag}_{k}.fq") for k in ("out1", "out2", "failed")}
        pipe = FastqPipeline(params, device=0, chunk_bytes=1 << 16)
        try:
            st = pipe.run(p1, p2, out["out1"], out["out2"] if paired else None, failed_out=out["failed"], adapter_counts=census)
            maps = pipe.adapter_counts()
            ctr, lay = pipe.counters(), pipe.eng.layout
        finally:
            pipe.close()
        files[tag] = {k: open(v, "rb").read() for k, v in out.items() if paired or k != "out2"}
        if not census:
            assert maps.a1 == {} and maps.a2 == {}
    assert files["census"] == files["plain"]
    got = refjson.build(ctr, lay, params, maps)["adapter_cutting"]
    assert maps.a1 and got == rep["adapter_cutting"]
    assert got["read1_adapter_counts"] == meta["json"]["adapter_cutting"]["read1_adapter_counts"]
    if paired:
        assert got["read2_adapter_counts"] == meta["json"]["adapter_cutting"]["read2_adapter_counts"]
