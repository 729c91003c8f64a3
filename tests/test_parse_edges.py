"""The device FASTQ parser (fastp_gpu_parse_fastq: the parse_* kernels of fq_device.h) at the edges of its geometry: a lane owns
16 bytes, 256 lanes a 4096-byte sub-block, four sub-blocks a 16 384-byte workgroup, and the scan kernel's 1024 threads one
workgroup's count each up to 16 MiB of text.  Texts are built so that line terminators start on those borders (parse_util.place),
end at every offset inside a lane, are cut at every byte, and are padded with bytes that would change the answer if they were
read.  The reference is the byte loop of parse_util.reference (FastqReader::getLine / read and the packer, restated); every
comparison is exact, and the output buffers' guard records must stay as they were.  Each body runs on the emulator
(test_sim_*) and, with the same parameter ids, on the GPU (test_gpu_*)."""
import functools

import numpy as np
import pytest

import engines
import format_util
import parse_util
from fastp_amd import abi

EOLS = {"lf": b"\n", "crlf": b"\r\n", "cr": b"\r"}
LINES = ("name", "seq", "plus", "qual")
# where a terminator's first byte is put: the last byte of a lane / sub-block / workgroup, the first of the next, the one
# behind.  No two of one line kind can be three bytes apart, so each neighbourhood's three offsets go to three texts; with
# \r\n the x5 / x7 ones have the \r as the last byte of one unit and the \n as the first of the next
SEAMS = ([15, 4095, 16383, 32767, 49151], [16, 4096, 16384, 32768, 49152], [17, 4097, 16385, 32769])


class Backend:
    """an engine per max_len, made once; fresh 'device' memory per call"""

    def __init__(self, mk_engine, mem):
        self.mk_engine, self.mem, self.engines = mk_engine, mem, {}

    def engine(self, max_len):
        if max_len not in self.engines:
            self.engines[max_len] = self.mk_engine(abi.default_params(False, max_len))
        return self.engines[max_len]

    def close(self):
        for g in self.engines.values():
            g.close()


@pytest.fixture(scope="module")
def sim():
    b = Backend(engines.sim_engine, format_util.NumpyMem)
    yield b
    b.close()


@pytest.fixture(scope="module")
def gpu():
    b = Backend(engines.gpu_engine, format_util.TorchMem)
    yield b
    b.close()


_WANT = {}


def want_for(text, max_len, max_records, is_last=True):
    """parse_util.reference, computed once for the texts several tests share"""
    if len(text) < 16384:
        return parse_util.reference(text, max_len, max_records, is_last)
    key = (text, max_len, max_records, is_last)
    if key not in _WANT:
        _WANT[key] = parse_util.reference(text, max_len, max_records, is_last)
    return _WANT[key]


def check(b, text, max_len, max_records, is_last=True, fill=b"\n", want=None, what=""):
    """one call of the parser against the reference: every table, every info field, the exotic list, the return code, and
    nothing written behind the records"""
    eng = b.engine(max_len)
    want = want or want_for(text, max_len, max_records, is_last)
    info, seq, qual, lens, loff, llen, guard = parse_util.run(eng, b.mem(), text, max_len, max_records, is_last, fill, check=False)
    for k in parse_util.FIELDS:
        assert getattr(info, k) == getattr(want, k), f"{what}: {k} {getattr(info, k)}, the reference has {getattr(want, k)}"
    assert info.rc == (abi.E_INVALID if want.first_bad >= 0 else 0), f"{what}: rc {info.rc}"
    assert info.n_exotic == len(want.exotic) and np.array_equal(eng.parse_exotic(), want.exotic), f"{what}: exotic list"
    for name, got, exp in (("lens", lens, want.lens), ("line_off", loff, want.line_off), ("line_len", llen, want.line_len)):
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5]}: {got[bad[:5]]}, the reference has {exp[bad[:5]]}"
    rows = want.kinds != parse_util.BAD_ALPHABET   # (a record refused for its quality bytes: its rows are nobody's to read)
    for name, got, exp in (("seq", seq, want.seq), ("qual", qual, want.qual)):
        bad = np.nonzero((got != exp).any(axis=1) & rows)[0]
        assert len(bad) == 0, f"{what}: {name} rows differ at records {bad[:5]}"
    for name, g in zip(("seq", "qual", "lens", "line_off", "line_len"), guard):
        assert (g == 0xEE).all(), f"{what}: {name} written behind record {info.n_records}"
    return info


# ---- a. terminators on every seam -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_texts(eol, line, max_len):
    """three texts of 52 KB, 170 records or more; text k has the terminator of line kind `line` start at SEAMS[k]"""
    out = []
    for k, offs in enumerate(SEAMS):
        text, _ = parse_util.place(170, EOLS[eol], [(o, LINES.index(line)) for o in offs], max_len=max_len, seed=11 + k,
                                   min_bytes=52000)
        out.append(text)
    return out


SEAM_CASES = [(e, l, 150) for e in EOLS for l in LINES] + [("crlf", "seq", 37), ("crlf", "qual", 37)]
SEAM_IDS = [f"{e}-{l}-{m}" for (e, l, m) in SEAM_CASES]


def seams_case(b, eol, line, max_len):
    for k, text in enumerate(seam_texts(eol, line, max_len)):
        info = check(b, text, max_len, 600, True, b"\n", what=f"terminators at {SEAMS[k]}")
        assert info.first_bad == -1 and info.consumed == len(text) and info.n_records >= 170


@pytest.mark.parametrize("eol,line,max_len", SEAM_CASES, ids=SEAM_IDS)
def test_sim_parse_terminators_on_every_seam(sim, eol, line, max_len):
    seams_case(sim, eol, line, max_len)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_terminators_on_every_seam")
@pytest.mark.parametrize("eol,line,max_len", SEAM_CASES, ids=SEAM_IDS)
def test_gpu_parse_terminators_on_every_seam(gpu, eol, line, max_len):
    seams_case(gpu, eol, line, max_len)


# ---- b. text ends -----------------------------------------------------------------------------------------------------------
def end_texts(eol, m):
    """three ragged records; (what, text) for the text with its last terminator, without it, and - \\r\\n - cut behind the \\r,
    each placed so that its own length is m modulo 16"""
    e = EOLS[eol]
    out = []
    for what, extra in (("whole", len(e)), ("unterminated", 0)) + ((("cut in the terminator", 1),) if eol == "crlf" else ()):
        off = 1600 + (m - extra) % 16
        text, _ = parse_util.place(3, e, [(700, 3, 0), (off, 3, 2)], seed=3 + m)
        text = text[:off + extra]
        assert len(text) % 16 == m
        out.append((what, text))
    return out


def text_ends_case(b, eol, m):
    for what, text in end_texts(eol, m):
        for is_last in (True, False):
            want = want_for(text, 150, 8, is_last)
            if not is_last and (what != "whole" or eol == "cr"):   # the last record stays for the next chunk
                assert want.n_records == 2 and want.consumed == want.line_off[7] + want.line_len[7] + len(EOLS[eol])
            else:
                assert want.n_records == 3 and want.consumed == len(text)
            for fill in parse_util.FILLS:
                check(b, text, 150, 8, is_last, fill, want, f"{what}, is_last={is_last}, padded with {fill!r}")


END_CASES = [(e, m) for e in EOLS for m in (0, 1, 15)]
END_IDS = [f"{e}-{m}" for (e, m) in END_CASES]


@pytest.mark.parametrize("eol,m", END_CASES, ids=END_IDS)
def test_sim_parse_text_ends(sim, eol, m):
    text_ends_case(sim, eol, m)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_text_ends")
@pytest.mark.parametrize("eol,m", END_CASES, ids=END_IDS)
def test_gpu_parse_text_ends(gpu, eol, m):
    text_ends_case(gpu, eol, m)


def tiny_texts(eol):
    """less than 16 bytes: one record of length 0, one of length 1, with and without the last terminator; and no text"""
    e = EOLS[eol]
    whole = [e.join((b"@", b"", b"+", b"")) + e, e.join((b"@", b"N", b"+", b"~")) + e]
    return whole + [t[:-len(e)] for t in whole] + [b"@", e, b""]


def tiny_case(b, eol):
    for text in tiny_texts(eol):
        assert len(text) < 16
        for is_last in (True, False):
            for fill in parse_util.FILLS:
                info = check(b, text, 150, 3, is_last, fill, what=f"{text!r}, is_last={is_last}, padded with {fill!r}")
                assert info.n_records <= 1 and (text or info.n_lines == 0)


@pytest.mark.parametrize("eol", list(EOLS))
def test_sim_parse_tiny_texts(sim, eol):
    tiny_case(sim, eol)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_tiny_texts")
@pytest.mark.parametrize("eol", list(EOLS))
def test_gpu_parse_tiny_texts(gpu, eol):
    tiny_case(gpu, eol)


# ---- c. every cut -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_text(eol):
    """six records; the third ends at the first sub-block's border (the \\r of its last \\r\\n is byte 4095), the fourth follows"""
    text, _ = parse_util.place(6, EOLS[eol], [(1900, 3, 0), (3800, 3, 1), (4095, 3, 2)], seed=21)
    w = parse_util.reference(text, 150, None, True)
    assert w.n_records == 6 and w.first_bad == -1
    return text, w


def cuts_for(eol):
    text, w = cut_text(eol)
    if eol == "crlf":   # every byte of the third and fourth record
        return list(range(int(w.line_off[8]), int(w.line_off[16]) + 1))
    ends = [int(w.line_off[k] + w.line_len[k]) for k in range(8, 12)]   # the 40 cuts around each terminator of the third
    return sorted({c for t in ends for c in range(t - 20, t + 20)})


def every_cut_case(b, eol):
    text, _ = cut_text(eol)
    for k, cut in enumerate(cuts_for(eol)):
        fill = parse_util.FILLS[k % 4]
        first = check(b, text[:cut], 150, 8, False, fill, what=f"text[:{cut}]")
        rest = check(b, text[first.consumed:], 150, 8, True, fill, what=f"text[{first.consumed}:] after a cut at {cut}")
        assert first.n_records + rest.n_records == 6, f"cut at {cut}: {first.n_records} + {rest.n_records} records"


@pytest.mark.parametrize("eol", list(EOLS))
def test_sim_parse_every_cut(sim, eol):
    every_cut_case(sim, eol)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_every_cut")
@pytest.mark.parametrize("eol", list(EOLS))
def test_gpu_parse_every_cut(gpu, eol):
    every_cut_case(gpu, eol)


# ---- d. max_records ---------------------------------------------------------------------------------------------------------
CAPS = ["1", "4", "5", "64", "65", "all", "all-1"]


def max_records_case(b, cap):
    """the cap below, at and above the record count: term_pos / term_len hold 4 max_records + 1 entries, and terminators
    ranked behind them are counted, not stored"""
    text = seam_texts("crlf", "qual", 150)[0]
    full = want_for(text, 150, 600, True)
    n = full.n_records
    cap = n if cap == "all" else n - 1 if cap == "all-1" else int(cap)
    info = check(b, text, 150, cap, True, b"\n", what=f"max_records={cap}")
    assert info.n_records == cap and info.n_lines == full.n_lines
    assert info.consumed == (len(text) if cap == n else full.line_off[4 * cap])


@pytest.mark.parametrize("cap", CAPS)
def test_sim_parse_max_records(sim, cap):
    max_records_case(sim, cap)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_max_records")
@pytest.mark.parametrize("cap", CAPS)
def test_gpu_parse_max_records(gpu, cap):
    max_records_case(gpu, cap)


# ---- e. several offenders, several workgroups -------------------------------------------------------------------------------
N_MANY = 4000   # records of 150 bases: 250 workgroups of the packer (16 records each), 80 of the indexer


@functools.lru_cache(maxsize=None)
def many_lines():
    rng = np.random.default_rng(77)
    lines = []
    for r in range(N_MANY):
        s = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=150, p=[0.245, 0.245, 0.245, 0.245, 0.02]).tobytes()
        lines += [b"@many:%d 1:N:0" % r, s, b"+", rng.integers(33, 127, size=150).astype(np.uint8).tobytes()]
    return lines


def too_long(ls, r):   # max_len + 1
    ls[4 * r + 1] += b"A"
    ls[4 * r + 3] += b"I"


def bad_quality(byte):
    def f(ls, r):
        q = ls[4 * r + 3]
        ls[4 * r + 3] = q[:r % 150] + byte + q[r % 150 + 1:]
    return f


def name_without_at(ls, r):
    ls[4 * r] = b"X" + ls[4 * r][1:]


def blank_line(ls, r):   # an empty name line; every record behind it is malformed as well
    ls.insert(4 * r, b"")


def plus_without_plus(ls, r):
    ls[4 * r + 2] = b"-"


def empty_plus(ls, r):
    ls[4 * r + 2] = b""


def quality_shorter(ls, r):
    ls[4 * r + 3] = ls[4 * r + 3][:-1]


def quality_longer(ls, r):
    ls[4 * r + 3] += b"I"


# variant -> [(record, mutation)]; the mutations are applied from the last record to the first (blank_line moves what follows)
OFFENDERS = {
    "far_apart": [(3990, too_long), (2500, bad_quality(b" ")), (1033, name_without_at)],
    "rotated": [(3990, bad_quality(b"\x7f")), (2500, plus_without_plus), (1033, too_long)],
    "rotated_again": [(3990, quality_shorter), (2500, too_long), (1033, bad_quality(b"\xc1"))],
    "one_workgroup": [(1602, empty_plus), (1601, bad_quality(b"\x1f")), (1600, too_long)],
    "one_workgroup_reversed": [(1602, too_long), (1601, bad_quality(b"\x80")), (1600, quality_longer)],
    "blank_line": [(3990, too_long), (2500, bad_quality(b" ")), (1033, blank_line)],
    "plus_without_plus": [(3990, too_long), (2500, bad_quality(b" ")), (1033, plus_without_plus)],
    "empty_plus": [(3990, too_long), (2500, bad_quality(b" ")), (1033, empty_plus)],
    "quality_shorter": [(3990, too_long), (2500, bad_quality(b" ")), (1033, quality_shorter)],
    "quality_longer": [(3990, too_long), (2500, bad_quality(b" ")), (1033, quality_longer)],
    "too_long_alone": [(3990, too_long)],
}
# (smallest refused record, its kind) as the mutations were meant; first_bad_expected must say the same
MEANT = {"far_apart": (1033, 1), "rotated": (1033, 2), "rotated_again": (1033, 3), "one_workgroup": (1600, 2),
         "one_workgroup_reversed": (1600, 1), "blank_line": (1033, 1), "plus_without_plus": (1033, 1), "empty_plus": (1033, 1),
         "quality_shorter": (1033, 1), "quality_longer": (1033, 1), "too_long_alone": (3990, 2)}


@functools.lru_cache(maxsize=None)
def offender_text(variant):
    ls = list(many_lines())
    for r, mutate in sorted(OFFENDERS[variant], key=lambda x: -x[0]):
        mutate(ls, r)
    return b"\n".join(ls) + b"\n"


def offenders_case(b, variant):
    text = offender_text(variant)
    first_bad, kind, _ = parse_util.first_bad_expected(text, 150, N_MANY + 8, True)
    assert (first_bad, kind) == MEANT[variant]
    info = check(b, text, 150, N_MANY + 8, True, b"@", what=variant)
    assert (info.first_bad, info.bad_kind) == (first_bad, kind)
    if variant in ("far_apart", "too_long_alone"):   # reads of exactly max_len pass, the one of max_len + 1 is reported
        assert info.max_seq_len == 151 and info.n_records == N_MANY


@pytest.mark.parametrize("variant", list(OFFENDERS))
def test_sim_parse_smallest_offender_wins(sim, variant):
    offenders_case(sim, variant)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_smallest_offender_wins")
@pytest.mark.parametrize("variant", list(OFFENDERS))
def test_gpu_parse_smallest_offender_wins(gpu, variant):
    """on the GPU the packer's workgroups run at once: atomic min on the (record, kind) word decides, whoever comes first"""
    offenders_case(gpu, variant)


@functools.lru_cache(maxsize=None)
def exotic_text():
    """300 records with letters outside ACGTN - lower case, IUPAC codes, '.' - one in every workgroup of the packer, record 0,
    two of one wavefront (records 8 and 9), the rest drawn; no record refused"""
    rng = np.random.default_rng(78)
    ls = list(many_lines())
    recs = {0, 8, 9} | {16 * w + (7 * w) % 16 for w in range(N_MANY // 16)}
    while len(recs) < 300:
        recs.add(int(rng.integers(0, N_MANY)))
    letters = np.frombuffer(b"acgtnRYKMSWBDHVryu.", dtype=np.uint8)
    for r in sorted(recs):
        s = np.frombuffer(ls[4 * r + 1], dtype=np.uint8).copy()
        at = {0: [0], 8: [149], 9: [3, 4]}.get(r, rng.integers(0, 150, size=int(rng.integers(1, 4))))
        s[at] = rng.choice(letters, size=len(at))
        ls[4 * r + 1] = s.tobytes()
    return b"\n".join(ls) + b"\n", sorted(recs)


def exotic_case(b):
    text, recs = exotic_text()
    first_bad, kind, exotic = parse_util.first_bad_expected(text, 150, N_MANY, True)
    assert (first_bad, kind) == (-1, 0) and exotic == recs and len(recs) == 300
    info = check(b, text, 150, N_MANY, True, b"\x7f", what="300 exotic records")
    assert info.n_exotic == 300 and list(b.engine(150).parse_exotic()) == recs


def test_sim_parse_exotic_records_of_every_workgroup(sim):
    exotic_case(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_exotic_records_of_every_workgroup")
def test_gpu_parse_exotic_records_of_every_workgroup(gpu):
    """on the GPU the list is filled by atomic adds from 250 workgroups in no particular order; the host sorts it"""
    exotic_case(gpu)


# ---- f. more than 1024 scan blocks ------------------------------------------------------------------------------------------
BIG_BYTES = (16 << 20) + (40 << 10)


def scan_blocks_case(b):
    """16 MiB + 40 KiB of text: 1027 workgroups' counts for the scan kernel's 1024 threads, so each thread sums and
    prefixes two (per = 2) and the last threads' runs are clamped to the block count.  Up to 16 MiB - the largest chunk the
    stream loop makes - per is 1; the scan kernel's thread count is fixed by the launch, so nothing smaller reaches the
    branch.  The reference is parse_util.reference_np (held equal to the byte loop by test_reference_np_equals_reference)."""
    text = parse_util.big_text(BIG_BYTES, b"\r\n", 250, seed=5)
    assert (len(text) + 16383) // 16384 == 1027
    want = parse_util.reference_np(text, 250, None, True, b.engine(250).lib)
    assert want.n_records > 30000 and want.first_bad == -1 and want.lens.max() == 250 and want.lens.min() == 0
    info = check(b, text, 250, want.n_records + 16, True, b"\n", want, "16 MiB + 40 KiB")
    assert info.consumed == len(text)


def test_sim_parse_more_than_1024_scan_blocks(sim):
    """the emulator goes through the 16 MiB in about 12 s, so the case has its twin after all"""
    scan_blocks_case(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_parse_more_than_1024_scan_blocks")
def test_gpu_parse_more_than_1024_scan_blocks(gpu):
    scan_blocks_case(gpu)


# ---- g. argument refusals (host code) ---------------------------------------------------------------------------------------
def test_sim_parse_argument_refusals(sim):
    """refused with E_INVALID before anything is launched: text not 16-byte aligned, 4 GiB, a negative capacity; no text and
    no capacity are fine and report no records - and no exotic records left over from the call before"""
    eng, mem = sim.engine(150), sim.mem()
    text = b"@r\nACGT\n+\nIIII\n"
    t = mem.upload(b"\0" * 8 + text, 48)
    outs = [mem.alloc(8 * w, 0xEE) for w in (abi.seq_stride(150), abi.qual_stride(150), 2, 16, 16)]
    ptrs = [mem.ptr(o) for o in outs]
    assert mem.ptr(t) % 16 == 0
    for nbytes, cap, ptr in ((len(text), 4, mem.ptr(t) + 8), (1 << 32, 4, mem.ptr(t)), (len(text), -1, mem.ptr(t))):
        info = eng.parse_fastq(ptr, nbytes, True, cap, *ptrs, check=False)
        assert info.rc == abi.E_INVALID and info.n_records == 0, (nbytes, cap)
    exotic = b"@r\nACRT\n+\nIIII\n"
    info, *_ = parse_util.run(eng, mem, exotic, 150, 4)
    assert info.n_exotic == 1 and list(eng.parse_exotic()) == [0]
    for nbytes, cap in ((0, 4), (len(text), 0)):
        info = eng.parse_fastq(mem.ptr(t) + 16, nbytes, True, cap, *ptrs, check=False)
        assert info.rc == 0 and info.first_bad == -1 and info.n_records == 0 and info.consumed == 0 and info.n_exotic == 0
        assert len(eng.parse_exotic()) == 0, "the exotic list of an earlier call"
    assert all((np.frombuffer(mem.download(o), dtype=np.uint8) == 0xEE).all() for o in outs)


# ---- the vectorised reference -----------------------------------------------------------------------------------------------
def small_texts():
    """(what, text, max_len, max_records, is_last) of every text above that the byte loop can go through"""
    for (eol, line, max_len) in SEAM_CASES:
        for k, text in enumerate(seam_texts(eol, line, max_len)):
            yield f"seams {eol} {line} {max_len} #{k}", text, max_len, 600, True
    for (eol, m) in END_CASES:
        for what, text in end_texts(eol, m):
            for is_last in (True, False):
                yield f"end {eol} {m} {what}", text, 150, 8, is_last
    for eol in EOLS:
        for text in tiny_texts(eol):
            for is_last in (True, False):
                yield f"tiny {text!r}", text, 150, 3, is_last
        text, _ = cut_text(eol)
        for cut in cuts_for(eol)[::7]:
            yield f"cut {eol} {cut}", text[:cut], 150, 8, False
            yield f"cut {eol} {cut} rest", text[cut:], 150, 8, True
    for cap in (1, 4, 5, 64, 65):
        yield f"max_records {cap}", seam_texts("crlf", "qual", 150)[0], 150, cap, True
    for variant in OFFENDERS:
        yield f"offenders {variant}", offender_text(variant), 150, N_MANY + 8, True
    yield "exotic", exotic_text()[0], 150, N_MANY, True


def test_reference_np_equals_reference():
    """what entitles the 16 MiB case to parse_util.reference_np: on every other text of this file it equals the byte loop,
    field by field"""
    lib = engines.sim_engine(abi.default_params(False, 150)).lib
    n = 0
    for what, text, max_len, cap, is_last in small_texts():
        diff = parse_util.same_reference(want_for(text, max_len, cap, is_last), parse_util.reference_np(text, max_len, cap, is_last, lib))
        assert diff is None, f"{what}: {diff}"
        n += 1
    assert n > 300
    text = parse_util.big_text(300000, b"\r\n", 250, seed=6)   # the builder of the 16 MiB case, at a size the loop can do
    a, b = parse_util.reference(text, 250, None, True), parse_util.reference_np(text, 250, None, True, lib)
    assert parse_util.same_reference(a, b) is None and a.first_bad == -1 and a.n_records > 500 and len(a.exotic) == 0
