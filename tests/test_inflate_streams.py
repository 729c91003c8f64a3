"""Both device inflate kernels (fq_inflate_wave.h: one wavefront per BGZF block; fq_inflate.h: one lane per block) and the
two host inflaters (fq_gunzip.h, fq_pgunzip.h) on hand-built DEFLATE streams (tests/deflate_build.py): the part of RFC 1951
that zlib never writes and FASTQ text never needs - every overlapping (distance, length) pair, distance symbols 28/29,
15-bit codes, one-symbol and absent distance codes, 1-bit literal codes, the repeat codes of the dynamic header at their
extremes, block chains with stored blocks against the staging buffers, every payload alignment - and the streams a decoder
has to refuse.  zlib is the reference: it has decoded (or refused) every stream before a kernel sees it.

Each emulator test has a `-m gpu` twin: the same case function on the device, at the device's size (SCALE)."""
import functools
import zlib

import numpy as np
import pytest

import deflate_build as db
import engines
import format_util
import synth
import test_hostsim_parity as hs
from deflate_build import Deflate, Raw
from fastp_amd import abi
from test_gunzip import MODES, _gunzip, lib  # noqa: F401  (lib: the module-scoped fixture over MODES)

VARIANTS = ["wave", "lane"]
VALID = ["match_grid", "symbol_extremes", "odd_codes", "block_chains", "many_members"]
# what differs between the emulator and the device: the distances of match_grid (the wave kernel costs seconds per MB on
# the emulator) and the member count of many_members (the emulator has three "CUs": 128 members are > 4 per workgroup there,
# as 2100 are for the device's 512 workgroups)
SCALE = {"sim": {"grid_d": 40, "members": 128}, "gpu": {"grid_d": 300, "members": 2100}}


def _one(build):
    """a member from a function that fills a Deflate"""
    d = Deflate()
    build(d)
    return d.finish()


# ---- match_grid ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def match_grid(dmax):
    """fixed-code members: 300 literals, then a match for every (distance 1..dmax, length 3..258) - inf_copy's three regimes
    (distance < 8, < 32, >= 32) and the wave kernel's two (distance < length: the remainder by reciprocal; >= length)"""
    head = [i % 251 for i in range(300)]
    members, tokens, size = [], list(head), 300
    for dist in range(1, dmax + 1):
        for ln in range(3, 259):
            if size + ln > 60000:
                members.append(_one(lambda d: d.fixed(tokens, True)))
                tokens, size = list(head), 300
            tokens.append((ln, dist))
            size += ln
    members.append(_one(lambda d: d.fixed(tokens, True)))
    return members


# ---- symbol_extremes -------------------------------------------------------------------------------------------------
# symbols 257, 264, 265, 268, 284, 285 at their smallest and largest length (284: extra 0 and 30; its extra 31 is in odd_codes)
LEN_EXTREMES = [3, 10, 11, 12, 17, 18, 227, 257, 258]
assert [db.len_symbol(n)[0] for n in LEN_EXTREMES] == [257, 264, 265, 265, 268, 268, 284, 284, 285]


@functools.lru_cache(maxsize=None)
def symbol_extremes():
    """one text, two dynamic encodings with complete 15-bit ladders over all 286 literal/length and all 30 distance symbols
    (HLIT and HDIST at their maximum, HCLEN 19): 32768 random literals, then every distance symbol 0..29 at its smallest and
    largest distance (1 ... 32768) with the smallest and largest length of symbols 257, 264, 265, 268, 284 (227 and 257 =
    extra 0 and 30) and 285.  The full product would be 81 548 bytes; a member holds 65536.  So the lengths up to 18 meet
    both distances of every symbol, and 227 / 257 / 258 meet one distance of every symbol each: 227 and 258 the smallest of
    the even symbols and the largest of the odd ones, 257 the other way round."""
    rng = np.random.default_rng(1951)
    tokens = [int(x) for x in rng.integers(0, 256, size=32768)]
    for ds in range(30):
        lo, hi = db.DIST_BASE[ds], db.DIST_BASE[ds] + (1 << db.DIST_EXTRA[ds]) - 1
        for ln in LEN_EXTREMES:
            if ln < 227:
                tokens += [(ln, lo), (ln, hi)]
            else:
                tokens.append((ln, (lo, hi)[(ds & 1) ^ (ln == 257)]))
    ll, dl = db.ladder(286), db.ladder(30)
    members = []
    for lit, dist in ((ll, dl), (ll[::-1], dl[::-1])):     # 15-bit codes on the length / high distance symbols; on the literals
        members.append(_one(lambda d: d.dynamic(tokens, True, lit, dist, cl_symbols=db.compact_cl(lit + dist))))
    assert members[0][1] == members[1][1] and 32768 < len(members[0][1]) <= 65536
    return members


# ---- odd_codes -------------------------------------------------------------------------------------------------------
def _wide_tokens():
    """48-bit tokens (15-bit length code, 5 extra bits, 15-bit distance code, 13 extra bits) at every bit offset of the
    wave kernel's 64-lane speculation step, the last lanes included: 1-bit literals shift them bit by bit"""
    lit = db.ladder(286)
    lit[0], lit[65] = lit[65], lit[0]                     # 'A' is the 1-bit code; symbols 256 and 284 keep 15 bits
    dist = db.ladder(30)
    assert lit[65] == 1 and lit[284] == 15 and dist[29] == 15
    tokens = [65] * 33000
    for j in range(100):
        tokens += [65] * j + [Raw(284, j % 32, 29, 8191 - 7 * j)]
    d = Deflate()
    d.token_bits = []
    d.dynamic(tokens, True, lit, dist, cl_symbols=db.compact_cl(lit + dist))
    # the wave kernel's steps: one starts at a token, takes the tokens that start in its 64 bits, the next starts behind them
    step, seen = d.token_bits[0][0], set()
    for at, nbits in d.token_bits:
        if at >= step + 64:
            step = at
        if nbits == 48:
            seen.add(at - step)
    assert set(range(56, 64)) <= seen and len(seen) > 48, sorted(seen)
    return d.finish()


def _repeat_codes():
    """the code-length symbols at their extremes: 18 with extra 127 and 0, 17 with extra 7 and 0, 16 with extra 3 and 0"""
    cl = [(18, 127), (18, 0), (17, 7), (17, 0), (3, 0), (16, 3), (6, 0), (16, 0), (18, 72), (5, 0), (6, 0), (6, 0), (1, 0), (1, 0)]
    lens = db.expand_cl(cl)
    assert len(lens) == 259 + 2 and [i for i, v in enumerate(lens) if v] == list(range(162, 173)) + [256, 257, 258, 259, 260]
    tokens = list(range(162, 173)) * 3 + [(3, 1), (4, 2), (3, 2), (4, 1)] + [170, 171]
    return _one(lambda d: d.dynamic(tokens, True, lens[:259], lens[259:], cl_symbols=cl))


def _run_across_the_border():
    """one 18 covers the last 25 literal/length lengths and the first 10 distance lengths; and a member where a 16 repeats
    the end-of-block symbol's length into the distance code"""
    used = [65, 67, 71, 84, 256, 257, 258, 259, 260]
    lit = db.balanced(286, used)
    dist = [0] * 10 + [1, 1]
    cl = db.plain_cl(lit[:261]) + [(18, 24)] + [(1, 0), (1, 0)]
    tokens = [65, 67, 71, 84] * 20 + [(3, 33), (4, 49), (5, 64), (6, 34)]
    a = _one(lambda d: d.dynamic(tokens, True, lit, dist, cl_symbols=cl))
    lit2 = [0] * 258
    lit2[65], lit2[67], lit2[256], lit2[257] = 1, 3, 3, 2
    cl2 = db.compact_cl(lit2[:257]) + [(2, 0), (16, 1)]
    b = _one(lambda d: d.dynamic([65, 67, 65, (3, 1), (3, 2), (3, 3), (3, 4), 67], True, lit2, [2, 2, 2, 2], cl_symbols=cl2))
    return [a, b]


def _sixteen_after_zeros():
    """a 16 directly behind a zero run repeats zero"""
    lit = db.balanced(257, [10, 65, 66, 256])
    cl = [(17, 0), (16, 0), (16, 1)] + db.plain_cl(lit[10:]) + [(0, 0)]
    assert db.expand_cl(cl) == lit + [0]
    return _one(lambda d: d.dynamic([65, 66, 10] * 7, True, lit, [0], cl_symbols=cl))


@functools.lru_cache(maxsize=None)
def odd_codes():
    out = []
    acgt = [65, 67, 71, 84, 256, 257, 258, 264]
    text = [65, 67, 71, 84, 84, 71] * 5
    # a distance code with a single 1-bit symbol (an incomplete code, the one RFC 1951 allows): symbol 4 = distances 5, 6
    out.append(_one(lambda d: d.dynamic(text + [(3, 5), (4, 6), (10, 5), (3, 6)], True, db.balanced(265, acgt), [0, 0, 0, 0, 1])))
    # HDIST = 0 and that one length 0: no distance code at all, literals only
    out.append(_one(lambda d: d.dynamic(text, True, db.balanced(265, acgt), [0])))
    # a 1-bit literal code: 64 tokens per speculation step of the wave kernel
    one_bit = [0] * 257
    one_bit[65] = one_bit[256] = 1
    out.append(_one(lambda d: d.dynamic([65] * 2000, True, one_bit, [0], cl_symbols=db.compact_cl(one_bit + [0]))))
    out.append(_wide_tokens())
    # length 258 as symbol 284 with extra 31 (no compressor writes it; zlib and RFC 1951's table accept it)
    out.append(_one(lambda d: d.fixed(list(range(40)) + [Raw(284, 31, 0, 0), Raw(284, 31, 9, 7), Raw(284, 31, 16, 127), (258, 300)], True)))
    # HLIT = 257 (no length symbol) and HLIT = 286
    out.append(_one(lambda d: d.dynamic(text, True, db.balanced(257, [65, 67, 71, 84, 256]), [0])))
    out.append(_one(lambda d: d.dynamic(text + [(258, 2), (3, 1), (258, 1)], True, db.balanced(286, [65, 67, 71, 84, 256, 257, 285]), [1, 1] + [0] * 28)))
    # HCLEN: 19 code-length code lengths (the lengths 1 and 15 come last in the order), and the fewest a block can have - with
    # four (16, 17, 18, 0) every length would be zero and the end-of-block symbol without a code: INVALID's "hclen_4"
    lad = [0] * 258
    for s, ln in zip(list(range(48, 62)) + [256, 257], db.ladder(16)):
        lad[s] = ln
    d = Deflate()
    d.dynamic(list(range(48, 62)) * 2 + [(3, 1)], True, lad, [1])
    out.append(d.finish())
    eights = [8] * 255 + [0, 8]
    cl = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0), (0, 0), (8, 0), (0, 0)]
    d = Deflate()
    d.dynamic(list(range(255)), True, eights, [0], cl_symbols=cl, hclen=5)
    out.append(d.finish())
    d = Deflate()
    d.dynamic(text, True, db.balanced(257, [65, 67, 71, 84, 256]), [0], hclen=19)
    out.append(d.finish())
    out.append(_repeat_codes())
    out += _run_across_the_border()
    out.append(_sixteen_after_zeros())
    return out


# ---- block_chains ----------------------------------------------------------------------------------------------------
STORED_LENGTHS = [2040, 2048, 2049, 4090, 4096, 4100, 6143, 8192, 12288, 40000]    # around the wave kernel's 2 KiB halves / 4 KiB ring


@functools.lru_cache(maxsize=None)
def block_chains():
    rng = np.random.default_rng(77)
    out = []
    offsets = set()
    for k in range(8):
        # 9-bit literals: the empty stored block's header follows bit offset (3 + 9k + 7) mod 8 = every offset
        data = rng.integers(0, 256, size=256 * (8 + k), dtype=np.uint8).tobytes()
        d = Deflate()
        d.fixed([200 + j for j in range(k)], False)
        d.stored(b"", False)
        offsets.add(d.header_bits[-1] % 8)
        d.stored(data, False)
        d.fixed([(258, len(data)), (3, 1), (100, 2047 + k), (17, len(data) + 258 + 3 + 100)] + [7, 8, 9], False)
        for _ in range(5):
            d.fixed([], False)
        d.dynamic([66], False, db.balanced(257, [66, 256]), [0])
        d.fixed([], True)
        out.append(d.finish())
    assert offsets == set(range(8))
    out.append(_one(lambda d: d.fixed([], True)))               # the whole payload is one empty fixed block
    out.append(_one(lambda d: d.stored(b"", True)))             # ... one empty stored block
    assert out[-1][1] == b"" and out[-2][1] == b""
    for n in STORED_LENGTHS:
        for lead in (0, 3):
            data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            d = Deflate()
            d.fixed([33, 34, 35][:lead], False)
            d.stored(data, False)
            d.fixed([(200, min(n, 32768)), (258, 1)], False)
            d.stored(b"final", True)
            out.append(d.finish())
    # stored headers around the end of the lane kernel's first 128-byte stage (n 8-bit literals = n bytes and 10 bits)
    for n in range(116, 135):
        d = Deflate()
        d.fixed([j % 144 for j in range(n)], False)
        d.stored(bytes(range(40)), False)
        d.fixed([(10, 40), (3, n + 50)], True)
        out.append(d.finish())
    # a member of exactly 65536 bytes of text
    out.append(_one(lambda d: d.fixed([1, 2, 3, 4] + [(258, 4)] * 254, True)))
    assert len(out[-1][1]) == 65536
    return out


EMPTY = None


def _empty():
    global EMPTY
    if EMPTY is None:
        EMPTY = _one(lambda d: d.fixed([], True))
    return EMPTY


@functools.lru_cache(maxsize=None)
def many_members(at_least):
    """odd_codes and block_chains with empty members between them, again and again: a workgroup of the wave kernel takes
    several blocks of different kinds one after the other (its LDS state is reused), the 64 lanes of the lane kernel hold
    blocks of different kinds side by side"""
    round_ = []
    for m in odd_codes() + block_chains():
        round_ += [m, _empty()]
    out = []
    while len(out) < at_least:
        out += round_
    return out


@functools.lru_cache(maxsize=None)
def _tiny_kinds():
    kinds = [m for m in odd_codes() + block_chains() if len(m[1]) < 300]
    assert len(kinds) >= 10
    stored = [_one(lambda d: d.stored(bytes(range(n)), True)) for n in range(37)]
    return kinds, stored


def _tiny_members(n):
    """n members of a few bytes each: stored ones (a wavefront of the emulator builds no table for them, which keeps the
    6144 blocks of the wave kernel within seconds there), every 64th one of the small Huffman members of the families"""
    kinds, stored = _tiny_kinds()
    return [kinds[(k >> 6) % len(kinds)] if k % 64 == 0 else stored[k % 37] for k in range(n)]


def valid_members(family, scale):
    s = SCALE[scale]
    return {"match_grid": lambda: match_grid(s["grid_d"]), "symbol_extremes": symbol_extremes, "odd_codes": odd_codes,
            "block_chains": block_chains, "many_members": lambda: many_members(s["members"])}[family]()


def _clear(mem):
    if hasattr(mem, "keep"):
        mem.keep.clear()


def _valid_case(mk_engine, mem, family, scale):
    members = valid_members(family, scale)
    comp, offs = db.bgzf_file(members)
    want = b"".join(text for _, text in members)
    if len(members) >= 16:
        assert {o % 16 for o in offs} == set(range(16))        # every payload alignment
    if family == "many_members":
        assert len(members) >= SCALE[scale]["members"]
    g = mk_engine(abi.default_params(False, 150))
    for check_crc in (True, False) if family == "match_grid" else (True,):
        info, rc, bad, got = hs._inflate(g, mem, comp, check_crc=check_crc, check=False)
        assert info.rc == 0 and rc == 0 and bad == -1, f"{family}: rc {rc}, first bad member {bad} (check_crc={check_crc})"
        assert info.n_blocks == len(members) and info.consumed == len(comp) and info.out_bytes == len(want)
        if got != want:
            at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
            k = max(j for j in range(len(members)) if sum(len(t) for _, t in members[:j]) <= at)
            raise AssertionError(f"{family}: the text differs at byte {at} (member {k}, check_crc={check_crc})")
        _clear(mem)
    g.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("family", VALID)
def test_sim_inflate_hand_built_streams(family, variant, monkeypatch):
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    _valid_case(engines.sim_engine, format_util.NumpyMem(), family, "sim")


@pytest.mark.gpu
@pytest.mark.twin("test_sim_inflate_hand_built_streams")
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("family", VALID)
def test_gpu_inflate_hand_built_streams(family, variant, monkeypatch):
    """match_grid: about 10 MB of text in about 170 members; many_members: 2100 members and more, over four per workgroup of
    the wave kernel's launch"""
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    _valid_case(engines.gpu_engine, format_util.TorchMem(), family, "gpu")


# ---- selection by size -----------------------------------------------------------------------------------------------
def _selection_case(mk_engine, mem, n_blocks):
    members = _tiny_members(n_blocks)
    comp, _ = db.bgzf_file(members)
    want = b"".join(text for _, text in members)
    g = mk_engine(abi.default_params(False, 150))
    info, rc, bad, got = hs._inflate(g, mem, comp, check=False)
    g.close()
    assert info.rc == 0 and rc == 0 and bad == -1 and info.n_blocks == n_blocks and info.consumed == len(comp)
    assert got == want


@pytest.mark.parametrize("n_blocks", [6144, 6145])
def test_sim_inflate_kernel_selected_by_size(n_blocks, monkeypatch, tmp_path):
    """FASTP_GPU_INFLATE unset: up to 6144 blocks the wave kernel, beyond them the lane kernel; both decode.  The emulator's
    launch trace (tests/test_launch_trace.py) names the kernel that ran."""
    monkeypatch.delenv("FASTP_GPU_INFLATE", raising=False)
    trace = tmp_path / "trace.txt"
    monkeypatch.setenv("FASTP_SIM_TRACE", str(trace))
    _selection_case(engines.sim_engine, format_util.NumpyMem(), n_blocks)
    launches = [ln.split()[1] for ln in trace.read_text().splitlines() if ln.startswith("launch fq_inflate")]
    assert launches == ["fq_inflate_wave_kernel" if n_blocks <= 6144 else "fq_inflate_kernel"]


@pytest.mark.gpu
@pytest.mark.twin("test_sim_inflate_kernel_selected_by_size")
@pytest.mark.parametrize("n_blocks", [6144, 6145])
def test_gpu_inflate_kernel_selected_by_size(n_blocks, monkeypatch):
    """(the device keeps no launch trace: the result alone)"""
    monkeypatch.delenv("FASTP_GPU_INFLATE", raising=False)
    _selection_case(engines.gpu_engine, format_util.TorchMem(), n_blocks)


# ---- streams that must be refused ------------------------------------------------------------------------------------
def _three(lit_a=65, lit_b=66):
    return db.balanced(257, [lit_a, lit_b, 256])       # lengths 1, 2, 2


def _invalid_streams():
    def one(build):
        d = Deflate()
        build(d)
        return d.finish_invalid()

    def btype3(d):
        d.fixed([1, 2, 3], False)
        d.w.bits(1, 1)
        d.w.bits(3, 2)
        d.w.bits(0, 13)

    def no_partner(d):      # (BFINAL, BTYPE and nothing else would do; the literals make it look like a member)
        d.fixed([5, 6, 7, 8], False)

    over = [0] * 257
    over[65] = over[66] = over[256] = 1
    lens = _three()
    return {
        "distance_past_the_start": one(lambda d: d.fixed(list(range(10)) + [(5, 11), 1, 2], True)),
        "match_first": one(lambda d: d.fixed([(3, 1), 65, 66], True)),
        "btype_3": one(btype3),
        "stored_nlen": one(lambda d: (d.fixed([9], False), d.stored(b"stored bytes", True, nlen=0xFFF2))),
        "oversubscribed": one(lambda d: d.dynamic([65, 66], True, over, [0])),
        "sixteen_first": one(lambda d: d.dynamic([65, 66], True, lens, [0], cl_symbols=[(16, 0)] + db.plain_cl(lens[3:] + [0]), strict=False)),
        "repeat_overrun": one(lambda d: d.dynamic([65, 66], True, lens, [0], cl_symbols=db.plain_cl(lens + [0])[:-2] + [(18, 0)], strict=False)),
        "hclen_4": one(lambda d: d.dynamic([], True, [0] * 257, [0], cl_symbols=[(18, 127), (18, 109)], eob=False)),
        "distance_symbol_30": one(lambda d: d.fixed([65, 66, 67, Raw(257, 0, 30), 68], True)),
        "length_symbol_286": one(lambda d: d.fixed([65, 66, Raw(286), 67], True)),
        "no_final_block": one(no_partner),
        "no_end_of_block": one(lambda d: d.fixed([65, 66, 67, 68, 69], True, eob=False)),
    }


def _incomplete_stream():
    """literal/length code lengths 2, 2, 2: a quarter of the code space has no symbol"""
    lens = [0] * 257
    lens[65] = lens[66] = lens[256] = 2
    d = Deflate()
    d.dynamic([65, 66, 65, 65], True, lens, [0])
    return d.finish_invalid()


INVALID = sorted(_invalid_streams())


def _guarded_inflate(g, mem, comp):
    """hs._inflate with 64 sentinel bytes behind the output and the CRC check off"""
    info, poff, plen, isz, crc, ooff = g.bgzf_index(np.frombuffer(comp, dtype=np.uint8), 1000, 1 << 40)
    d_comp = mem.upload(comp, 16)
    dev = [mem.upload(a.tobytes(), 16) for a in (poff, plen, isz, crc, ooff)]
    nout = int(info.out_bytes)
    out = mem.alloc(nout + 64, 0xEE)
    mem.sync()
    rc, bad = g.inflate_bgzf(mem.ptr(d_comp), info.n_blocks, *[mem.ptr(x) for x in dev], mem.ptr(out), nout, False, check=False)
    got = mem.download(out)
    assert got[nout:] == b"\xEE" * 64, "wrote past the output buffer"
    return info, rc, bad, got[:nout]


def _good_members():
    return odd_codes()[0], block_chains()[3]


def _invalid_case(mk_engine, mem, name):
    raw, nominal = _incomplete_stream() if name == "incomplete" else _invalid_streams()[name]
    first, third = _good_members()
    comp = db.bgzf_member(*first, pad=3) + db.bgzf_member(raw, nominal, pad=0) + db.bgzf_member(*third, pad=6)
    g = mk_engine(abi.default_params(False, 150))
    info, rc, bad, got = _guarded_inflate(g, mem, comp)
    g.close()
    assert info.n_blocks == 3 and info.out_bytes == len(first[1]) + len(nominal) + len(third[1])
    assert got[:len(first[1])] == first[1] and got[len(got) - len(third[1]):] == third[1]
    return rc, bad, got[len(first[1]):len(got) - len(third[1])], nominal


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", INVALID)
def test_sim_inflate_refuses_invalid_streams(name, variant, monkeypatch):
    """the bad member between two good ones, CRC check off: the structural check refuses it, the neighbours' text is whole,
    nothing is written behind the output"""
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    rc, bad, _, _ = _invalid_case(engines.sim_engine, format_util.NumpyMem(), name)
    assert rc == abi.E_INVALID and bad == 1


@pytest.mark.gpu
@pytest.mark.twin("test_sim_inflate_refuses_invalid_streams")
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", INVALID)
def test_gpu_inflate_refuses_invalid_streams(name, variant, monkeypatch):
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    rc, bad, _, _ = _invalid_case(engines.gpu_engine, format_util.TorchMem(), name)
    assert rc == abi.E_INVALID and bad == 1


def _incomplete_case(mk_engine, mem):
    """An incomplete literal/length code in a dynamic block.  zlib refuses it ("invalid literal/lengths set"), and so do both
    host inflaters (E_INVALID, test_host_inflaters_refuse_invalid_streams).  Neither device kernel is required to, and
    neither does: both build the tables and decode the tokens, which use existing codes only - the wave kernel and the lane
    kernel return 0 with the text "ABAA".  What must hold either way: the neighbours' text is whole and nothing is written
    outside the member's own output range (_invalid_case, _guarded_inflate)."""
    rc, bad, got, nominal = _invalid_case(mk_engine, mem, "incomplete")
    assert (rc, bad) in ((0, -1), (abi.E_INVALID, 1))
    if rc == 0:
        assert got == nominal


@pytest.mark.parametrize("variant", VARIANTS)
def test_sim_inflate_incomplete_literal_code_stays_in_bounds(variant, monkeypatch):
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    _incomplete_case(engines.sim_engine, format_util.NumpyMem())


@pytest.mark.gpu
@pytest.mark.twin("test_sim_inflate_incomplete_literal_code_stays_in_bounds")
@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_inflate_incomplete_literal_code_stays_in_bounds(variant, monkeypatch):
    monkeypatch.setenv("FASTP_GPU_INFLATE", variant)
    _incomplete_case(engines.gpu_engine, format_util.TorchMem())


# ---- the host inflaters ----------------------------------------------------------------------------------------------
def test_host_inflaters_hand_built_streams(lib, tmp_path):
    """every valid member above as a gzip member, one file (empty members between them): fq_gunzip.h and fq_pgunzip.h"""
    members = [m for f in VALID for m in valid_members(f, "sim")]
    blob = b"".join(db.gzip_member(raw, text) for raw, text in members)
    want = b"".join(text for _, text in members)
    rc, got = _gunzip(lib, tmp_path, blob, len(want) + 10)
    assert rc == 0 and len(got) == len(want)
    assert got == want


def test_host_inflaters_refuse_invalid_streams(lib, tmp_path):
    first, third = _good_members()
    streams = dict(_invalid_streams(), incomplete=_incomplete_stream())
    for name, (raw, nominal) in streams.items():
        blob = db.gzip_member(*first) + db.gzip_member(raw, nominal) + db.gzip_member(*third)
        rc, _ = _gunzip(lib, tmp_path, blob, 1 << 20)
        assert rc == abi.E_INVALID, name
    rc, got = _gunzip(lib, tmp_path, db.gzip_member(*first) + db.gzip_member(*third), 1 << 20)      # the control
    assert rc == 0 and got == first[1] + third[1]


def test_host_inflaters_decoy_stream_inside_stored_blocks(lib, tmp_path):
    """one member of about 660 KB of text: two dynamic pieces written by zlib around stored blocks whose bytes are themselves a
    complete raw DEFLATE stream of 300 KB of FASTQ text.  A thread of fq_pgunzip.h that looks for a block start inside the
    stored data finds perfectly valid dynamic headers, and whole blocks behind them; the member's text is the stored bytes"""
    d = synth.synth_pairs(3000, L=150, seed=19, paired=False)
    fq = synth.to_fastq(d["seq1"], d["qual1"], d["len1"], 1)
    assert len(fq) > 900000
    a, inner_text, b = fq[:290000], fq[290000:590000], fq[590000:880000]
    inner = zlib.compressobj(6, zlib.DEFLATED, -15, 4)          # memLevel 4: blocks of 1 K symbols, many headers
    inner = inner.compress(inner_text) + inner.flush()
    assert zlib.decompress(inner, -15) == inner_text
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(a) + c.flush(zlib.Z_FULL_FLUSH)            # ends on a byte boundary
    stored = Deflate()
    for at in range(0, len(inner), 30000):
        stored.stored(inner[at:at + 30000], False)
    raw += stored.w.getvalue()
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    raw += c.compress(b) + c.flush()
    text = a + inner + b
    assert zlib.decompress(raw, -15) == text and 640000 < len(text) < 700000
    rc, got = _gunzip(lib, tmp_path, db.gzip_member(raw, text), len(text) + 10)
    assert rc == 0 and got == text
