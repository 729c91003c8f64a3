"""A token-level DEFLATE (RFC 1951) writer for the tests: streams zlib never writes - chosen code lengths, chosen repeat
codes in the dynamic header, any distance / length symbol with any extra bits, block chains of every kind - and the
streams a decoder has to refuse.

    d = Deflate()
    d.fixed([65, 66, (10, 2)], last=False)
    d.stored(b"xyz", last=True)
    raw, text = d.finish()

A token is a literal (int), a match (length, distance) written with the symbols RFC 1951 3.2.5 gives it, or a `Raw`
(a length symbol and a distance symbol with chosen extra bits - symbol 284 with extra 31, and the symbols that do not
exist).  The writer is never trusted on its own: `finish()` has zlib decode every stream it hands out and compares the
text with `expand()`, the plain-Python meaning of the tokens; `finish_invalid()` has zlib refuse the stream."""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32          # symbols 30 and 31 have codes and no meaning (3.2.6)


class BitWriter:
    """LSB-first: the first bit written is bit 0 of the first byte (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, width):
        assert 0 <= value < (1 << width) or width == 0
        self.acc |= value << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: packed starting with its most significant bit"""
        rev = 0
        for _ in range(length):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bit_pos(self):
        return len(self.out) * 8 + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)} of the symbols with a non-zero length.  (An over-subscribed set gives
    codes that do not fit their length; they are masked - such a set only ever heads a stream that must be refused.)"""
    count = [0] * 17
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def kraft(lengths):
    """sum of 2^-length in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def ladder(n):
    """n code lengths of a COMPLETE code that reaches 15 bits and keeps its short codes: 1, 2, 3, ... as far as the symbol
    count lets it, the rest as deep as possible.  (Start from one leaf; always split the deepest leaf above 15 bits.)"""
    assert 2 <= n <= 32768
    count = [0] * 16
    count[0] = 1
    for _ in range(n - 1):
        ln = max(k for k in range(15) if count[k])
        count[ln] -= 1
        count[ln + 1] += 2
    out = [ln for ln in range(16) for _ in range(count[ln])]
    assert len(out) == n and kraft(out) == 32768
    return out


def balanced(n, used):
    """n code lengths, a complete code over the symbols `used` whose lengths differ by one bit at most"""
    used = sorted(used)
    assert len(used) >= 2
    k = (len(used) - 1).bit_length()
    short = (1 << k) - len(used)
    out = [0] * n
    for i, s in enumerate(used):
        out[s] = k - 1 if i < short else k
    assert kraft(out) == 32768
    return out


def len_symbol(length):
    """(symbol, extra bits, extra value) as a compressor writes the length: 258 is symbol 285"""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


_LEN_SYM = {ln: len_symbol(ln) for ln in range(3, 259)}
_DIST_SYM = {}


class Raw:
    """the writer hook: length symbol `lsym` with `lextra` in its extra bits, then (unless dsym is None) distance symbol
    `dsym` with `dextra`.  Symbols without a meaning (286, 287; 30, 31) carry no extra bits."""

    def __init__(self, lsym, lextra=0, dsym=None, dextra=0):
        self.lsym, self.lextra, self.dsym, self.dextra = lsym, lextra, dsym, dextra

    def meaning(self):
        """(length, distance), or None where the symbols have none"""
        if not (257 <= self.lsym <= 285) or self.dsym is None or self.dsym > 29:
            return None
        return LEN_BASE[self.lsym - 257] + self.lextra, DIST_BASE[self.dsym] + self.dextra


def _copy(out, length, dist):
    if dist > len(out) or dist < 1:
        raise ValueError("distance reaches in front of the text")
    if dist >= length:
        start = len(out) - dist
        out += out[start:start + length]
    else:
        pat = bytes(out[-dist:])
        out += (pat * (length // dist + 1))[:length]


def expand(tokens, history=b""):
    """the text the tokens stand for, behind `history` (the member's text so far); returns only the new bytes"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, dist = t.meaning() if isinstance(t, Raw) else t
            _copy(out, ln, dist)
    return bytes(out[len(history):])


def expand_cl(cl_symbols):
    """the code lengths a sequence of (code-length symbol, extra) stands for (3.2.7)"""
    out = []
    for s, x in cl_symbols:
        if s < 16:
            out.append(s)
        elif s == 16:
            assert 0 <= x <= 3
            out += [out[-1]] * (3 + x)
        elif s == 17:
            assert 0 <= x <= 7
            out += [0] * (3 + x)
        else:
            assert s == 18 and 0 <= x <= 127
            out += [0] * (11 + x)
    return out


def plain_cl(lengths):
    """one code-length symbol per length, no repeats"""
    return [(ln, 0) for ln in lengths]


def compact_cl(lengths):
    """greedy run-length form, as a compressor would write it"""
    out, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i
        i = j
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
        out += [(v, 0)] * run
    return out


def _cl_code_lengths(used):
    """a complete code of at most 7 bits over the code-length symbols in use (a lone symbol gets a partner: zlib
    refuses an incomplete code-length code)"""
    used = sorted(used)
    if len(used) == 1:
        used.append(next(s for s in (0, 1, 2) if s not in used))
    n = len(used)
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    assert kraft(lens) == 32768 and max(lens) <= 7
    return lens


class Deflate:
    """one raw DEFLATE stream, block by block; keeps the text the blocks stand for"""

    def __init__(self):
        self.w = BitWriter()
        self.text = bytearray()
        self.header_bits = []      # bit offset of every block header (the tests check what they meant to build)
        self.token_bits = None     # set to [] to record (first bit, bits) of every token written

    # ---- blocks ----
    def stored(self, data, last, nlen=None):
        self.header_bits.append(self.w.bit_pos())
        assert len(data) <= 65535
        self.w.bits(int(last), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.out += data
        self.text += data

    def fixed(self, tokens, last, eob=True):
        self.header_bits.append(self.w.bit_pos())
        self.w.bits(int(last), 1)
        self.w.bits(1, 2)
        self._tokens(tokens, canonical_codes(FIXED_LITLEN), canonical_codes(FIXED_DIST), eob)

    def dynamic(self, tokens, last, litlen_lengths, dist_lengths, cl_symbols=None, hclen=None, cl_lengths=None, strict=True,
                eob=True):
        """litlen_lengths (257..286 of them) and dist_lengths (1..30) are what HLIT and HDIST announce.  cl_symbols is the
        header's sequence of (code-length symbol, extra); by default one symbol per length.  hclen = how many code-length
        code lengths are sent (default: as few as the code allows).  strict=False: cl_symbols need not spell the lengths
        (for streams that must be refused)."""
        self.header_bits.append(self.w.bit_pos())
        nl, nd = len(litlen_lengths), len(dist_lengths)
        assert 257 <= nl <= 288 and 1 <= nd <= 32
        if cl_symbols is None:
            cl_symbols = plain_cl(list(litlen_lengths) + list(dist_lengths))
        if strict:
            assert expand_cl(cl_symbols) == list(litlen_lengths) + list(dist_lengths), "cl_symbols spell other code lengths"
        if cl_lengths is None:
            cl_lengths = _cl_code_lengths({s for s, _ in cl_symbols})
        need = max(k for k in range(19) if cl_lengths[CL_ORDER[k]]) + 1
        if hclen is None:
            hclen = max(4, need)
        assert 4 <= hclen <= 19 and (hclen >= need or not strict)
        w = self.w
        w.bits(int(last), 1)
        w.bits(2, 2)
        w.bits(nl - 257, 5)
        w.bits(nd - 1, 5)
        w.bits(hclen - 4, 4)
        for k in range(hclen):
            w.bits(cl_lengths[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl_lengths)
        for s, x in cl_symbols:
            w.code(*cl_codes[s])
            if s >= 16:
                w.bits(x, {16: 2, 17: 3, 18: 7}[s])
        self._tokens(tokens, canonical_codes(litlen_lengths), canonical_codes(dist_lengths), eob)

    def _tokens(self, tokens, lcodes, dcodes, eob):
        w = self.w
        code, bits, text = w.code, w.bits, self.text
        for t in tokens:
            if self.token_bits is not None:
                if self.token_bits and self.token_bits[-1][1] is None:
                    self.token_bits[-1][1] = w.bit_pos() - self.token_bits[-1][0]
                self.token_bits.append([w.bit_pos(), None])
            if isinstance(t, int):
                code(*lcodes[t])
                text.append(t)
                continue
            if isinstance(t, Raw):
                code(*lcodes[t.lsym])
                if 257 <= t.lsym <= 285:
                    bits(t.lextra, LEN_EXTRA[t.lsym - 257])
                if t.dsym is not None:
                    code(*dcodes[t.dsym])
                    if t.dsym <= 29:
                        bits(t.dextra, DIST_EXTRA[t.dsym])
                m = t.meaning()
                if m is not None and 1 <= m[1] <= len(text):
                    _copy(text, *m)
                continue
            ln, dist = t
            ls, lb, lx = _LEN_SYM[ln]
            code(*lcodes[ls])
            bits(lx, lb)
            d = _DIST_SYM.get(dist)
            if d is None:
                d = _DIST_SYM[dist] = dist_symbol(dist)
            code(*dcodes[d[0]])
            bits(d[2], d[1])
            if dist <= len(text):
                _copy(text, ln, dist)
            else:
                text += bytes(ln)      # (a stream that must be refused: what a decoder without the check would write)
        if self.token_bits:
            self.token_bits[-1][1] = w.bit_pos() - self.token_bits[-1][0]
        if eob:
            code(*lcodes[256])

    # ---- the finished stream ----
    def finish(self):
        """(raw stream, text) - after zlib has decoded the stream to exactly this text and used every byte of it"""
        raw, text = self.w.getvalue(), bytes(self.text)
        z = zlib.decompressobj(-15)
        got = z.decompress(raw)
        assert z.eof and not z.unused_data and got == text, "the writer and zlib disagree"
        return raw, text

    def finish_invalid(self):
        """(raw stream, nominal text) of a stream zlib refuses"""
        raw = self.w.getvalue()
        z = zlib.decompressobj(-15)
        try:
            z.decompress(raw)
            refused = not z.eof         # (a stream that simply ends: zlib waits for more)
        except zlib.error:
            refused = True
        assert refused, "zlib accepts this stream"
        return raw, bytes(self.text)


# ---- containers ---------------------------------------------------------------------------------------------------
def bgzf_member(raw, text, pad=None, crc=None, isize=None):
    """a BGZF member around a raw stream.  pad = None: bgzip's header; otherwise a dummy extra subfield with `pad` bytes of
    data (4 + pad bytes in all) in front of BC, which moves the payload's address byte by byte."""
    extra = b"" if pad is None else b"PD" + struct.pack("<H", pad) + bytes(range(1, pad + 1))
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(raw) + 8
    assert bsize <= 65536, f"member of {bsize} bytes"
    assert len(text) <= 65536
    hdr = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return hdr + raw + struct.pack("<II", (zlib.crc32(text) if crc is None else crc) & 0xFFFFFFFF, len(text) if isize is None else isize)


def bgzf_file(members, residues=True):
    """[(raw, text) ...] -> (BGZF bytes, payload offsets).  residues: member k's payload starts at an offset = k mod 16
    (the caller uploads the file to a 16-byte aligned address), so that a run of members meets every alignment."""
    out, offs = bytearray(), []
    for k, (raw, text) in enumerate(members):
        pad = (k - (len(out) + 12 + 4 + 6)) % 16 if residues else None
        m = bgzf_member(raw, text, pad)
        offs.append(len(out) + len(m) - 8 - len(raw))
        assert not residues or offs[-1] % 16 == k % 16
        out += m
    return bytes(out), offs


def gzip_member(raw, text, crc=None, isize=None):
    """a plain RFC 1952 member (for the host inflaters)"""
    return (b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + raw
            + struct.pack("<II", (zlib.crc32(text) if crc is None else crc) & 0xFFFFFFFF, (len(text) if isize is None else isize) & 0xFFFFFFFF))
