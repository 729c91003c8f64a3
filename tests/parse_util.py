"""helpers for the device FASTQ parser tests (hostsim: plain numpy buffers; GPU: torch tensors)"""
from types import SimpleNamespace

import numpy as np

from fastp_amd import abi, engine, hostloop

BAD_MALFORMED, BAD_TOO_LONG, BAD_ALPHABET = 1, 2, 3   # FASTP_GPU_PARSE_BAD_* (include/fastp_gpu.h)
GUARD = 4                                             # records the runner allocates behind max_records
FILLS = (b"\n", b"\r", b"@", b"\x7f")                 # pad bytes that would change the answer if they were read as text
_QUAL_OK = bytes(range(33, 127))


def split_lines(text: bytes, is_last=True):
    """FastqReader::getLine over the chunk: a line ends at the first \\r or \\n; \\r\\n is one terminator.  A non-final chunk
    leaves an unterminated last line, and a last line whose terminator is the chunk's last byte and a \\r (it may be half of a
    \\r\\n), to the next chunk.  -> (lines, their offsets, the offset behind the last line taken)"""
    lines, offs = [], []
    i, n = 0, len(text)
    while i < n:
        j = i
        while j < n and text[j] not in (10, 13):
            j += 1
        if j == n:
            if not is_last:
                break
            lines.append(text[i:j]); offs.append(i); i = n
            break
        if text[j] == 13 and j == n - 1 and not is_last:
            break   # may be half of a \r\n
        lines.append(text[i:j]); offs.append(i)
        i = j + (2 if text[j] == 13 and j + 1 < n and text[j + 1] == 10 else 1)
    return lines, offs, i


def record_kinds(lines, nrec, max_len):
    """FastqReader::read's checks and the packer's, in the order fastp_gpu.h documents for FASTP_GPU_PARSE_BAD_*:
    malformed, then too long, then a quality byte outside '!'..'~'.  -> (kind of every record, 0 = accepted; the accepted
    records with a letter outside ACGTN, ascending)"""
    kinds, exotic = [], []
    for r in range(nrec):
        name, s, plus, q = lines[4 * r:4 * r + 4]
        if len(name) == 0 or name[0] != 64 or len(plus) == 0 or plus[0] != 43 or len(s) != len(q):
            kinds.append(BAD_MALFORMED)
        elif len(s) > max_len:
            kinds.append(BAD_TOO_LONG)
        elif q.translate(None, _QUAL_OK):
            kinds.append(BAD_ALPHABET)
        else:
            kinds.append(0)
            if s.translate(None, b"ACGTN"):
                exotic.append(r)
    return kinds, exotic


def _summary(kinds, exotic, seqlens, nlines, consumed):
    """the fields of fastp_gpu_parse_info that are not tables"""
    bad = [r for r, k in enumerate(kinds) if k]
    formed = [int(seqlens[r]) for r, k in enumerate(kinds) if k != BAD_MALFORMED]
    return dict(n_records=len(kinds), n_lines=nlines, consumed=consumed, max_seq_len=max(formed) if formed else 0,
                first_bad=bad[0] if bad else -1, bad_kind=kinds[bad[0]] if bad else 0,
                exotic=np.array(exotic, dtype=np.int32), kinds=np.array(kinds, dtype=np.int32))


def reference(text: bytes, max_len: int, max_records=None, is_last=True):
    """everything fastp_gpu_parse_fastq reports for `text`, by a byte loop: seq / qual rows, lens, line_off, line_len and the
    info fields (_summary).  A malformed or over-long record is refused before it is packed: length 0, zero rows.  A record
    refused for a quality byte is packed like any other (its rows are the caller's to ignore)."""
    lines, offs, end = split_lines(text, is_last)
    nrec = len(lines) // 4
    if max_records is not None:
        nrec = min(nrec, max_records)
    kinds, exotic = record_kinds(lines, nrec, max_len)
    ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
    seq = np.zeros((nrec, ss), dtype=np.uint8)
    qual = np.zeros((nrec, qs), dtype=np.uint8)
    lens = np.zeros(nrec, dtype=np.uint16)
    code = {65: 0, 84: 1, 67: 2, 71: 3}
    for r in range(nrec):
        if kinds[r] in (BAD_MALFORMED, BAD_TOO_LONG):
            continue
        s, q = lines[4 * r + 1], lines[4 * r + 3]
        lens[r] = len(s)
        for j, ch in enumerate(s):
            seq[r, j >> 2] |= code.get(ch, 0) << ((j & 3) * 2)
            qual[r, j] = q[j] | (0x80 if ch == 78 else 0)
    loff = np.array(offs[:4 * nrec], dtype=np.uint32)
    llen = np.array([len(x) for x in lines[:4 * nrec]], dtype=np.uint32)
    if nrec == 0:
        consumed = 0
    elif 4 * nrec < len(lines):
        consumed = offs[4 * nrec]
    else:
        consumed = end
    return SimpleNamespace(seq=seq, qual=qual, lens=lens, line_off=loff, line_len=llen,
                           **_summary(kinds, exotic, llen[1::4], len(lines), consumed))


def expected(text: bytes, max_len: int, max_records=None, is_last=True):
    """what FastqReader + the packer would produce for the complete records of `text`:
    (seq rows, qual rows, lens, line offsets, line lengths, consumed)"""
    w = reference(text, max_len, max_records, is_last)
    return w.seq, w.qual, w.lens, w.line_off, w.line_len, w.consumed


def first_bad_expected(text: bytes, max_len: int, max_records=None, is_last=True):
    """(index of the smallest refused record or -1, its FASTP_GPU_PARSE_BAD_* kind or 0, the accepted records with a letter
    outside ACGTN, ascending)"""
    lines, _, _ = split_lines(text, is_last)
    nrec = len(lines) // 4 if max_records is None else min(len(lines) // 4, max_records)
    kinds, exotic = record_kinds(lines, nrec, max_len)
    bad = [r for r, k in enumerate(kinds) if k]
    return (bad[0], kinds[bad[0]], exotic) if bad else (-1, 0, exotic)


def reference_np(text: bytes, max_len: int, max_records=None, is_last=True, lib=None):
    """reference() restated on whole arrays, for texts too large for a byte loop; the rows come from the library's host
    packer (engine.pack_ascii).  tests/test_parse_edges.py holds it equal to reference() on every small text."""
    t = np.frombuffer(text, dtype=np.uint8)
    n = len(t)
    cr, lf = t == 13, t == 10
    after_cr = np.concatenate(([False], cr[:-1])) if n else cr
    pos = np.flatnonzero(cr | (lf & ~after_cr)).astype(np.int64)       # where a terminator starts
    tp = np.concatenate((t, np.zeros(1, dtype=np.uint8)))              # (t[n] reads as "no \n")
    tlen = 1 + ((tp[pos] == 13) & (tp[pos + 1] == 10) & (pos + 1 < n)).astype(np.int64)
    if not is_last and n and t[-1] == 13:                              # may be half of a \r\n: the next chunk's line
        pos, tlen = pos[:-1], tlen[:-1]
    starts = np.concatenate(([0], pos + tlen)).astype(np.int64)        # starts[k]: line k; the last: behind the last terminator
    ends = pos
    if is_last and starts[-1] < n:                                     # an unterminated last line still is a line
        ends = np.concatenate((ends, [n]))
    else:
        starts = starts[:-1]
    nlines = len(ends)
    nrec = nlines // 4 if max_records is None else min(nlines // 4, max_records)
    loff, llen = starts[:4 * nrec], (ends - starts)[:4 * nrec]
    if nrec == 0:
        consumed = 0
    elif 4 * nrec < nlines:
        consumed = int(starts[4 * nrec])
    else:
        consumed = int(pos[-1] + tlen[-1]) if len(pos) == nlines else n
    o, l = loff.reshape(nrec, 4), llen.reshape(nrec, 4)
    malformed = (l[:, 0] == 0) | (tp[o[:, 0]] != 64) | (l[:, 2] == 0) | (tp[o[:, 2]] != 43) | (l[:, 1] != l[:, 3])
    too_long = ~malformed & (l[:, 1] > max_len)
    L = np.where(malformed | too_long, 0, l[:, 1])
    col = np.arange(max(max_len, 1), dtype=np.int64)
    live = col[None, :] < L[:, None]
    S = np.where(live, tp[np.minimum(o[:, 1][:, None] + col[None, :], n)], 0).astype(np.uint8)
    Q = np.where(live, tp[np.minimum(o[:, 3][:, None] + col[None, :], n)], 0).astype(np.uint8)
    badq = (((Q < 33) | (Q > 126)) & live).any(axis=1)
    foreign = (~np.isin(S, np.frombuffer(b"ACGTN", dtype=np.uint8)) & live).any(axis=1)
    kinds = np.where(malformed, BAD_MALFORMED, np.where(too_long, BAD_TOO_LONG, np.where(badq, BAD_ALPHABET, 0)))
    # the host packer refuses a quality byte outside '!'..'~': such a record is packed with a stand-in and its quality row set
    # by the packer's rule (the byte, 0x80 added under an N)
    Qp = np.where(badq[:, None] & live, np.uint8(73), Q)
    ex = np.zeros(max(nrec, 1), dtype=np.uint8)
    seq, qual, lens = engine.pack_ascii(lib or engine.load_library(), max_len, S, Qp, L.astype(np.int32), ex)
    for r in np.flatnonzero(badq):
        qual[r, :L[r]] = Q[r, :L[r]] | np.where(S[r, :L[r]] == 78, 0x80, 0).astype(np.uint8)
    return SimpleNamespace(seq=seq, qual=qual, lens=lens, line_off=loff.astype(np.uint32), line_len=llen.astype(np.uint32),
                           **_summary(kinds.tolist(), np.flatnonzero(foreign & (kinds == 0)).tolist(), l[:, 1], nlines, consumed))


def expected_np(text: bytes, max_len: int, max_records=None, is_last=True, lib=None):
    """expected(), from reference_np"""
    w = reference_np(text, max_len, max_records, is_last, lib)
    return w.seq, w.qual, w.lens, w.line_off, w.line_len, w.consumed


FIELDS = ("n_records", "n_lines", "consumed", "max_seq_len", "first_bad", "bad_kind")
TABLES = ("seq", "qual", "lens", "line_off", "line_len", "exotic", "kinds")


def same_reference(a, b):
    """the first field in which two results of reference() / reference_np() differ, or None"""
    for k in FIELDS:
        if getattr(a, k) != getattr(b, k):
            return f"{k}: {getattr(a, k)} != {getattr(b, k)}"
    for k in TABLES:
        x, y = getattr(a, k), getattr(b, k)
        if x.shape != y.shape or not np.array_equal(x, y):
            return f"{k} differs"
    return None


def run_numpy(eng, text: bytes, max_len: int, max_records: int, is_last=True, check=True):
    """hostsim: 'device' pointers are host pointers"""
    pad = (-len(text)) % 16 + 16
    buf = np.frombuffer(text + b"\0" * pad, dtype=np.uint8).copy()
    base = buf.ctypes.data
    shift = (-base) % 16
    if shift:   # 16-byte alignment
        big = np.zeros(len(buf) + 16, dtype=np.uint8)
        o = (-big.ctypes.data) % 16
        big[o:o + len(buf)] = buf
        buf = big[o:o + len(buf)]
    ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
    seq = np.full((max(1, max_records), ss), 0xEE, dtype=np.uint8)
    qual = np.full((max(1, max_records), qs), 0xEE, dtype=np.uint8)
    lens = np.zeros(max(1, max_records), dtype=np.uint16)
    loff = np.zeros(4 * max(1, max_records), dtype=np.uint32)
    llen = np.zeros(4 * max(1, max_records), dtype=np.uint32)
    info = eng.parse_fastq(buf.ctypes.data, len(text), is_last, max_records, seq.ctypes.data, qual.ctypes.data,
                           lens.ctypes.data, loff.ctypes.data, llen.ctypes.data, check=check)
    n = info.n_records
    return info, seq[:n], qual[:n], lens[:n], loff[:4 * n], llen[:4 * n]


def run(eng, mem, text: bytes, max_len: int, max_records: int, is_last=True, pad_fill=b"\0", check=True):
    """run_numpy on the NumpyMem / TorchMem of tests/format_util.py, so that one test body serves the emulator and the GPU.
    The text gets the documented minimum of padding, (-len) % 16 bytes, plus 16, filled with `pad_fill` repeated.  The output
    buffers hold max_records + GUARD records and are 0xEE throughout before the call.
    -> (info, seq, qual, lens, line_off, line_len, guard): the tables of the info.n_records records, and what lies behind
    them in the five buffers - the capacity not used and the GUARD records - as five uint8 arrays that must still be 0xEE"""
    pad = (-len(text)) % 16 + 16
    t = mem.upload(text + (pad_fill * pad)[:pad])
    cap = max(0, max_records) + GUARD
    ss, qs = abi.seq_stride(max_len), abi.qual_stride(max_len)
    widths = (ss, qs, 2, 16, 16)
    bufs = [mem.alloc(cap * w, 0xEE) for w in widths]
    mem.sync()
    info = eng.parse_fastq(mem.ptr(t), len(text), is_last, max_records, *[mem.ptr(b) for b in bufs], check=check)
    n = info.n_records
    raw = [np.frombuffer(mem.download(b, cap * w), dtype=np.uint8) for b, w in zip(bufs, widths)]
    guard = [a[n * w:] for a, w in zip(raw, widths)]
    seq, qual = raw[0][:n * ss].reshape(n, ss), raw[1][:n * qs].reshape(n, qs)
    lens, loff, llen = raw[2][:2 * n].view(np.uint16), raw[3][:16 * n].view(np.uint32), raw[4][:16 * n].view(np.uint32)
    return info, seq, qual, lens, loff, llen, guard


# ---- text builders ----------------------------------------------------------------------------------------------------------
_NAME_FILL = b"abcdefghijklmnopqrstuvwxyz0123456789:/_#ABCDEFGHIJKLMNOPQRSTUVWXYZ "
_HIT_NAME_MAX = 1200   # a record takes a target once its name line would be at most this long (a filler record is shorter)


def _name(r, length):
    """a name line of exactly `length` >= 1 bytes"""
    s = b"@" + b"r%d:" % r + _NAME_FILL * (length // len(_NAME_FILL) + 1)
    return s[:length]


def _read(rng, L):
    """sequence and quality lines of L bases: N at bases 0, 3, 4 and L - 1 of some reads; '!' and '~' among the qualities;
    quality lines that start with '@'"""
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
    q = rng.integers(35, 75, size=L).astype(np.uint8)
    if L:
        for at in (0, 3, 4, L - 1):
            if at < L and rng.random() < 0.35:
                s[at] = 78
        q[rng.integers(0, L)] = 33
        q[rng.integers(0, L)] = 126
        if rng.random() < 0.3:
            q[0] = 64
    return s.tobytes(), q.tobytes()


def place(records: int, eol: bytes, targets, max_len=150, seed=1, last_eol=True, min_bytes=0):
    """FASTQ text of at least `records` ragged records in which, for every (offset, line) or (offset, line, record) of
    `targets` (ascending offsets; line 0 name, 1 sequence, 2 plus, 3 quality), the terminator of that line of one record
    - of that record, when it is named - starts at exactly that byte.  Records are emitted in order; the one that reaches for
    a target gets a name line of the length that puts the terminator there.  Read lengths are drawn from 0 .. max_len (the
    first two records without a target have max_len and 0), '+' lines are bare or repeat the name.  The text ends behind the
    last target once there are `records` records and `min_bytes` bytes.
    -> (text, [(offset, line, record)] as hit); asserts every target was hit"""
    rng = np.random.default_rng(seed)
    e = len(eol)
    todo = [tuple(t) + (None,) * (3 - len(t)) for t in sorted(targets)]
    parts, hit = [], []
    pos, r, fillers = 0, 0, 0
    while todo or r < records or pos < min_bytes:
        L = int(rng.integers(0, max_len + 1))
        repeat = rng.random() < 0.4
        nlen = None
        if todo:
            off, line, rec = todo[0]
            # bytes between the name line's end and the terminator aimed at (the '+' line of such a record is bare)
            between = (0, e, 2 * e + 1, 3 * e + 1)[line]
            if off - pos - between - (0, L, L, 2 * L)[line] < 1:   # too near for this read: an empty one
                L = 0
            need = off - pos - between - (0, L, L, 2 * L)[line]
            assert need >= 1, f"target {off} (line {line}) cannot be reached from offset {pos}"
            assert rec is None or rec >= r, f"target {off}: record {rec} is behind it"
            if rec == r or (rec is None and need <= _HIT_NAME_MAX):
                nlen, repeat = need, repeat and line < 2
                hit.append((off, line, r))
                todo.pop(0)
        if nlen is None:
            nlen = int(rng.integers(1, 140))
            if fillers < 2:
                L = (max_len, 0)[fillers]
            fillers += 1
        name = _name(r, nlen)
        s, q = _read(rng, L)
        rec_bytes = eol.join((name, s, b"+" + name[1:] if repeat else b"+", q)) + eol
        parts.append(rec_bytes)
        pos += len(rec_bytes)
        r += 1
    text = b"".join(parts)
    if not last_eol:
        text = text[:-e]
    lines, offs, _ = split_lines(text + (b"" if last_eol else eol), True)
    for off, line, rec in hit:
        k = 4 * rec + line
        assert offs[k] + len(lines[k]) == off and text[off:off + e] in (eol, eol[:len(text) - off]), (off, line, rec)
    assert len(hit) == len(targets)
    return text, hit


def big_text(nbytes: int, eol=b"\r\n", max_len=250, seed=5):
    """ragged FASTQ text of whole records, less than one record short of `nbytes`, built on whole arrays: names '@' + nine
    digits, reads of max_len bases (seven in ten) or of 0 .. max_len, N in one base of fifty, '+' lines bare or repeating the
    name (every other record), qualities '!' .. '~'"""
    rng = np.random.default_rng(seed)
    e = len(eol)
    guess = nbytes // (12 + 4 * e) + 1   # (more records than fit)
    L = np.where(rng.random(guess) < 0.7, max_len, rng.integers(0, max_len + 1, size=guess)).astype(np.int64)
    plen = np.where(np.arange(guess) % 2 == 1, 10, 1).astype(np.int64)
    size = 10 + plen + 2 * L + 4 * e
    n = int(np.searchsorted(np.cumsum(size), nbytes, side="right"))
    L, plen, size = L[:n], plen[:n], size[:n]
    start = np.cumsum(size) - size
    out = np.zeros(int(size.sum()), dtype=np.uint8)
    digits = ((np.arange(n)[:, None] // 10 ** np.arange(8, -1, -1)[None, :]) % 10 + 48).astype(np.uint8)
    eolb = np.frombuffer(eol, dtype=np.uint8)

    def put(at, rows):   # rows [n, w] at offsets at[n]
        out[at[:, None] + np.arange(rows.shape[1])[None, :]] = rows

    def put_ragged(at, flat):   # L[k] bytes of flat at offset at[k]
        out[np.repeat(at, L) + np.arange(len(flat)) - np.repeat(np.cumsum(L) - L, L)] = flat

    s_at = start + 10 + e
    p_at = s_at + L + e
    q_at = p_at + plen + e
    put(start, np.concatenate((np.full((n, 1), 64, dtype=np.uint8), digits), axis=1))
    for at in (start + 10, s_at + L, p_at + plen, q_at + L):
        put(at, np.broadcast_to(eolb, (n, e)))
    total = int(L.sum())
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=total)
    bases[rng.random(total) < 0.02] = 78
    put_ragged(s_at, bases)
    put_ragged(q_at, rng.integers(33, 127, size=total).astype(np.uint8))
    out[p_at] = 43
    rep = plen == 10
    out[p_at[rep][:, None] + 1 + np.arange(9)[None, :]] = digits[rep]
    return out.tobytes()
