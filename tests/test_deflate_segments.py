"""fastp_gpu_deflate_bgzf_segments: one text cut into segments that share no gzip member (the file slices of a --split run's
trip), against fastp_gpu_deflate_bgzf_level on every segment alone - the same bytes - and against gzip / zlib.  Every case
runs on the emulator in the CPU suite and, under -m gpu, on the card.

Byte equality and the emulator: the greedy match stage (levels 0..4, fq_deflate.h def_parse_greedy) lets the lanes of a step
that hash to one bucket store their positions to the same LDS word; whichever store lands last is the candidate of later
steps.  The card settles that the same way every time; the emulator resumes lanes in a shuffled order on purpose, so there
two identical fastp_gpu_deflate_bgzf calls already give different (equally valid) members.  The emulator cases therefore
compare bytes at the chain levels (6, 9: their insert is ordered) and check everything else at every level; for levels 0 and 1
one-segment calls are compared in fresh interpreters (the same generator state on both sides); the GPU cases compare bytes at
all four levels, every segment."""
import gzip
import zlib

import numpy as np
import pytest

import engines
import format_util
import test_hostsim_parity as hs
from fastp_amd import abi
from test_deflate_levels import BLOCK, EOF_MEMBER, _members

LEVELS = [0, 1, 6, 9]
EDGE_LENGTHS = [0, 1, 65279, 65280, 65281, 130561]
EDGE_EOF = [1, 0, 1, 0, 0, 1]          # (the empty segment carries one: an end-of-file member and nothing else)
_cache = {}


def _text():
    if "t" not in _cache:
        _cache["t"] = hs._se_fastq_text(1500, 5)
    return _cache["t"]


def _capacity(nbytes, n_segments):
    return nbytes + 31 * (nbytes // BLOCK + n_segments) + 28 * n_segments     # include/fastp_gpu.h


def _offsets(lengths, first=0):
    return [first + int(x) for x in np.concatenate([[0], np.cumsum(lengths)])]


def _segments(g, mem, text, seg_off, seg_eof, level, cap=None):
    """(rc, output bytes up to min(needed, cap), seg_out_off); asserts that nothing lies behind the reported size"""
    t = mem.upload(text, 16)
    nbytes = seg_off[-1] - seg_off[0]
    cap = _capacity(nbytes, len(seg_off) - 1) if cap is None else cap
    out = mem.alloc(max(16, cap), 0xEE)
    mem.sync()
    rc, out_off = g.deflate_bgzf_segments(mem.ptr(t), seg_off, seg_eof, level, mem.ptr(out), cap, check=False)
    raw = mem.download(out)
    keep = min(out_off[-1], cap)
    assert raw[keep:].count(b"\xEE") == len(raw) - keep, "bytes written past the reported size"
    return rc, raw[:keep], out_off


def _alone(g, mem, piece, eof, level):
    t = mem.upload(piece, 16)
    cap = len(piece) + 31 * (len(piece) // BLOCK + 1) + 28
    out = mem.alloc(max(16, cap), 0xEE)
    mem.sync()
    rc, n = g.deflate_bgzf(mem.ptr(t), len(piece), mem.ptr(out), cap, bool(eof), check=False, level=level)
    assert rc == 0
    return mem.download(out, n)


def _same_bytes(mk_engine, level):
    return mk_engine is engines.gpu_engine or level >= 5


def _check(g, mem, text, seg_off, seg_eof, level, compare_alone=True):
    rc, comp, out_off = _segments(g, mem, text, seg_off, seg_eof, level)
    n = len(seg_off) - 1
    assert rc == 0 and len(out_off) == n + 1 and out_off[0] == 0 and out_off[-1] == len(comp)
    assert out_off[-1] <= _capacity(seg_off[-1] - seg_off[0], n)
    for i in range(n):
        piece = text[seg_off[i]:seg_off[i + 1]]
        eof = bool(seg_eof[i]) if seg_eof is not None else False
        got = comp[out_off[i]:out_off[i + 1]]
        if not piece and not eof:
            assert got == b""
            continue
        assert gzip.decompress(got) == piece, f"segment {i}"
        mem_list = _members(got)
        assert len(mem_list) == (len(piece) + BLOCK - 1) // BLOCK + int(eof)
        for k, m in enumerate(mem_list[:len(mem_list) - int(eof)]):   # no member spans a cut, none reaches in front of its block
            assert zlib.decompress(m, 31) == piece[k * BLOCK:(k + 1) * BLOCK], f"segment {i} member {k}"
        assert not eof or got.endswith(EOF_MEMBER)
        if compare_alone:
            assert got == _alone(g, mem, piece, eof, level), f"segment {i}: not the bytes of the segment deflated alone"
    return comp, out_off


def _edge_case(mk_engine, mem, level):
    text = _text()
    seg_off = _offsets(EDGE_LENGTHS, first=37)     # (the first segment does not start the text)
    assert seg_off[-1] <= len(text)
    g = mk_engine(abi.default_params(False, 150))
    try:
        _check(g, mem, text, seg_off, EDGE_EOF, level, compare_alone=_same_bytes(mk_engine, level))
    finally:
        g.close()


def _many_case(mk_engine, mem, level):
    """300 segments: 13 rounds of blocks on the emulator's three CUs (a round is cus * 8 blocks)"""
    text = _text()
    rng = np.random.default_rng(31)
    lengths = rng.integers(100, 3001, size=300)
    seg_off = _offsets(lengths)
    assert seg_off[-1] <= len(text) and len(lengths) > 3 * 8
    eof = [int(i % 7 == 3) for i in range(300)]
    g = mk_engine(abi.default_params(False, 150))
    try:
        comp, out_off = _check(g, mem, text, seg_off, eof, level, compare_alone=_same_bytes(mk_engine, level))
        # without flags: the members of the whole call inflate to the text
        comp, out_off = _check(g, mem, text, seg_off, None, level, compare_alone=False)
        assert gzip.decompress(comp) == text[:seg_off[-1]]
    finally:
        g.close()


def _arguments_case(mk_engine, mem):
    text = _text()[:70000]
    g = mk_engine(abi.default_params(False, 150))
    try:
        rc, comp, out_off = _segments(g, mem, text, [0], None, 6)                 # no segment
        assert rc == 0 and comp == b"" and out_off == [0]
        rc, comp, out_off = _segments(g, mem, text, [5, 5, 5], None, 6)           # empty ones alone
        assert rc == 0 and comp == b"" and out_off == [0, 0, 0]
        rc, comp, out_off = _segments(g, mem, text, [5, 5, 5], [0, 1], 6)
        assert rc == 0 and comp == EOF_MEMBER and out_off == [0, 0, 28]
        # too small a buffer: the needed size, and what fits of whole members in front of the 0xEE fill
        seg_off, eof = [0, 1000, 1000, 66500, 70000], [1, 0, 0, 1]
        rc, whole, want_off = _segments(g, mem, text, seg_off, eof, 6)
        assert rc == 0
        for cap in (0, 10, want_off[1], want_off[3] + 5, want_off[-1] - 1):
            rc, part, out_off = _segments(g, mem, text, seg_off, eof, 6, cap=cap)
            assert rc == abi.E_OVERFLOW and out_off == want_off, cap
        rc, part, out_off = _segments(g, mem, text, seg_off, eof, 6, cap=want_off[-1])
        assert rc == 0 and part == whole and gzip.decompress(part) == text
        for bad_off in ([0, 10, 5], [-1, 4]):
            rc, _, _ = _segments(g, mem, text, bad_off, None, 6, cap=100000)
            assert rc == abi.E_INVALID
        for level in (-1, 10):
            rc, _, _ = _segments(g, mem, text, [0, 10], None, level)
            assert rc == abi.E_INVALID
    finally:
        g.close()


@pytest.mark.parametrize("level", LEVELS)
def test_sim_deflate_segments_at_block_edges(level):
    _edge_case(engines.sim_engine, format_util.NumpyMem(), level)


@pytest.mark.parametrize("level", LEVELS)
def test_sim_deflate_segments_over_several_rounds(level):
    _many_case(engines.sim_engine, format_util.NumpyMem(), level)


def test_sim_deflate_segments_arguments():
    _arguments_case(engines.sim_engine, format_util.NumpyMem())


_CHILD = """
import hashlib, sys
import engines, format_util
import test_deflate_segments as t
from fastp_amd import abi
how, level, first, length = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
g = engines.sim_engine(abi.default_params(False, 150))
mem = format_util.NumpyMem()
text = t._text()
if how == "segments":
    rc, comp, off = t._segments(g, mem, text, [first, first + length], [1], level)
    assert rc == 0 and off == [0, len(comp)]
else:
    comp = t._alone(g, mem, text[first:first + length], 1, level)
print(hashlib.sha256(comp).hexdigest())
"""


def _fresh(how, level, first, length):
    """one call in a fresh interpreter (test_deflate_levels._sim_default_bytes has the reason: the emulator's lane order comes
    from one generator per process, so only the first calls of two processes that launch the same grids see the same order)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", _CHILD, how, str(level), str(first), str(length)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("length", [65279, 65281])
@pytest.mark.parametrize("level", [0, 1])
def test_sim_deflate_segments_greedy_levels_equal_in_fresh_interpreters(level, length):
    """levels 0 and 1 on the emulator: a one-segment call (the block table's path, the segment 37 bytes into the text, the
    end-of-file member from the gather kernel) writes the bytes of fastp_gpu_deflate_bgzf_level on that piece - each in its own
    interpreter, where both launch the same grids from the same generator state"""
    engines.build_sim()
    assert _fresh("segments", level, 37, length) == _fresh("alone", level, 37, length)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_deflate_segments_at_block_edges")
@pytest.mark.parametrize("level", LEVELS)
def test_gpu_deflate_segments_at_block_edges(level):
    _edge_case(engines.gpu_engine, format_util.TorchMem(), level)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_deflate_segments_over_several_rounds")
@pytest.mark.parametrize("level", LEVELS)
def test_gpu_deflate_segments_over_several_rounds(level):
    _many_case(engines.gpu_engine, format_util.TorchMem(), level)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_deflate_segments_arguments")
def test_gpu_deflate_segments_arguments():
    _arguments_case(engines.gpu_engine, format_util.TorchMem())
