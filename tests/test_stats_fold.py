"""The Stats fold has two kernels: fq_reduce_kernel walks a group of REDUCE_GROUP slabs one load at a time, and
fq_reduce_wide_kernel - what a launch with more than one such group takes - splits a larger group's slabs over the
waves of a workgroup, keeps WIDE_UNROLL loads in flight per lane, reads a packed per-cycle cell as one 8-byte load and
adds the waves' partial sums in LDS.  They are one mapping from slab to counter block (reduce_emit_* in fq_device.h);
here hand-built slabs go through both (fastp_gpu_debug_stats_fold: the same argument set-up as a launch) and the two
counter blocks must be equal int64 for int64.

Slab counts sit at the edges of both groupings: 1 (a launch this small takes fq_reduce_kernel), 63 / 64 / 65 and 129
around REDUCE_GROUP, on the device also 255 .. 257, 512, 513 and WIDE_PARTS x WIDE_UNROLL consecutive counts, which leave
every wave of the last workgroup row with every remainder of the unrolled loop.  Contents: all zero (nothing may be
added), every field at its maximum in every slab (cnt = q20 = q30 = 16383, qsum = 2^22 - 1, every 5-mer and histogram
dword 0xFFFFFFFF - the slab is all ones, and the sums pass 2^32 from the second slab on), random fields, and one
non-zero slab among zero ones, placed last in a group and in the unroll's remainder.  Contexts: the default (kept ->
POST and PRE), -f 5 -F 3 (front[] shifts the POST cycles and drops those below the front), --merge (slot 3 goes to read
1's POST only).  Every context that has Stats slabs folds them with one_pass set (fastp_gpu.hip: a split plan is a
one-pass plan), so there is no case without it."""
import numpy as np
import pytest

import engines
from fastp_amd import abi

SIM_COUNTS = (1, 30, 63, 64, 65, 107, 129)
GPU_COUNTS = (255, 256, 257, 512, 513)

# name: (params overrides, max_len on the emulator - small, so that 129 slabs stay cheap -, max_len on the device)
CONTEXTS = {
    "default": ({}, 36, 150),
    "front_trim": ({"trim_front1": 5, "trim_front2": 3}, 36, 150),
    "merge": ({"merge": 1, "correction": 1, "cut_right": 1}, 36, 100),
}
CONTENTS = ("zero", "max", "random", "one_slab")


def _params(name, max_len):
    p = abi.default_params(True, max_len)
    for k, v in CONTEXTS[name][0].items():
        setattr(p, k, v)
    return p


def _slabs(content, nb, sd, rng, where=None):
    if content == "zero":
        return np.zeros((nb, sd), dtype=np.uint32)
    if content == "max":
        return np.full((nb, sd), 0xFFFFFFFF, dtype=np.uint32)
    rnd = rng.integers(0, 1 << 32, size=(nb, sd), dtype=np.uint64).astype(np.uint32)
    if content == "random":
        return rnd
    s = np.zeros((nb, sd), dtype=np.uint32)
    s[where] = rnd[where]
    return s


def _fold(g, ptr, nb, which):
    """the context's counter block after a fresh run's worth of the slabs at `ptr` folded by `which`"""
    g.reset()
    info = g.debug_stats_fold(ptr, nb, which)
    g.synchronize()
    return g.counters(), info


def _one_slab_places(nb, info, edges):
    """the last slab of all (in the unroll's remainder of its wave unless that wave's share is whole unrolls) and, at
    the `edges` counts, the last slab of a group of either fold"""
    places = {nb - 1}
    if not edges:
        return [nb - 1]
    for grp in (info["reduce_group"], info["wide_group"]):
        if nb >= grp:
            places.add(grp - 1)
            places.add((nb - 1) // grp * grp - 1 if nb > grp else grp - 1)
    return sorted(p for p in places if 0 <= p < nb)


def check_context(make_engine, ctx_name, max_len, content, counts, run=0):
    """run: also WIDE_PARTS x WIDE_UNROLL consecutive counts"""
    g = make_engine(_params(ctx_name, max_len))
    ptr = 0
    try:
        info = g.debug_stats_fold()
        sd = info["slab_dwords"]
        assert sd == 4 * info["cp"] * 5 * 2 + 4 * 1024 + 4 * 128 and info["c"] <= info["cp"], info
        # consecutive counts: every wave's share of the last group takes every remainder of the unrolled loop
        edges = tuple(counts)
        counts = edges + tuple(range(258, 258 + run * info["wide_parts"] * info["wide_unroll"]))
        g.reset()
        g.synchronize()
        empty = g.counters()
        rng = np.random.default_rng(1234)
        ptr = g.device_alloc(max(counts) * sd * 4)
        for nb in counts:
            for where in (_one_slab_places(nb, info, nb in edges) if content == "one_slab" else [None]):
                slabs = _slabs(content, nb, sd, rng, where)
                g.device_upload(ptr, slabs.tobytes())
                old, i0 = _fold(g, ptr, nb, "groups")
                wide, i1 = _fold(g, ptr, nb, "wide")
                assert i0["last_stats_fold"] == "groups" and i1["last_stats_fold"] == "wide"
                bad = np.nonzero(old != wide)[0]
                assert len(bad) == 0, (f"{ctx_name} / {content} / {nb} slabs (non-zero: {where}): {len(bad)} counters differ, first at "
                                       f"{bad[:6]}: fq_reduce_kernel {old[bad[:6]]} wide {wide[bad[:6]]}")
                if content == "zero":
                    assert np.array_equal(old, empty)
                else:
                    assert not np.array_equal(old, empty), "the fold added nothing: the slabs did not reach it"
                if content == "max" and nb >= 2:
                    assert int(old.max()) > 1 << 32
                auto, ia = _fold(g, ptr, nb, "auto")   # what a launch with this many Stats slabs takes
                assert ia["last_stats_fold"] == ("wide" if nb > info["reduce_group"] else "groups"), (nb, ia)
                assert np.array_equal(auto, old)
    finally:
        if ptr:
            g.device_free(ptr)
        g.close()


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("ctx_name", list(CONTEXTS))
def test_sim_wide_fold_equals_the_group_fold(ctx_name, content):
    check_context(engines.sim_engine, ctx_name, CONTEXTS[ctx_name][1], content, SIM_COUNTS)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_wide_fold_equals_the_group_fold")
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("ctx_name", list(CONTEXTS))
def test_gpu_wide_fold_equals_the_group_fold(ctx_name, content):
    check_context(engines.gpu_engine, ctx_name, CONTEXTS[ctx_name][2], content, SIM_COUNTS + GPU_COUNTS, run=1)
