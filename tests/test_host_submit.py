"""The host submits through the C ABI: fastp_gpu_submit_host_async / fastp_gpu_wait / fastp_gpu_poll - what the drop-in
binding (oracle/patches/gpu_worker.cpp) drives - against fastp_gpu_submit_host, which every parity test goes through.
Characterisation tests: whatever one of the two calls returns the other must return too - records, sparse lists, counts,
counters and error codes - and the slots keep their contract (include/fastp_gpu.h "Pipelined host submits").

Batches of 300, 129 and 1 units of 150 bases: n * 2, n * stride and the record arrays are no multiples of the staging's
256-byte pieces.  What the asynchronous calls read and write lies in page-locked memory of fastp_gpu_host_alloc.  The
test_sim_* cases run on the emulator, the test_gpu_* cases are the same checks on the card."""
import ctypes as C

import numpy as np
import pytest

import cases
import driver
import engines
import golden_util
import synth
from fastp_amd import abi, engine

BATCHES = (300, 129, 1)
EQUAL_CASES = ["pe_default", "pe_correction", "pe_adapter_fasta", "se_adapter_cut", "pe_exotic_default"]
GOLDEN_CASES = ["pe_default", "pe_correction", "se_adapter_cut"]
SLOTS = 4


def sim(params, cls=engine.GpuEngine):
    return cls(params, lib_path=engines.build_sim())


def gpu(params, cls=engine.GpuEngine):
    return cls(params, device=0)


def case_data(name, n=sum(BATCHES)):
    paired, _, pf, skw = cases.CASES[name]
    d = synth.synth_pairs(n, L=150, seed=21, paired=paired, **skw)
    return cases.finalize_params(name, pf(150), d["seq1"], d["len1"], d.get("seq2"), d.get("len2")), d, paired


def pack(eng, d, lo, hi, paired):
    """units lo..hi of d as GpuEngine.process hands them to submit_packed: its positional arguments, and `exotic`"""
    ml, mask = eng.params.max_len, np.zeros(hi - lo, dtype=np.uint8)
    mates = (("seq1", "qual1", "len1"), ("seq2", "qual2", "len2"))[:2 if paired else 1]
    rows = [engine.pack_ascii(eng.lib, ml, *(d[k][lo:hi] for k in m), mask) for m in mates]
    exotic = None
    if mask.any():
        xu = np.flatnonzero(mask).astype(np.int32)
        text = [np.ascontiguousarray(d[m[0]][lo:hi][xu]) for m in mates]
        exotic = (xu, text, [np.arange(len(xu), dtype=np.uint32) * np.uint32(t.shape[1]) for t in text])
    return [a for r in rows for a in r] + [None] * (3 * (2 - len(rows))), exotic


class Staged:
    """One batch and its result block as the C ABI takes them: abi.Batch `b` and abi.Results `res` over page-locked memory
    (pinned) or numpy arrays.  corrections: False leaves the list NULL; corr_capacity: the list's size."""

    def __init__(self, eng, rows, exotic=None, pinned=True, corrections=True, corr_capacity=None, flags=abi.BATCH_STAT_ISIZE):
        self.eng, self.pinned, self.ptrs = eng, pinned, []
        s1, q1, l1, s2, q2, l2 = rows
        n, paired = len(l1), s2 is not None
        self.n, self.paired = n, paired
        b, res = abi.Batch(), abi.Results()
        b.n, b.flags = n, flags
        self.inputs = [self._put(a) if a is not None else None for a in rows]
        b.seq1, b.qual1, b.len1, b.seq2, b.qual2, b.len2 = [a.ctypes.data if a is not None else None for a in self.inputs]
        if exotic is not None:
            xu, xt, xo = exotic
            self.xu = np.ascontiguousarray(xu)          # the unit list is host memory, read during the call
            self.xt, self.xo = [self._put(t) for t in xt], [self._put(o) for o in xo]
            b.n_exotic, b.exotic_unit = len(xu), self.xu.ctypes.data
            for m in range(len(xt)):
                b.exotic_text[m], b.exotic_off[m], b.exotic_text_bytes[m] = self.xt[m].ctypes.data, self.xo[m].ctypes.data, self.xt[m].nbytes
        self.r1 = self._new(n, abi.READ_RESULT_DTYPE)
        self.r2 = self._new(n, abi.READ_RESULT_DTYPE) if paired else None
        self.pr = self._new(n, abi.PAIR_RESULT_DTYPE) if paired else None
        res.r1 = self.r1.ctypes.data
        res.r2, res.pair = (self.r2.ctypes.data, self.pr.ctypes.data) if paired else (None, None)
        self.ncorr, self.nev = C.c_int32(-1), C.c_int32(-1)
        self.corr_capacity = max(1024, n * 32) if corr_capacity is None else corr_capacity
        self.corr = self._new(self.corr_capacity, abi.CORRECTION_DTYPE) if corrections else None
        res.corrections = self.corr.ctypes.data if corrections else None
        res.corrections_capacity = self.corr_capacity
        res.n_corrections = C.addressof(self.ncorr)
        nfasta = int(eng.params.n_adapter_fasta)
        self.ev = self._new(max(16, n * 2 * min(nfasta, 8)) if nfasta else 0, abi.ADAPTER_EVENT_DTYPE)
        if nfasta:
            res.adapter_events, res.adapter_events_capacity = self.ev.ctypes.data, len(self.ev)
            res.n_adapter_events = C.addressof(self.nev)
        self.b, self.res = b, res

    def _new(self, n, dtype):
        if not self.pinned:
            return np.zeros(n, dtype=dtype)
        self.ptrs.append(self.eng.host_alloc(n * np.dtype(dtype).itemsize))
        a = self.eng.host_view(self.ptrs[-1], n, dtype)
        a.view(np.uint8)[:] = 0
        return a

    def _put(self, src):
        src = np.ascontiguousarray(src)
        a = self._new(src.size, src.dtype).reshape(src.shape)
        a[...] = src
        return a

    def submit_host(self):
        return self.eng.lib.fastp_gpu_submit_host(self.eng.h, C.byref(self.b), C.byref(self.res))

    def submit_async(self, slot):
        return self.eng.submit_host_async(self.b, self.res, slot, check=False)

    def results(self):
        """(r1, r2, pair, corrections sorted, adapter events sorted) as copies; the page-locked memory is given back"""
        nc, ne = self.ncorr.value, max(self.nev.value, 0)
        out = (self.r1.copy(), self.r2.copy() if self.paired else None, self.pr.copy() if self.paired else None,
               np.sort(self.corr[:nc].copy(), order=["read", "pos"]) if self.corr is not None else None,
               np.sort(self.ev[:ne].copy(), order=["read", "adapter"]))
        self.free()
        return out

    def free(self):
        for p in self.ptrs:
            self.eng.host_free(p)
        self.ptrs = []


def assert_same(got, want, what):
    assert len(got) == len(want)
    for g, w, part in zip(got, want, ("r1", "r2", "pair", "corrections", "adapter events")):
        if w is None:
            assert g is None, f"{what}: {part}"
        else:
            assert np.array_equal(g, w), f"{what}: {part} differ"


def sync_reference(eng, rows, exotic):
    """the batch through GpuEngine.submit_packed, in the shape of Staged.results"""
    r1, r2, pr, corr = eng.submit_packed(*rows, exotic=exotic)
    return r1, r2, pr, np.sort(corr, order=["read", "pos"]), eng.last_adapter_events


def batches_of(eng, d, paired, sizes=BATCHES):
    lo, out = 0, []
    for n in sizes:
        out.append(pack(eng, d, lo, lo + n, paired))
        lo += n
    return out


# ---- 1. async equals sync, batches in flight ----
def check_async_equals_sync(make, name):
    params, d, paired = case_data(name)
    a, b = make(params), make(params)
    packs = batches_of(a, d, paired)
    want = [sync_reference(a, rows, x) for rows, x in packs]
    staged = [Staged(b, rows, x) for rows, x in packs]
    for slot, st in enumerate(staged):      # all three in flight
        assert st.submit_async(slot) == abi.OK, b.lib.fastp_gpu_last_error(b.h)
    for slot, st in enumerate(staged):
        assert b.wait(slot, check=False) == abi.OK, b.lib.fastp_gpu_last_error(b.h)
    for k, st in enumerate(staged):
        assert_same(st.results(), want[k], f"{name}, batch {k} ({BATCHES[k]} units)")
    if name == "pe_correction":
        assert sum(len(w[3]) for w in want) > 0, "the case made no correction"
    if name == "pe_adapter_fasta":
        assert sum(len(w[4]) for w in want) > 0, "the case made no adapter event"
    ca, cb = a.counters(), b.counters()
    a.close()
    b.close()
    assert np.array_equal(ca, cb), f"{name}: {int((ca != cb).sum())} counters differ"


@pytest.mark.parametrize("name", EQUAL_CASES)
def test_sim_async_equals_sync(name):
    check_async_equals_sync(sim, name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_async_equals_sync")
@pytest.mark.parametrize("name", EQUAL_CASES)
def test_gpu_async_equals_sync(name):
    check_async_equals_sync(gpu, name)


# ---- 2. the goldens through the async path ----
class AsyncEngine(engine.GpuEngine):
    """submit_packed as an asynchronous submit and its wait, on rotating slots"""
    slot = 0

    def submit_packed(self, s1, q1, l1, s2=None, q2=None, l2=None, flags=abi.BATCH_STAT_ISIZE, corr_capacity=None, exotic=None):
        st = Staged(self, [s1, q1, l1, s2, q2, l2], exotic, corr_capacity=corr_capacity, flags=flags)
        slot, self.slot = self.slot, (self.slot + 1) % SLOTS
        self.submit_host_async(st.b, st.res, slot)
        self.wait(slot)
        r1, r2, pr, corr, self.last_adapter_events = st.results()
        return r1, r2, pr, corr


def check_golden(make, name):
    fq1, fq2, meta = golden_util.load(name)
    params = golden_util.params_for(name, max_len=152, fq1=fq1, fq2=fq2)
    eng = make(params, AsyncEngine)
    outs, ctr, rep = driver.run_engine(eng, params, fq1, fq2, umi=golden_util.umi_for(name))
    eng.close()
    golden_util.check_against_golden(name, outs, rep, meta)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_sim_async_matches_reference_golden(name):
    check_golden(sim, name)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_async_matches_reference_golden")
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_gpu_async_matches_reference_golden(name):
    check_golden(gpu, name)


# ---- 3. the slot contract ----
def check_slot_contract(make):
    params, d, paired = case_data("pe_default")
    a, b = make(params), make(params)
    (big, _), (small, _) = batches_of(a, d, paired, (300, 1))
    want_big, want_small = sync_reference(a, big, None), sync_reference(a, small, None)
    for slot in (-1, SLOTS, SLOTS + 1):   # (SLOTS: the context's own slot is not a public one)
        st = Staged(b, small)
        assert st.submit_async(slot) == abi.E_INVALID
        assert b.wait(slot, check=False) == abi.E_INVALID
        assert b.poll(slot) == abi.E_INVALID
        st.free()
    for slot in range(SLOTS):
        assert b.poll(slot) == 1            # free
        assert b.wait(slot, check=False) == abi.OK
    st, late = Staged(b, big), Staged(b, small)
    assert st.submit_async(2) == abi.OK
    assert late.submit_async(2) == abi.E_INVALID   # busy until it has been waited for
    assert b.wait(2, check=False) == abi.OK
    assert_same(st.results(), want_big, "the batch in flight while its slot was asked for again")
    assert b.poll(2) == 1
    assert late.submit_async(2) == abi.OK          # a waited slot takes the next batch
    arrived = 0
    while arrived == 0:
        arrived = b.poll(2)
    assert arrived == 1 and b.poll(2) == 1
    assert_same(late.results(), want_small, "the next batch on the slot")
    # an empty batch: the asynchronous call refuses it, the synchronous one accepts it and reports no correction
    for pinned in (True, False):
        empty = Staged(b, [r[:0] for r in small], pinned=pinned)
        if pinned:
            assert empty.submit_async(0) == abi.E_INVALID
            assert b.poll(0) == 1
        else:
            assert empty.submit_host() == abi.OK
            assert empty.ncorr.value == 0
        empty.free()
    ca, cb = a.counters(), b.counters()
    a.close()
    b.close()
    assert np.array_equal(ca, cb)


def test_sim_slot_contract():
    check_slot_contract(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_slot_contract")
def test_gpu_slot_contract():
    check_slot_contract(gpu)


# ---- 4. a slot's staging grows ----
def check_growth(make):
    params, d, paired = case_data("pe_default")
    a, b = make(params), make(params)
    packs = batches_of(a, d, paired, (1, 300))
    for k, (rows, x) in enumerate(packs):
        want = sync_reference(a, rows, x)
        st = Staged(b, rows, x)
        assert st.submit_async(1) == abi.OK
        assert b.wait(1, check=False) == abi.OK
        assert_same(st.results(), want, f"batch {k} on the one slot")
    ca, cb = a.counters(), b.counters()
    a.close()
    b.close()
    assert np.array_equal(ca, cb)


def test_sim_slot_staging_grows():
    check_growth(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_slot_staging_grows")
def test_gpu_slot_staging_grows():
    check_growth(gpu)


# ---- 5. bad input leaves the engine usable ----
def check_bad_input(make):
    params, d, paired = case_data("pe_default")
    a, b = make(params), make(params)
    (rows, _), = batches_of(a, d, paired, (129,))
    want = sync_reference(a, rows, None)
    for pinned in (True, False):
        bad = Staged(b, rows, pinned=pinned)
        bad.b.seq2 = None
        assert (bad.submit_async(0) if pinned else bad.submit_host()) == abi.E_INVALID
        bad.free()
    st = Staged(b, rows)
    assert st.submit_async(0) == abi.OK
    assert b.wait(0, check=False) == abi.OK
    assert_same(st.results(), want, "the submit after the refused ones")
    ca, cb = a.counters(), b.counters()
    a.close()
    b.close()
    assert np.array_equal(ca, cb)


def test_sim_bad_input_leaves_the_engine_usable():
    check_bad_input(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_bad_input_leaves_the_engine_usable")
def test_gpu_bad_input_leaves_the_engine_usable():
    check_bad_input(gpu)


# ---- 6. a correction list that is too small ----
def check_overflow(make):
    """What both calls guarantee: FASTP_GPU_E_OVERFLOW, n_corrections = the capacity, and that many entries of the list."""
    params, d, paired = case_data("pe_correction")
    a = make(params)
    (rows, _), = batches_of(a, d, paired, (300,))
    full = sync_reference(a, rows, None)[3]
    a.close()
    assert len(full) >= 4, f"the case made {len(full)} corrections"
    cap = len(full) // 2
    members = set(full.tolist())
    for pinned in (True, False):
        b = make(params)
        st = Staged(b, rows, pinned=pinned, corr_capacity=cap)
        if pinned:
            assert st.submit_async(3) == abi.OK
            rc = b.wait(3, check=False)
        else:
            rc = st.submit_host()
        assert rc == abi.E_OVERFLOW
        assert st.ncorr.value == cap
        got = st.results()[3]
        b.close()
        assert len(got) == cap and len(set(got.tolist())) == cap and set(got.tolist()) <= members


def test_sim_correction_list_overflow():
    check_overflow(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_correction_list_overflow")
def test_gpu_correction_list_overflow():
    check_overflow(gpu)


# ---- 7. a -c engine without a correction list ----
def check_null_list(make):
    params, d, paired = case_data("pe_correction")
    a = make(params)
    (rows, _), = batches_of(a, d, paired, (300,))
    want = sync_reference(a, rows, None)
    a.close()
    assert len(want[3]) > 0
    for pinned in (True, False):
        b = make(params)
        st = Staged(b, rows, pinned=pinned, corrections=False)
        if pinned:
            assert st.submit_async(0) == abi.OK
            rc = b.wait(0, check=False)
        else:
            rc = st.submit_host()
        assert rc == abi.OK
        assert st.ncorr.value == 0
        got = st.results()
        b.close()
        assert_same(got[:3], want[:3], "records without a correction list")


def test_sim_no_correction_list():
    check_null_list(sim)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_no_correction_list")
def test_gpu_no_correction_list():
    check_null_list(gpu)
