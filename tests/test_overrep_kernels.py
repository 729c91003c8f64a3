"""The overrepresentation kernels (-p: fq_ovr_pass / scan / tasks / count and the correction-link kernels, fq_device.h)
on hand-built seeds and reads (tests/overrep_util.py), against oraclelib.Oracle: the three result arrays byte for byte
and every counter, overrepresentation counts and `dist` included.  Every family is one list of cases, run as test_sim_*
on the emulator and as its test_gpu_* twin on the device.  Each case first asserts, on the oracle's output alone, that
its input does what it was built for.

a. Table tiers.  ovr_count_body's round-6 branch needs the reads' symbols and every seed table in LDS; otherwise the
   older branch runs, with a table probed in global memory.  launch_overrep gives the kernel 150 KB (aux_lds_cap); the
   symbol rows take (longest read + 4) x 32 bytes - 4,928 at max_len 150, 8,128 at max_len 250 - and a table 8 bytes x the
   power of two >= 4 x seeds: 64 KB up to 2048 seeds, 128 KB up to 4096, 256 KB above.  8,128 + 2 x 65,536 and
   8,128 + 131,072 are within 153,600 and 8,128 + 2 x 131,072 is not, so the tiers of max_len 250 are those of 150:
       seeds per list   paired                                   single-end
       <= 2048          both tables in LDS (the round-6 branch)   in LDS
       2049 .. 4096     read 1's in LDS, read 2's in global       in LDS
       >= 4097          both in global memory                     in global memory
   Which one ran is asked of the engine (debug_overrep_plan), not derived here.
b. Hit rules (stats.cpp:270-288): the window that ends at the read's last base is never examined, a hit continues at
   i + step + 1, `dist` is clipped at the evaluated length, a hit falls on any slide of a four-position trip, and the
   fifth step min(150, eval_len - 2) repeats another step (eval_len 12, 22, 42, 102: both passes count), is below 10,
   or is 0.
c. Probing: seeds that collide into chains and across the table's wrap-around, and windows that are no seeds but land
   on the head of such a chain.
d. Task list and ranks: fq_ovr_tasks' slot arithmetic (per-lane totals 0..4 through ballot bit planes, one atomic per
   workgroup), task_cap reached exactly at sampling 1, the running POST rank across workgroups, launches and batches.
e. Mixed waves: plain units, units with correction chains and units with letters outside ACGTN in one launch, so that
   both ways of staging a read's symbols run and differ between the waves of a workgroup.

Left out: sym_cap == 0 (reads read from global memory, never staged) needs reads longer than 3,836 bases, which no
context accepts; two different windows with one 32-bit key cannot be built at a test's cost - the near-misses (a seed
with one base changed) stand in for them."""
import functools

import numpy as np
import pytest

import engines
import oraclelib
import overrep_util as U
from fastp_amd import abi


class Case:
    def __init__(self, p, batches, paired, floors, plan=None, split=False):
        self.p, self.batches, self.paired, self.floors, self.plan, self.split = p, batches, paired, floors, plan, split


def _args(d, paired):
    return (d["seq1"], d["qual1"], d["len1"]) + ((d["seq2"], d["qual2"], d["len2"]) if paired else ())


@functools.lru_cache(maxsize=None)
def _reference(family, name):
    """the case and the oracle's results for it: computed once, shared by the emulator test and its device twin"""
    c = BUILD[family](name)
    o = oraclelib.Oracle(c.p)
    try:
        ro = [o.process(*_args(b, c.paired)) for b in c.batches]
        co = o.counters()
    finally:
        o.close()
    return c, ro, co, o.layout


def check(family, name, make_engine):
    c, ro, co, lay = _reference(family, name)
    c.floors(ro, co, lay)
    g = make_engine(c.p)
    try:
        rg = [g.process(*_args(b, c.paired)) for b in c.batches]
        cg = g.counters()
        plan = g.debug_overrep_plan()
    finally:
        g.close()
    for bi, (a, b) in enumerate(zip(ro, rg)):
        for k, what in enumerate(("read1 results", "read2 results", "pair results")):
            if a[k] is not None:
                assert b[k].tobytes() == a[k].tobytes(), f"{name}: batch {bi}: {what} differ from the oracle"
    bad = np.nonzero(cg != co)[0]
    assert np.array_equal(cg, co), f"{name}: {len(bad)} counters differ, first at {bad[:8]}: oracle {co[bad[:8]]} engine {cg[bad[:8]]}"
    assert plan["launches"] >= len(c.batches)
    if c.plan is not None:
        assert plan["sym_cap"] == c.p.max_len, f"{name}: {plan}"
        got = tuple(x >= 0 for x in plan["table_lds"])
        assert got == c.plan, f"{name}: seed tables in LDS {got}, the case was written for {c.plan}: {plan}"


def _stats_with_seeds(lay):
    return [s for s in range(4) if int(lay.n_overrep[s]) > 0]


# ---- a. table tiers ---------------------------------------------------------------------------------------------
# name: (paired, max_len, evaluated length, seeds of read 1, seeds of read 2, (read 1's table in LDS, read 2's table in LDS))
TIERS = {}
for _ml in (150, 250):
    TIERS[f"pe_2048_len{_ml}"] = (True, _ml, _ml, 2048, 2048, (True, True))
    TIERS[f"pe_2049_len{_ml}"] = (True, _ml, _ml, 2049, 2049, (True, False))
    TIERS[f"pe_4096_len{_ml}"] = (True, _ml, _ml, 4096, 4096, (True, False))
    TIERS[f"pe_4097_len{_ml}"] = (True, _ml, _ml, 4097, 4097, (False, False))
    TIERS[f"se_4096_len{_ml}"] = (False, _ml, _ml, 4096, 0, (True, False))
    TIERS[f"se_4097_len{_ml}"] = (False, _ml, _ml, 4097, 0, (False, False))
TIERS["pe_4097_and_10"] = (True, 150, 150, 4097, 10, (False, True))
TIERS["pe_10_and_4097"] = (True, 150, 150, 10, 4097, (True, False))
# reads longer than the evaluated length where a table is probed in global memory: that branch's own clip of `dist`
TIERS["pe_2049_len150_eval100"] = (True, 150, 100, 2049, 2049, (True, False))
TIERS["pe_4097_len150_eval100"] = (True, 150, 100, 4097, 4097, (False, False))
TIERS["se_4097_len150_eval100"] = (False, 150, 100, 4097, 0, (False, False))
TIER_UNITS = 240


def build_tier(name):
    paired, ml, ev, n1, n2, plan = TIERS[name]
    rng = np.random.default_rng(1000 + list(TIERS).index(name))
    lists, reads = [], []
    for n in (n1, n2) if paired else (n1,):
        seeds, core = U.seed_list(rng, ev, count=n)
        if n < len(seeds):   # (the short list: structured seeds only)
            seeds = core = sorted(s for s in core if len(s) <= 100)[:n]
        assert len(seeds) == n
        lists.append(seeds)
        reads.append(U.seed_reads(seeds, TIER_UNITS, ml, rng, favoured=core))
    d = U.as_batch(reads[0], reads[1] if paired else None, ml)
    p = U.params(paired, ml, lists[0], lists[1] if paired else [], ev, 3)

    def floors(ro, co, lay):
        ss = _stats_with_seeds(lay)
        assert len(ss) == (4 if paired else 2)
        for s in ss:
            assert int(U.hits(co, lay, s).sum()) >= 100, f"{name}: Stats {s}: {int(U.hits(co, lay, s).sum())} hits"
        passed = int((ro[0][0]["code"] == 0).sum())
        assert 0 < passed < TIER_UNITS   # the POST rank is not the unit index
    return Case(p, [d], paired, floors, plan=plan)


# ---- b. hit rules -----------------------------------------------------------------------------------------------
HIT_LENGTHS = [(150, 150), (150, 102), (102, 102), (60, 42), (40, 22), (30, 12), (30, 7), (30, 3), (30, 2), (150, 100),
               (250, 250), (250, 151)]
HITS = {f"{e}_max{ml}_eval{ev}": (e == "pe", ml, ev) for ml, ev in HIT_LENGTHS for e in ("pe", "se")}


def build_hits(name):
    paired, ml, ev = HITS[name]
    rng = np.random.default_rng(2000 + list(HITS).index(name))
    mates = [U.planted(rng, ml, ev) for _ in range(2 if paired else 1)]
    n = max(len(m[0]) for m in mates)
    for reads, _, marks in mates:
        reads += U.seed_reads([q for q in marks["core"] if b"N" not in q], n - len(reads), ml, rng)
    d = U.as_batch(mates[0][0], mates[1][0] if paired else None, ml)
    p = U.params(paired, ml, mates[0][1], mates[1][1] if paired else [], ev, 1, length_required=min(15, ml // 2))

    def floors(ro, co, lay):
        for m, (_, _, marks) in enumerate(mates):
            assert len(marks["never"]) > 0 and len(marks["last"]) > 0
            for slot in (2 * m, 2 * m + 1):
                h = U.hits(co, lay, slot)
                assert (h[marks["never"]] == 0).all(), f"{name}: a seed at len - step was counted (Stats {slot})"
                if slot == 2 * m:   # (every read reaches the PRE Stats; a unit whose other mate fails a filter skips the POST ones)
                    assert (h[marks["last"]] > 0).all(), f"{name}: a seed at len - step - 1 was not counted (Stats {slot})"
    return Case(p, [d], paired, floors)


# ---- c. probing -------------------------------------------------------------------------------------------------
PROBING = {"pe": True, "se": False}


def build_probing(name):
    paired = PROBING[name]
    rng = np.random.default_rng(3000 + int(paired))
    lists, reads, checks = [], [], []
    for n_seeds in (300, 40) if paired else (300,):
        seeds, decoys = U.probing_list(rng, n_seeds=n_seeds)
        lists.append(seeds)
        reads.append(U.seed_reads(decoys + seeds[:7] + seeds[-20:], 120, 150, rng, favoured=decoys, cut_frac=0.1))
        checks.append((U.table_facts(seeds), U.occupied_first_slot(seeds, decoys), len(decoys)))
    d = U.as_batch(reads[0], reads[1] if paired else None, 150)
    p = U.params(paired, 150, lists[0], lists[1] if paired else [], 150, 1)

    def floors(ro, co, lay):   # (the oracle cannot see the table: the util's own check of what it built)
        for facts, occupied, n_decoys in checks:
            assert facts["longest_probe"] >= 3 and facts["wrapped"] >= 1, facts
            assert occupied == n_decoys >= 20
        for s in _stats_with_seeds(lay):
            assert int(U.hits(co, lay, s)[:7].sum()) >= 20   # the chained seeds themselves are found
    return Case(p, [d], paired, floors)


# ---- d. task list and ranks -------------------------------------------------------------------------------------
TASK_OPTS = {
    "pe": (True, {}, True),
    "se": (False, {}, True),
    "merge": (True, {"merge": 1, "correction": 1}, True),
    "merge_unmerged": (True, {"merge": 1, "correction": 1, "merge_include_unmerged": 1}, True),
    "dedup": (True, {"dedup": 1}, True),
    "pe_nofilter": (True, {}, False),     # every unit passes: four tasks per unit at sampling 1, task_cap reached exactly
    "se_nofilter": (False, {}, False),
}
TASK_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]
TASK_SAMPLINGS = [1, 2, 3, 7, 20, "n1"]   # "n1": n + 1
TASKS = {}
for _oi, _o in enumerate(["pe", "se", "merge", "merge_unmerged", "dedup"]):
    for _ci, _n in enumerate(TASK_COUNTS):
        _s = TASK_SAMPLINGS[(_ci + _oi) % len(TASK_SAMPLINGS)]
        TASKS[f"{_o}_n{_n}_s{_s}"] = (_o, _n, _s, None)
for _o, _n in (("pe_nofilter", 256), ("pe_nofilter", 1025), ("se_nofilter", 257), ("merge", 257), ("dedup", 1025)):
    TASKS[f"{_o}_n{_n}_s1"] = (_o, _n, 1, None)
for _o, _s in (("pe", 3), ("merge_unmerged", 2), ("dedup", 7)):
    TASKS[f"{_o}_n900_s{_s}_batches"] = (_o, 900, _s, (250, 251))
TASK_LEN = 100


def build_tasks(name):
    opt, n, s, cuts = TASKS[name]
    paired, opts, filtered = TASK_OPTS[opt]
    sampling = n + 1 if s == "n1" else s
    rng = np.random.default_rng(4000 + list(TASKS).index(name))
    L = TASK_LEN
    seeds1, core1 = U.seed_list(rng, L, count=60)
    seeds2, core2 = U.seed_list(rng, L, count=60)
    if opts.get("merge"):
        join, po, pr = (U.rand_seq(rng, 20) for _ in range(3))
        seeds1 = seeds1 + [join, po, pr]
        d = U.merge_pairs(rng, n, L, rng.integers(0, 4, size=n), join, po, pr, [q for q in seeds1 if len(q) <= 40])
        seeds2 = U.cut_windows(d, "2", rng)
    else:
        d = U.as_batch(U.seed_reads(seeds1, n, L, rng, favoured=core1, cut_frac=0.0),
                       U.seed_reads(seeds2, n, L, rng, favoured=core2, cut_frac=0.0) if paired else None, L)
    if opts.get("dedup"):
        U.plant_duplicates(d, rng)
    if filtered:
        U.fail_a_third(d, rng, paired, 30)
    p = U.params(paired, L, seeds1, seeds2, L, sampling, length_required=30, **opts)
    edges = [0] + list(cuts or ()) + [n]
    batches = [{k: v[a:b] for k, v in d.items()} for a, b in zip(edges, edges[1:])]

    def floors(ro, co, lay):
        code = np.concatenate([r[0]["code"] for r in ro])
        if paired:
            code = code | np.concatenate([r[1]["code"] for r in ro])
        failed = int((code != 0).sum())
        if not filtered:
            assert failed == 0
        elif n >= 63:
            assert 0.15 * n < failed < 0.6 * n, failed
        if n >= 63:
            flags = np.concatenate([r[0]["flags"] for r in ro])
            if opts.get("dedup"):
                assert int((flags & abi.RF_DUP != 0).sum()) >= 3
            if opts.get("merge"):
                assert int((flags & abi.RF_MERGED != 0).sum()) >= n // 4
            if sampling <= 7:
                for st in _stats_with_seeds(lay):
                    if not (opts.get("merge") and st == 3):   # (merge mode has no POST Stats of read 2 unless unmerged pairs pass)
                        assert int(U.hits(co, lay, st).sum()) > 0, st
    return Case(p, batches, paired, floors, split=cuts is not None)


# ---- e. mixed waves ---------------------------------------------------------------------------------------------
MIXED = {"pe_correction": ({"correction": 1}, 3), "merge": ({"merge": 1, "correction": 1, "merge_include_unmerged": 1}, 2)}
MIXED_UNITS, MIXED_RUN = 384, 32


def build_mixed(name):
    opts, sampling = MIXED[name]
    rng = np.random.default_rng(5000 + list(MIXED).index(name))
    L, n = 150, MIXED_UNITS
    plain, _ = U.seed_list(rng, L, count=40)
    join, po, pr = (U.rand_seq(rng, 20) for _ in range(3))
    # runs of 32 units: plain / with a correction / across the join / plain with letters outside ACGTN
    run_kind = np.arange(n) // MIXED_RUN % 4
    kinds = np.where(run_kind == 0, U.PLAIN, np.where(run_kind == 1, np.where(rng.random(n) < 0.5, U.POST_ONLY, U.PRE_ONLY),
                                                      np.where(run_kind == 2, U.JOIN, U.PLAIN)))
    d = U.merge_pairs(rng, n, L, kinds, join, po, pr, [q for q in plain if len(q) <= 40])
    exotic_units = []
    for a in range(3 * MIXED_RUN, n, 4 * MIXED_RUN):
        U.add_exotic_to(d, a, a + MIXED_RUN, seed=a)
        exotic_units += list(range(a, a + MIXED_RUN))
    sampled = [u for u in exotic_units if u % sampling == 0]   # (cut from units the PRE Stats analyse, so they are hit)
    x1, x2 = U.exotic_seeds(d, sampled, "1", k=8), U.exotic_seeds(d, sampled, "2", k=8)
    assert len(x1) >= 2 and len(x2) >= 2
    seeds1 = [join, po, pr] + sorted(set(plain) | set(x1))
    seeds2 = sorted(set(U.cut_windows(d, "2", rng)) | set(x2))
    p = U.params(True, L, seeds1, seeds2, L, sampling, **opts)

    def floors(ro, co, lay):
        pre1, post1 = U.hits(co, lay, abi.STATS_PRE1), U.hits(co, lay, abi.STATS_POST1)
        assert len(ro[0][3]) >= 60, "corrections"
        assert pre1[0] == 0
        if opts.get("merge"):
            assert post1[0] >= 30, f"{name}: {post1[0]} merged units with a hit across the join"
        assert pre1[1] == 0 and post1[2] == 0
        assert post1[1] + pre1[2] >= 10 and post1[1] > 0 and pre1[2] > 0, (post1[1], pre1[2])
        for st, xs, seeds in ((abi.STATS_PRE1, x1, seeds1), (abi.STATS_PRE2, x2, seeds2)):
            assert sum(int(U.hits(co, lay, st)[seeds.index(q)]) for q in xs) > 0, "a seed with a letter outside ACGTN was hit"
    return Case(p, [d], True, floors)


BUILD = {"tier": build_tier, "hits": build_hits, "probing": build_probing, "tasks": build_tasks, "mixed": build_mixed}


# ---- the emulator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIERS))
def test_sim_table_tiers(name):
    check("tier", name, engines.sim_engine)


@pytest.mark.parametrize("name", list(HITS))
def test_sim_hit_rules(name):
    check("hits", name, engines.sim_engine)


@pytest.mark.parametrize("name", list(PROBING))
def test_sim_probing(name):
    check("probing", name, engines.sim_engine)


@pytest.mark.parametrize("name", list(TASKS))
def test_sim_task_list_and_ranks(name, monkeypatch):
    if TASKS[name][3] is not None:   # the batches' launches split as well: 3 "CUs" x 2 tiles x 32 pairs per launch
        monkeypatch.setenv("FASTP_GPU_TILE", "32")
        monkeypatch.setenv("FASTP_GPU_MAX_TILES_PER_BLOCK", "2")
    check("tasks", name, engines.sim_engine)


@pytest.mark.parametrize("name", list(MIXED))
def test_sim_mixed_waves(name):
    check("mixed", name, engines.sim_engine)


# ---- the device --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.twin("test_sim_table_tiers")
@pytest.mark.parametrize("name", list(TIERS))
def test_gpu_table_tiers(name):
    check("tier", name, engines.gpu_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_hit_rules")
@pytest.mark.parametrize("name", list(HITS))
def test_gpu_hit_rules(name):
    check("hits", name, engines.gpu_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_probing")
@pytest.mark.parametrize("name", list(PROBING))
def test_gpu_probing(name):
    check("probing", name, engines.gpu_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_task_list_and_ranks")
@pytest.mark.parametrize("name", list(TASKS))
def test_gpu_task_list_and_ranks(name):
    check("tasks", name, engines.gpu_engine)


@pytest.mark.gpu
@pytest.mark.twin("test_sim_mixed_waves")
@pytest.mark.parametrize("name", list(MIXED))
def test_gpu_mixed_waves(name):
    check("mixed", name, engines.gpu_engine)
