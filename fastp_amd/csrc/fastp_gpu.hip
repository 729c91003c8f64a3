// fastp_gpu.hip - C ABI of the engine (include/fastp_gpu.h) on the HIP runtime:
// context, HBM buffers, kernel launches.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "fq_device.h"
#include "fq_timeline.h"
#include "fq_stats.h"
#include "fq_stats5.h"
#include "fq_lane.h"
#include "fq_text.h"
#include "fq_inflate.h"
#include "fq_eval.h"
#include "fq_deflate.h"
#include "fq_inflate_wave.h"
#include "fq_host.h"
#include "fq_census.h"

using namespace fq;

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(1024) fq_fused_kernel(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    // read the argument block through the kernarg segment pointer (scalar loads where a field is
    // used) instead of holding all ~150 dwords in SGPRs for the whole persistent loop
    fused_body<false>(*kernel_args(&a), fq_lds);
}
// the per-read kernel of the split plan as one large workgroup per CU (A/B against the small-workgroup form)
extern "C" __global__ void __launch_bounds__(1024) fq_scan_wide_kernel(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    fused_body<true>(*kernel_args(&a), fq_lds);
}
// the per-read kernel of the split plan: 256-lane workgroups, four to a CU (fq_stats_kernel counts afterwards)
extern "C" __global__ void __launch_bounds__(256, 4) fq_scan_kernel(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    fused_body<true>(*kernel_args(&a), fq_lds);
}
// the per-read path with one lane per pair, reads in registers (fq_lane.h): SWM base words per read (10: up to 160
// bases, 16: up to 256), B bloom buffers hashed (0: no hashing in this launch), byte planes per prime, paired / single
#ifndef FQ_LANE_WAVES
#define FQ_LANE_WAVES 3   // wavefronts per SIMD the lane kernel is compiled for (168 VGPRs: no spills; 4 = 128 VGPRs spills ~26 dwords)
#endif
// (reads of up to 256 bases, SWM = 16: the row stage alone is 16 KB per wavefront, two workgroups fit a CU whatever the
// register count - compiled for two wavefronts per SIMD, no spills)
// One workgroup per CU that owns the whole LDS: the tables every wavefront reads (hash planes, counters, LUTs: 12 KB) are then
// held once per CU instead of once per 256-lane workgroup, which is what makes room for twelve wavefronts' row stages PLUS
// read 1's partial quality sums (three 256-lane workgroups of 51 KB fitted, of 56 KB they do not: two per CU, a third of
// the wavefronts gone - profiles/r04_lane_metrics_ab.txt).  FQ_LANE_WAVES wavefronts per SIMD: 168 VGPRs.
template <int SWM> struct LaneGeom { enum { MAX_THREADS = SWM > 10 ? 512 : 256 * FQ_LANE_WAVES }; };
template <int SWM, int B, int NPL, bool PAIRED, int EXT>
__global__ void __launch_bounds__(LaneGeom<SWM>::MAX_THREADS, 1) fq_lane_kernel(LaneArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    lane_body<SWM, B, NPL, PAIRED, EXT>(*kernel_args(&a), fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024, 8) fq_stats_kernel(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
#ifdef FQ_PROFILE_ABLATION
    if ((a.debug_skip & 0x1C0u) && a.kc == 4) { stats_body4<4, true>(a, fq_lds); return; }   // profiling build only (FASTP_GPU_DEBUG_SKIP)
#endif
    if (a.kc == 4) stats_body4<4, false>(a, fq_lds);
    else if (a.kc == 2) stats_body4<2, false>(a, fq_lds);
    else stats_body4<1, false>(a, fq_lds);
}
// form 5 of the Stats kernel (fq_stats5.h): one 1024-lane workgroup per CU that owns the joint table (110 KB at ten item columns).
// A kernel per instantiation of stats_body5 (the host picks one, stats5_inst_for): a kernel is allocated the registers of its
// greediest branch, and as ONE kernel with six branches every launch paid the 128 VGPRs of the ONE / front-trim form - four waves
// per SIMD x 128 = the whole register file, no wave of the tail stream's small kernels got in beside it.  Alone the ONE / no-front
// form (the 2x150 default) takes 118 -> 120: 32 registers per SIMD stay free, a wave of the MISC fold or of Duplicate's losers /
// winners (28 / 22 / 25 VGPRs) fits beside the four.
template <int KC, int HS, bool ABL, bool ONE, bool NF>
__global__ void __launch_bounds__(1024) fq_st5_kernel(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    stats_body5<KC, HS, ABL, ONE, NF>(a, fq_lds);
}
typedef void (*stats5_kernel_fn)(StatsArgs);
// the instantiations the host selects among (fastp_gpu_debug_kernel_regs reports the id)
enum { ST5_ONE_NF = 0, ST5_ONE = 1, ST5_BLOCKS10 = 2, ST5_BLOCKS8 = 3, ST5_ANY_KC2 = 4, ST5_ANY_KC1 = 5, ST5_ABLATION = 6 };
// Do two streams run BESIDE each other?  HIP hands a stream one of a few hardware queues when it is created; two streams of one
// engine can land on the same queue (other engines, torch's and the caller's streams hold the others) and then run one behind the
// other whatever the events between them say - the kernels the engine puts beside the lane / Stats kernels on its second stream (the
// text kernel, Duplicate's tail, the overrepresentation analysis) lost exactly that inside a process that held a second engine
// (profiles/r06_e_*: one soft-masked pair in 1000, 4.48 ms alone, 6.43 ms inside bench.py).  The probe: one kernel on the first
// stream waits (bounded) for a word that a kernel on the second stream sets.
extern "C" __global__ void __launch_bounds__(64) fq_probe_wait_kernel(int* flag, long long budget_cycles) {
#ifndef FQ_HOSTSIM
    if (threadIdx.x == 0) {
        const long long t0 = clock64();
        int seen = 0;
        while (clock64() - t0 < budget_cycles) {
            if (__hip_atomic_load(&flag[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { seen = 1; break; }
            __builtin_amdgcn_s_sleep(16);
        }
        flag[1] = seen;
    }
#else
    (void)flag; (void)budget_cycles;
#endif
}
extern "C" __global__ void __launch_bounds__(64) fq_probe_set_kernel(int* flag) {
    if (threadIdx.x == 0) __hip_atomic_store(&flag[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
extern "C" __global__ void __launch_bounds__(256) fq_front_stats_kernel(FrontStatsArgs c) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    front_stats_body(c, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_hash_kernel(KernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    hash_body(*kernel_args(&a), fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_ovr_pass_kernel(OvrArgs o) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    ovr_pass_body(o, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_ovr_scan_kernel(OvrArgs o, int nblocks) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    ovr_scan_body(o, nblocks, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_ovr_tasks_kernel(OvrArgs o) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    ovr_tasks_body(o, fq_lds);
}
extern "C" __global__ void __launch_bounds__(OVR_BLOCK) fq_ovr_count_kernel(OvrArgs o) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    ovr_count_body(o, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_ovr_corr_link_kernel(OvrArgs o) { ovr_corr_link_body(o); }
extern "C" __global__ void __launch_bounds__(256) fq_parse_count_kernel(ParseArgs p) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    parse_count_body(p, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_parse_scan_kernel(ParseArgs p, int nblocks) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    parse_scan_body(p, nblocks, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_parse_index_kernel(ParseArgs p) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    parse_index_body(p, fq_lds);
}
extern "C" __global__ void __launch_bounds__(64) fq_parse_finish_kernel(ParseArgs p) { parse_finish_body(p); }
extern "C" __global__ void __launch_bounds__(256) fq_parse_pack_kernel(ParseArgs p) { parse_pack_body(p); }
extern "C" __global__ void __launch_bounds__(64) fq_inflate_kernel(InflateArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    inflate_body(a, (u16*)fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_corr_stats_kernel(CorrStatsArgs c) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    corr_stats_body(c, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_corr_link_kernel(OvrArgs o) { corr_link_stride_body(o); }
extern "C" __global__ void __launch_bounds__(256) fq_dedup_apply_kernel(DedupApplyArgs d) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    dedup_apply_body(d, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_dup_final_kernel(DupFinalArgs d) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    dup_final_body(d, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_or_images_kernel(OrArgs o) { or_images_body(o); }
extern "C" __global__ void __launch_bounds__(256) fq_phred64_kernel(Phred64Args a) { phred64_body(a); }
extern "C" __global__ void __launch_bounds__(256) fq_fmt_len_kernel(FmtArgs f) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    fmt_len_body(f, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_fmt_scan_kernel(FmtArgs f) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    fmt_scan_body(f, (u64*)fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_fmt_write_kernel(FmtArgs f) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    fmt_write_body(f, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_fmt_fix_kernel(FmtArgs f) { fmt_fix_body(f); }
extern "C" __global__ void __launch_bounds__(64) fq_inflate_wave_kernel(InflateArgs a) {
    extern __shared__ u32 fq_lds[];
    inflate_wave_body(a, fq_lds);
}
extern "C" __global__ void __launch_bounds__(64) fq_deflate_kernel(DeflateArgs a) {
    extern __shared__ u32 fq_lds[];
    deflate_body<DefLds>(a, fq_lds);
}
// levels 5..9: the chain stage of fq_deflate.h (its own LDS layout, its own blocks per CU)
extern "C" __global__ void __launch_bounds__(64) fq_deflate_chain_kernel(DeflateArgs a) {
    extern __shared__ u32 fq_lds[];
    deflate_body<DefChainLds>(a, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_deflate_scan_kernel(DeflateArgs a) {
    extern __shared__ u32 fq_lds[];
    deflate_scan_body(a, (u64*)fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_deflate_gather_kernel(DeflateArgs a) { deflate_gather_body(a); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_kmer_kernel(EvalKmerArgs a) { eval_kmer_body<false>(a, EvalText{}); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_census_kernel(EvalCensusArgs a) { eval_census_body<false>(a, EvalText{}); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_harvest_kernel(EvalCensusArgs a) { eval_harvest_body(a); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_text_kernel(EvalCensusArgs a) { eval_text_body<false>(a, EvalText{}); }
extern "C" __global__ void __launch_bounds__(64 * EVAL_MATCH_WAVES) fq_eval_match_kernel(EvalMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    eval_match_body(a, fq_lds);
}
extern "C" __global__ void __launch_bounds__(64) fq_eval_replay_kernel(EvalMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    eval_replay_body(a, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_eval_seed_gather_kernel(EvalSeedArgs a) { eval_seed_gather_body<false>(a, EvalText{}); }
extern "C" __global__ void __launch_bounds__(1024) fq_eval_seed_walk_kernel(EvalSeedArgs a) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    eval_seed_walk_body(a, fq_lds);
}
// the text-aware forms (reads with letters outside ACGTN, fastp_gpu_eval_*_x)
extern "C" __global__ void __launch_bounds__(256) fq_eval_list_kernel(EvalListArgs a) { eval_list_body(a); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_kmer_x_kernel(EvalKmerArgs a, EvalText x) { eval_kmer_body<true>(a, x); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_census_x_kernel(EvalCensusArgs a, EvalText x) { eval_census_body<true>(a, x); }
extern "C" __global__ void __launch_bounds__(256) fq_eval_text_x_kernel(EvalCensusArgs a, EvalText x) { eval_text_body<true>(a, x); }
extern "C" __global__ void __launch_bounds__(64 * EVAL_MATCH_WAVES) fq_eval_match_x_kernel(EvalMatchArgs a, EvalText x) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    eval_match_x_body(a, x, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_eval_seed_gather_x_kernel(EvalSeedArgs a, EvalText x) { eval_seed_gather_body<true>(a, x); }
extern "C" __global__ void __launch_bounds__(1024) fq_eval_seed_walk_x_kernel(EvalSeedArgs a, EvalText x) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    eval_seed_walk_x_body(a, x, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_fmts_corr_kernel(FmtsArgs f) { fmts_corr_body(f); }
extern "C" __global__ void __launch_bounds__(256) fq_fmts_len_kernel(FmtsArgs f) {
    extern __shared__ u32 fq_lds[];
    fmts_len_body<FMTS_STREAMS, 2>(f, fq_lds);
}
extern "C" __global__ void __launch_bounds__(1024) fq_fmts_scan_kernel(FmtsArgs f) {
    extern __shared__ u32 fq_lds[];
    fmts_scan_body(f, (u64*)fq_lds);
}
// (six wavefronts per SIMD, i.e. 80 VGPRs, as before the name plan: without the bound the allocator takes 82 - 87 and drops to
// five.  The bound changes the allocation of the options-off path as well - 73 -> 80 VGPRs, 33 -> 50 SGPRs spilled to VGPR lanes;
// what was measured is one shape in one visit, 1 M pairs of 2 x 150 bases: 1.58 - 1.59 ms against the parent's 1.60)
extern "C" __global__ void __launch_bounds__(256, 6) fq_fmts_write_kernel(FmtsArgs f) {
    extern __shared__ u32 fq_lds[];
    fmts_write_body<FMTS_STREAMS, 2>(f, fq_lds);
}
// the same with --overlapped_out's stream: seven streams, up to three emissions per unit (fastp_gpu_format_all_streams;
// fq_fmts_corr_kernel and fq_fmts_scan_kernel serve both, the latter with one workgroup per stream)
extern "C" __global__ void __launch_bounds__(256) fq_fmts7_len_kernel(FmtsArgs f) {
    extern __shared__ u32 fq_lds[];
    fmts_len_body<FMTS_ALL_STREAMS, 3>(f, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256, 6) fq_fmts7_write_kernel(FmtsArgs f) {
    extern __shared__ u32 fq_lds[];
    fmts_write_body<FMTS_ALL_STREAMS, 3>(f, fq_lds);
}
// the adapter census (fq_census.h): a kernel per phase - the boundary is what hands one phase's writes to the next
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_gather_kernel(CsArgs a) { cs_gather_units_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_events_kernel(CsArgs a) { cs_gather_events_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_hash_kernel(CsArgs a) { cs_hash_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_lookup_kernel(CsArgs a) { cs_lookup_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_insert_kernel(CsArgs a) { cs_insert_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_first_kernel(CsArgs a) { cs_first_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_verify_kernel(CsArgs a) { cs_verify_body(a); }
extern "C" __global__ void __launch_bounds__(256) fq_census_hist_kernel(CsArgs a) {
    extern __shared__ u32 fq_lds[];  // 256 dwords: the workgroup's histogram
    cs_hist_body(a, fq_lds);
}
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_admit_kernel(CsArgs a) { cs_admit_body(a); }
extern "C" __global__ void __launch_bounds__(CS_BLOCK) fq_census_pair_kernel(CsArgs a) { cs_pair_verdict_body(a); }
extern "C" __global__ void __launch_bounds__(64 * TEXT_WAVES) fq_text_kernel(TextArgs e) {
    extern __shared__ __attribute__((aligned(16))) u32 fq_lds[];
    text_body(*kernel_args(&e), fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_text_mask_kernel(TextMaskArgs m) { text_mask_body(m); }
extern "C" __global__ void __launch_bounds__(256) fq_reduce_kernel(ReduceArgs r) { reduce_body(r); }
// the Stats fold of a launch with more than REDUCE_GROUP Stats slabs (fold_slabs); runs behind the Stats kernel, not beside it
extern "C" __global__ void __launch_bounds__(WIDE_THREADS) fq_reduce_wide_kernel(ReduceArgs r) {
    extern __shared__ u32 fq_lds[];  // WIDE_LDS_DWORDS: the partial sums of a workgroup's waves
    reduce_wide_body(r, fq_lds);
}
extern "C" __global__ void __launch_bounds__(256) fq_dup_claim_kernel(DupArgs d) { dup_claim_body(d); }
extern "C" __global__ void __launch_bounds__(256) fq_dup_losers_kernel(DupArgs d) { dup_losers_body(d); }
extern "C" __global__ void __launch_bounds__(256) fq_dup_winners_kernel(DupArgs d) { dup_winners_body(d); }
extern "C" __global__ void __launch_bounds__(1024) fq_dup_finish_kernel(DupArgs d) {
    extern __shared__ u32 fq_lds[];  // 1 dword: the workgroup's duplicate count
    dup_finish_body(d, fq_lds);
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

// The FASTP_GPU_* environment switches of this file, read once when a context is created (read_switches).  Each is what a
// test or a tool sets before it creates the engine; DESIGN.md, "Environment switches", has the table.
struct Switches {
    int verbose;              // geometry lines on stderr: tests/test_launch_geometry.py, test_ref_binding.py, bench.py
    int lane;                 // 0 = no lane plan: the parity tests run the tile kernels of the split plan
    int split;                // 0 = Stats inside the fused kernel whatever the options: the parity tests
    int threads;              // workgroup size of the tile kernels (0: 256 split, 1024 fused): the parity tests
    int tile;                 // pairs per tile (0: the largest that fits): the parity tests
    int lds_kb;               // the tile kernels' LDS budget (0: not set): tests/test_launch_geometry.py
    int max_tiles_per_block;  // > 0 caps a launch so that a small batch takes several: the parity tests
    int hash_generic;         // the multiply form of the duplicate hash: tests/test_hostsim_parity.py
    int claim_fused;          // 0 = Duplicate's claim as its own kernel: tests/test_hostsim_parity.py, tools/dup_forms_check.py
    int dedup_fold;           // 0 = --dedup through the hash pre-pass on the lane plan too: tests/test_hostsim_parity.py
    int stats_blocks_per_cu;  // Stats workgroups per CU (0: what fits): tests/test_hostsim_parity.py, tools/two_engine_probe.py
    int exact;                // every unit through the text kernel: tests/test_gpu_parity.py
    int test_merge_slow;      // every merged read's second part counted by the lane kernel: the parity tests
    int inflate;              // FASTP_GPU_INFLATE=lane (1) | wave (2) forces an inflate kernel (0: by size): the parity tests
    int debug_skip;           // FQ_PROFILE_ABLATION builds only (tools/build_ablation.sh, tools/phase_pmc.sh); bench.py refuses it
    int phase_timing;         // per-phase cycle counters: fastp_amd/engine.py, tools/phase_prof.py
    int census_hash_bits;     // FASTP_GPU_DEBUG_CENSUS_HASH_BITS=<k>: the adapter census keeps the low k bits of its hashes, so that
                              // different strings share one (the collision path): tests/test_adapter_census.py
};

// A kernel's dynamic LDS as the context launches it (kernel_lds_table): create refuses a context whose `need` is over the device's
// LDS per workgroup (check_kernel_lds) and sets `set` as the kernel's MaxDynamicSharedMemorySize (set_kernel_attributes).  The two
// differ for the kernels that size their tables to aux_lds_cap at each launch; need = LDS_NO_CHECK: the attribute only.
struct KernelLds { const char* name; const void* fn; long long need; int set; };
constexpr long long LDS_NO_CHECK = 0;

struct fastp_gpu_ctx {
    fastp_gpu_params params;
    Switches sw;
    std::string adapter1, adapter2;
    DevParams dp;
    HostLuts luts;
    TileConfig cfg;
    LdsLayout L;
    fastp_gpu_counter_layout cl;
    int device = 0;
    int cus = 0;
    int lds_bytes = 0;       // the device's LDS per workgroup (hipDeviceProp_t::sharedMemPerBlock): every LDS decision uses it
    int blocks = 0;           // persistent workgroups per launch
    int tiles_per_block = 0;  // tiles a workgroup of the tile kernel takes per launch (its packed per-cycle counters bound it)
    int max_pairs_per_launch = 0;
    std::vector<KernelLds> kernel_lds;   // every kernel with dynamic LDS this context may launch, in the order create checks them
    // split plan (fq_stats.h): the per-read kernel as small workgroups, Stats::statRead as its own streaming kernel
    bool split = false;
    int st_threads = 0, st_blocks = 0;     // the Stats kernel's workgroup size and the most workgroups it is launched with
    int st_lds_dwords = 0, st_slab_dwords = 0;
    u32* d_corr_int = nullptr; size_t corr_int_cap = 0;      // -c on the lane plan: the launch's corrections (KernelArgs::corr_int) + 1 counter word
    u32* d_corr_chain = nullptr; size_t corr_chain_cap = 0;  // their per-read chains: head[reads] | next[capacity]
    int st_form = 4, st_max_reads = CYC_MAX_READS, st_max_grid = 0;   // the Stats kernel's form: 5 (fq_stats5.h) where it fits, else 4 (fq_stats.h)
    stats5_kernel_fn st5_fn = nullptr; int st5_inst = -1;   // form 5: the instantiation this context launches (stats5_inst_for), chosen at create
    int finish_threads = 1024;   // fq_dup_finish_kernel's workgroup: the largest whose waves fit beside the Stats kernel's (choose_finish_threads, at create)
    int last_stats_fold = -1;    // which fold the most recent launch's Stats fold took (FOLD_GROUPS / FOLD_WIDE; -1: none yet)
    // Argument blocks with their constant part filled once (fill_arg_templates, at the end of fastp_gpu_create): a launch copies the
    // block and sets what differs per launch - pointers, n, first, units per block, debug_skip.  The Stats kernel's geometry (H, Hs,
    // kc, H16, its LDS offsets) lives in t_stats only: create's sizing writes it there.
    StatsArgs t_stats = {};
    ReduceArgs t_reduce = {};
    TextCtr t_text_ctr = {};
    LaneArgs t_lane = {};
    FrontStatsArgs t_front = {};
    CorrStatsArgs t_corr = {};
    u32* d_st_slabs = nullptr;
    // lane plan (fq_lane.h): one lane per pair, reads in registers - the option family lane_plan_supported() admits
    bool lane = false;
    int ln_swm = 0, ln_blocks = 0, ln_threads = 256;
    LaneLds ln_lds;
    u32* d_ln_slabs = nullptr;
    // split plans (never null there): Duplicate's losers / winners / finish kernels of a launch run on this stream beside its Stats kernel
    hipStream_t tail = nullptr;
    hipEvent_t ev_k1 = nullptr, ev_tail = nullptr;
    u32* d_swin[2] = {nullptr, nullptr}; size_t swin_cap[2] = {0, 0};
    hipStream_t stream = nullptr;
    // device buffers
    int16_t* d_ov_limit = nullptr;
    u16* d_lowq = nullptr;
    u16* d_cplx = nullptr;
    u32* d_primes = nullptr;
    u32* d_planes = nullptr;  // byte planes of the primes (DevLuts::dup_planes)
    u64* d_posum = nullptr;
    u32* d_fasta_words = nullptr;
    int* d_fasta_len = nullptr;
    std::vector<std::string> fasta_strings;
    std::vector<const char*> fasta_ptrs;
    int64_t* d_ctr = nullptr;
    u32* d_slabs = nullptr;
    int slab_dwords = 0;
    u32* d_bitmap = nullptr;  // Duplicate::mDupBuf as u32 words
    u64* d_dup_pos = nullptr; size_t dup_pos_cap = 0;
    u64* d_table = nullptr; size_t table_cap = 0;
    u8* d_need = nullptr; size_t need_cap = 0;
    u8* d_setw = nullptr; size_t setw_cap = 0;
    u32* d_cfilter = nullptr;
    u8* d_dupflag = nullptr; size_t dupflag_cap = 0;   // --dedup: per-unit duplicate decision
    u32* d_prefix = nullptr;                           // sharded runs: OR of the preceding shards' bitmaps
    bool has_prefix = false;
    bool host_overlapped = false;   // fastp_gpu_host_writes_overlapped: the caller assembles --overlapped_out's stream from the records
    bool fmt_interleaved = false;   // fastp_gpu_format_interleaved: --stdout's one stream for a passing pair
    bool cuts_armed = false;        // fastp_gpu_format_pack_cuts: the plan of the next format call
    fastp_gpu_pack_cuts cuts = {};
    // overrepresentation analysis
    u32* d_ovr_table[2] = {nullptr, nullptr};
    u8* d_ovr_sym[2] = {nullptr, nullptr};
    int* d_ovr_len[2] = {nullptr, nullptr};
    u64* d_post_seen = nullptr;
    u32* d_ovr_work = nullptr; size_t ovr_work_cap = 0;   // blocksum | blockbase | n_tasks | tasks
    int ovr_launches = 0; int ovr_plan[3] = {0, -1, -1};  // launch_overrep's last LDS plan (fastp_gpu_debug_overrep_plan)
    u8* d_def = nullptr; size_t def_cap = 0;              // deflate scratch: member slots | tokens | sizes | offsets | (levels 5..9) chains
    u8* d_eval = nullptr; size_t eval_cap = 0;            // Evaluator pre-pass: census table | hot list | text
    u8* d_eval_x = nullptr; size_t eval_x_cap = 0;        // its text-aware calls: an offset per read | the listed reads
    u32* d_ovr_corr = nullptr; size_t ovr_corr_cap = 0;   // correction chains: head[reads] | next[capacity]
    u32* d_parse = nullptr; size_t parse_cap = 0;         // FASTQ parse scratch
    u64* d_fmt = nullptr; size_t fmt_cap = 0;             // FASTQ format scratch
    u8* d_inf = nullptr; size_t inf_cap = 0;              // inflate scratch: code lengths | status | first_bad
    uint64_t units_seen = 0;                               // units submitted so far (the pre-filtering Stats' mReads)
    const void* last_corr = nullptr; int32_t last_corr_cap = 0;   // the correction list of the last submit and its capacity
    std::vector<std::string> ovr_strings[2];
    std::vector<const char*> ovr_ptrs[2];
    // exact plan (fq_text.h): the worker loop on the text, for units with letters outside ACGTN
    bool exact_all = false;                                // FASTP_GPU_EXACT=1: every unit takes it (tests)
    int* d_x_unit = nullptr; size_t x_unit_cap = 0;        // the submitted batch's exotic unit list
    u8* d_x_skip = nullptr; size_t x_skip_cap = 0;          // KernelArgs::xskip of the launch
    u32* d_al[4] = {nullptr, nullptr, nullptr, nullptr}; size_t al_cap[4] = {0, 0, 0, 0};   // merge mode: 16-byte aligned copies of a launch's rows
    u16* d_x_len = nullptr; size_t x_len_cap = 0;          // the launch's length arrays with the text kernel's units zeroed (what the plan's kernels see)
    void* d_x_text[2] = {nullptr, nullptr}; size_t x_text_cap[2] = {0, 0};   // host submits: the raw text + offsets staged in HBM
    void* d_x_off[2] = {nullptr, nullptr}; size_t x_off_cap[2] = {0, 0};
    std::vector<int32_t> parse_exotic;                     // records of the last fastp_gpu_parse_fastq call with letters outside ACGTN
    // host submits: device staging, completion event and what to finish per slot.  The public slots, then the one
    // fastp_gpu_submit_host uses (no slot number reaches it)
    struct AsyncSlot {
        void* d_stage = nullptr; size_t cap = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
        int32_t* counts = nullptr;            // pinned: n_corrections, n_adapter_events as the device left them
        fastp_gpu_results res;                // the caller's result block (host pointers)
        const void* d_corr = nullptr;         // the batch's sparse lists in the slot's device staging: copied out when the batch
        const void* d_ev = nullptr;           // has arrived, as many entries as were written (not their whole capacity per batch)
        hipStream_t copy = nullptr;
    } aslot[FASTP_GPU_ASYNC_SLOTS + 1];
    u64* d_phase = nullptr;   // optional per-phase cycle counters (FASTP_GPU_PHASE_TIMING=1)
    // adapter census (fq_census.h): FilterResult::mAdapter1 / mAdapter2 as two persistent tables, allocated at the first use
    u8* d_cs_map[2] = {nullptr, nullptr};
    CsMap cs_map[2] = {};
    u32 cs_entries[2] = {0, 0};                             // host mirror of the tables' sizes
    u8* d_cs_blob = nullptr;                                // adapter sequences as bytes | offsets | lengths
    u8* d_cs_items = nullptr; size_t cs_items_cap = 0;      // a launch's item list | counters | select histogram
    u8* d_cs_slots = nullptr; size_t cs_slots_cap = 0;      // a launch's dedupe table
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_events;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
    double kernel_ms = 0.0;
    int64_t kernel_launches = 0;
    std::string err;
};

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            std::string m_ = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            if (ctx) (ctx)->err = m_;                                                           \
            g_last_error = m_;                                                                  \
            return FASTP_GPU_E_HIP;                                                             \
        }                                                                                       \
    } while (0)

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

static Switches read_switches() {
    Switches w;
    w.verbose = env_int("FASTP_GPU_VERBOSE", 0);
    w.lane = env_int("FASTP_GPU_LANE", 1);
    w.split = env_int("FASTP_GPU_SPLIT", 1);
    w.threads = env_int("FASTP_GPU_THREADS", 0);
    w.tile = env_int("FASTP_GPU_TILE", 0);
    w.lds_kb = env_int("FASTP_GPU_LDS_KB", 0);
    w.max_tiles_per_block = env_int("FASTP_GPU_MAX_TILES_PER_BLOCK", 0);
    w.hash_generic = env_int("FASTP_GPU_HASH_GENERIC", 0);
    w.claim_fused = env_int("FASTP_GPU_CLAIM_FUSED", 1);
    w.dedup_fold = env_int("FASTP_GPU_DEDUP_FOLD", 1);
    w.stats_blocks_per_cu = env_int("FASTP_GPU_STATS_BLOCKS_PER_CU", 0);
    w.exact = env_int("FASTP_GPU_EXACT", 0);
    w.test_merge_slow = env_int("FASTP_GPU_TEST_MERGE_SLOW", 0);
    const char* how = getenv("FASTP_GPU_INFLATE");
    w.inflate = !how ? 0 : !strcmp(how, "lane") ? 1 : !strcmp(how, "wave") ? 2 : 3;   // (3: a word that is neither - the wave kernel where it fits)
    w.debug_skip = env_int("FASTP_GPU_DEBUG_SKIP", 0);
    w.phase_timing = env_int("FASTP_GPU_PHASE_TIMING", 0);
    w.census_hash_bits = env_int("FASTP_GPU_DEBUG_CENSUS_HASH_BITS", 0);
    return w;
}

static int fail(fastp_gpu_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    g_last_error = msg;
    return code;
}

extern "C" const char* fastp_gpu_last_error(const fastp_gpu_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

static void drain_events(fastp_gpu_ctx* ctx) {
    for (auto& pr : ctx->pending_events) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            ctx->kernel_ms += ms;
            ctx->kernel_launches += 1;
        }
        ctx->free_events.push_back(pr);
    }
    ctx->pending_events.clear();
}

// set by fq_comm.cpp once a communicator exists: lets fastp_gpu_destroy drop the context's rank
extern "C" { void (*fastp_gpu_comm_destroy_hook)(fastp_gpu_ctx*) = nullptr; }

extern "C" void fastp_gpu_destroy(fastp_gpu_ctx* ctx) {
    if (!ctx) return;
    if (fastp_gpu_comm_destroy_hook) fastp_gpu_comm_destroy_hook(ctx);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    drain_events(ctx);
    for (auto& sl : ctx->aslot) {
        if (sl.d_stage) (void)hipFree(sl.d_stage);
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.copy) (void)hipStreamDestroy(sl.copy);
        if (sl.counts) (void)hipHostFree(sl.counts);
    }
    for (auto& pr : ctx->free_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    void* bufs[] = {ctx->d_ov_limit, ctx->d_lowq, ctx->d_cplx, ctx->d_primes, ctx->d_planes, ctx->d_posum, ctx->d_fasta_words, ctx->d_fasta_len, ctx->d_ctr, ctx->d_slabs,
                    ctx->d_bitmap, ctx->d_dup_pos, ctx->d_table, ctx->d_need, ctx->d_dupflag, ctx->d_phase,
                    ctx->d_ovr_table[0], ctx->d_ovr_table[1], ctx->d_ovr_sym[0], ctx->d_ovr_sym[1], ctx->d_ovr_len[0],
                    ctx->d_ovr_len[1], ctx->d_post_seen, ctx->d_ovr_work, ctx->d_parse, ctx->d_fmt, ctx->d_prefix, ctx->d_inf, ctx->d_ovr_corr, ctx->d_eval, ctx->d_eval_x, ctx->d_def, ctx->d_setw, ctx->d_cfilter,
                    ctx->d_st_slabs, ctx->d_swin[0], ctx->d_swin[1], ctx->d_ln_slabs,
                    ctx->d_cs_map[0], ctx->d_cs_map[1], ctx->d_cs_blob, ctx->d_cs_items, ctx->d_cs_slots,
                    ctx->d_corr_int, ctx->d_corr_chain, ctx->d_x_unit, ctx->d_x_len, ctx->d_x_skip, ctx->d_al[0], ctx->d_al[1], ctx->d_al[2], ctx->d_al[3], ctx->d_x_text[0], ctx->d_x_text[1], ctx->d_x_off[0], ctx->d_x_off[1]};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->tail) (void)hipStreamDestroy(ctx->tail);
    if (ctx->ev_k1) (void)hipEventDestroy(ctx->ev_k1);
    if (ctx->ev_tail) (void)hipEventDestroy(ctx->ev_tail);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// The LDS layout of form 5 of the Stats kernel (fq_stats5.h) with hb table columns and kc copies of the 5-mer counters: the joint
// table [2][8][4][ST5_QN][hb] of 16-bit cell pairs, kc copies of the mate's 5-mer counters, the packed cells of what the table has
// no cell for, the histogram of those, a list per wavefront.  Writes the dword offsets into sa and returns the total: the one
// statement of the layout, for the fit test (stats5_copies) and for the context's kernel (plan_stats_kernel) alike.
static int stats5_lds_layout(StatsArgs& sa, int Cp, int hb, int kc) {
    int o = 0;
    sa.l_cyc = o; o += 2 * 8 * 4 * ST5_QN * hb;
    sa.l_kmer = o; o += 2 * KMER_BINS * kc;
    o = (o + 1) & ~1;
    sa.l_ovf = o; o += 2 * Cp * N_CLS * 2;
    sa.l_qh = o; o += 2 * 128;
    sa.l_wl = o; o += (1024 / 64) * 2 * ST5_WL / 2;   // (u16 entries)
    return o;
}
// The LDS layout of form 4 (fq_stats.h): [2][8][ST4_ROWS][Hs] u32 per-cycle cells of ONE mate, four copies of its 5-mer counters,
// its histogram; the class stride padded to 32 items (= all 64 banks).  Shrinks sa.Hs, then sa.kc, until two workgroups fit a CU
// (or nothing is left to shrink); writes the dword offsets into sa and returns the total.
static int stats4_lds_layout(StatsArgs& sa, int lds_bytes) {
    sa.kc = 4;
    sa.Hs = sa.H < 32 ? 32 : sa.H;
    for (;;) {
        sa.wl_cap = 511;
        int o = 0;
        sa.l_cyc = o; o += 2 * 8 * ST4_ROWS * sa.Hs;
        sa.l_kmer = o; o += 2 * KMER_BINS * sa.kc;
        sa.l_qh = o; o += ST_QH_COPIES * 2 * 128;
        o = (o + 3) & ~3;
        sa.l_lut = o; o += 4 * 256;
        sa.l_mt = o; o += 18 + 2;
        sa.l_wl = o; o += 1 + sa.wl_cap;
        if (2 * o * 4 <= lds_bytes) return o;   // two workgroups per CU
        if (sa.Hs > sa.H) sa.Hs = sa.H;         // first the padding,
        else if (sa.kc > 1) sa.kc /= 2;         // then the copies
        else return o;
    }
}
// form 5 of the Stats kernel: the copies of the 5-mer table its LDS layout has room for (0: it does not fit)
// (and, through hb, the columns its table holds: reads with more 16-base columns than fit are taken in blocks of hb columns;
// reads of up to 176 bases fit one workgroup's LDS whole; merge mode's third pass exists in form 4 only)
static int stats5_copies(const DevParams& p, int lds_bytes, int* hb_out = nullptr) {
    if (p.merge_lane) return 0;
    const int H16 = (p.qw_g + 3) / 4, Cp = (p.cycles + 3) & ~3;
    if (H16 > p.sw_g || H16 > 64) return 0;
    StatsArgs probe = {};
    for (int nblk = 1; nblk <= 4; nblk++) {
        const int hb = (H16 + nblk - 1) / nblk;
        for (int kc = 2; kc >= 1; kc--)
            if (stats5_lds_layout(probe, Cp, hb, kc) * 4 <= lds_bytes) {
                if (hb_out) *hb_out = hb;
                return kc;
            }
    }
    return 0;
}
// which instantiation of form 5 a context launches: everything it depends on is fixed at fastp_gpu_create (the table's columns
// and copies, the reads' columns, whether any front trim exists).  ONE: the table holds every column of the reads; NF: no front
// trim of any kind, no result record read.
static int stats5_inst_for(int Hs, int kc, int H16, bool nofront) {
    if (Hs == 10 && kc == 2 && H16 <= 10) return nofront ? ST5_ONE_NF : ST5_ONE;   // reads of up to 160 bases
    if (Hs == 10 && kc == 2) return ST5_BLOCKS10;
    if (Hs == 8 && kc == 2) return ST5_BLOCKS8;    // two blocks of eight columns: reads of up to 256 bases
    return kc == 2 ? ST5_ANY_KC2 : ST5_ANY_KC1;
}
static stats5_kernel_fn stats5_kernel_for(int inst) {
    switch (inst) {
        case ST5_ONE_NF: return fq_st5_kernel<2, 10, false, true, true>;
        case ST5_ONE: return fq_st5_kernel<2, 10, false, true, false>;
        case ST5_BLOCKS10: return fq_st5_kernel<2, 10, false, false, false>;
        case ST5_BLOCKS8: return fq_st5_kernel<2, 8, false, false, false>;
        case ST5_ANY_KC2: return fq_st5_kernel<2, 0, false, false, false>;
        case ST5_ANY_KC1: return fq_st5_kernel<1, 0, false, false, false>;
#ifdef FQ_PROFILE_ABLATION
        case ST5_ABLATION: return fq_st5_kernel<2, 10, true, false, false>;   // profiling build only (FASTP_GPU_DEBUG_SKIP)
#endif
    }
    return nullptr;
}
static bool stats5_no_front(const DevParams& p) {
    return !p.front_per_read && !(p.front_lane && (p.lane_front1 != 0 || p.lane_front2 != 0));
}
// the option family the lane kernel covers: nothing moves or edits a kept base (split plan), no step that needs an
// unbounded indexed walk along a read (adapter sequences, one-gap overlap, polyX, complexity), windows of up to 8
// bases, reads of up to 256 bases, a duplicate hash with the byte-plane table and 3-byte primes
static bool lane_plan_supported(const DevParams& p, const HostLuts& luts, int lds_bytes) {
    if (p.front_per_read && !stats5_copies(p, lds_bytes)) return false;   // a front per read: form 5 of the Stats kernel only
    if (!(p.stats_one_pass || p.front_lane || p.corr_lane || p.merge_lane) || p.allow_gap || p.overlapped_out) return false;
    if (p.n_fasta && p.fasta_max_len > 64) return false;   // (--adapter_fasta: each sequence like -a, in four uniform words)
    if (p.merge && !p.merge_lane) return false;
    if ((p.has_a1 && p.alen1 > 64) || (p.has_a2 && p.alen2 > 64)) return false;   // the lane kernel keeps an adapter in four uniform words
    if (p.max_len > 256 || p.sw_g > 16 || (p.qw_g & 1)) return false;
    if (p.cut_right && (p.wR < 1 || p.wR > 8)) return false;
    if (p.cut_tail && !p.cut_right && (p.wT < 1 || p.wT > 8)) return false;
    if (p.dup_enabled && !(luts.dup_nq > 0 && (p.dup_bufnum == 2 || p.dup_bufnum == 4) && p.dup_npl == 3)) return false;
    return true;
}

// the dynamic LDS the overrepresentation count and text kernels may take (they size their tables to it at each launch)
static int aux_lds_cap(const fastp_gpu_ctx* ctx) { return std::min(150 * 1024, ctx->lds_bytes); }
// the dynamic LDS of the kernels whose size is a formula: create's check, the attribute and the launch all ask here
// (DevParams::cycles and the counter layout's cycles are both fastp_gpu_cycles_for of the context's parameters)
static size_t front_stats_lds_bytes(const fastp_gpu_ctx* ctx) { return (size_t)(ctx->dp.paired ? 2 : 1) * 34 * (size_t)ctx->dp.cycles * 4; }
static size_t corr_stats_lds_bytes(const fastp_gpu_ctx* ctx) {
    return (size_t)(ctx->dp.paired ? 2 : 1) * (33 * (size_t)ctx->dp.cycles + 128 + KMER_BINS) * 4;
}
static int inflate_lane_lds_bytes() { return INF_ENTRIES * INF_LANES * 2 + INF_SBUF * INF_LANES * 4; }
// the tile kernel of the context's plan, and what create's messages call it
static const void* tile_kernel_for(const fastp_gpu_ctx* ctx, const char** name = nullptr) {
    const bool wide = ctx->cfg.threads > 256;
    if (name) *name = ctx->split ? (wide ? "scan_wide kernel" : "scan kernel") : "fused kernel";
    return ctx->split ? (wide ? (const void*)fq_scan_wide_kernel : (const void*)fq_scan_kernel) : (const void*)fq_fused_kernel;
}

typedef void (*lane_kernel_fn)(LaneArgs);
template <int EXT>
static lane_kernel_fn lane_kernel_pick(int swm, int B, bool paired) {
    if (swm == 10) {
        if (B == 0) return paired ? fq_lane_kernel<10, 0, 3, true, EXT> : fq_lane_kernel<10, 0, 3, false, EXT>;
        if (B == 2) return paired ? fq_lane_kernel<10, 2, 3, true, EXT> : fq_lane_kernel<10, 2, 3, false, EXT>;
        return paired ? fq_lane_kernel<10, 4, 3, true, EXT> : fq_lane_kernel<10, 4, 3, false, EXT>;
    }
    if (B == 0) return paired ? fq_lane_kernel<16, 0, 3, true, EXT> : fq_lane_kernel<16, 0, 3, false, EXT>;
    if (B == 2) return paired ? fq_lane_kernel<16, 2, 3, true, EXT> : fq_lane_kernel<16, 2, 3, false, EXT>;
    return paired ? fq_lane_kernel<16, 4, 3, true, EXT> : fq_lane_kernel<16, 4, 3, false, EXT>;
}
// ext: 1 = adapter sequences, polyX trimming or the complexity filter are on (the instantiation that carries those steps);
// 2 = a front trim or -c as well (round 5; an instantiation of its own: with their code in it the first one spilled 77 dwords)
// 3 = --merge as well (paired only)
static int lane_ext(const DevParams& p) {
    if (p.merge_lane) return 3;
    if (p.front_lane || p.corr_lane) return 2;
    return (p.has_a1 || p.has_a2 || p.n_fasta || p.poly_x || p.complexity_filter) ? 1 : 0;
}
static lane_kernel_fn lane_kernel_merge(int swm, int B) {
    if (swm == 10) return B == 0 ? fq_lane_kernel<10, 0, 3, true, 3> : B == 2 ? fq_lane_kernel<10, 2, 3, true, 3> : fq_lane_kernel<10, 4, 3, true, 3>;
    return B == 0 ? fq_lane_kernel<16, 0, 3, true, 3> : B == 2 ? fq_lane_kernel<16, 2, 3, true, 3> : fq_lane_kernel<16, 4, 3, true, 3>;
}
static lane_kernel_fn lane_kernel_for(int swm, int B, bool paired, int ext) {
    if (ext == 3) return lane_kernel_merge(swm, B);
    return ext == 2 ? lane_kernel_pick<2>(swm, B, paired) : ext == 1 ? lane_kernel_pick<1>(swm, B, paired) : lane_kernel_pick<0>(swm, B, paired);
}

// The constant part of the argument blocks a launch fills (ctx->t_*): the counter layout, the options and the Stats kernel's
// geometry - nothing of it changes after fastp_gpu_create.
static void fill_arg_templates(fastp_gpu_ctx* ctx) {
    const fastp_gpu_counter_layout& cl = ctx->cl;
    const DevParams& dp = ctx->dp;
    TextCtr& c = ctx->t_text_ctr;
    c.filter = cl.filter_stats; c.adapter_reads = cl.adapter_reads; c.adapter_bases = cl.adapter_bases;
    c.polyx_reads = cl.polyx_reads; c.polyx_bases = cl.polyx_bases; c.correction = cl.correction;
    c.corrected_reads = cl.corrected_reads; c.merged = cl.merged_pairs; c.isize = cl.isize;
    for (int k = 0; k < 4; k++) c.stats[k] = cl.stats[k];
    c.st_reads = cl.st_reads; c.st_length_sum = cl.st_length_sum; c.st_qual_hist = cl.st_qual_hist;
    c.st_kmer = cl.st_kmer; c.st_cycle = cl.st_cycle; c.cycles = cl.cycles;
    ReduceArgs& r = ctx->t_reduce;
    r.L = ctx->L;
    r.isize_max = dp.isize_max;
    r.one_pass = dp.stats_one_pass || (ctx->split && (dp.front_lane || dp.corr_lane || dp.merge_lane));
    r.merge_tail = (ctx->split && dp.merge_lane) ? 1 : 0;
    if (ctx->split && dp.front_lane) { r.front[0] = dp.lane_front1; r.front[1] = dp.lane_front2; }
    r.ctr = ctx->d_ctr;
    r.o_filter = cl.filter_stats; r.o_adapter_reads = cl.adapter_reads; r.o_adapter_bases = cl.adapter_bases;
    r.o_polyx_reads = cl.polyx_reads; r.o_polyx_bases = cl.polyx_bases; r.o_correction = cl.correction;
    r.o_corrected_reads = cl.corrected_reads; r.o_merged = cl.merged_pairs; r.o_isize = cl.isize;
    for (int s = 0; s < 4; s++) r.o_stats[s] = cl.stats[s];
    r.st_reads = cl.st_reads; r.st_length_sum = cl.st_length_sum; r.st_qual_hist = cl.st_qual_hist;
    r.st_kmer = cl.st_kmer; r.st_cycle = cl.st_cycle; r.cycles = cl.cycles;
    if (!ctx->split) return;
    StatsArgs& sa = ctx->t_stats;   // (H, Hs, kc, H16 and the LDS offsets: set where create chose the kernel's form)
    sa.paired = dp.paired; sa.sw_g = dp.sw_g; sa.qw_g = dp.qw_g;
    sa.magic_H = magic_for((u32)sa.H);
    sa.Cp = ctx->L.Cp;
    if (dp.front_lane) { sa.front[0] = dp.lane_front1; sa.front[1] = dp.lane_front2; }
    sa.merge = dp.merge_lane;
    sa.l_total = ctx->st_lds_dwords;
    sa.magic_H16 = (ctx->st_form == 5 && sa.Hs) ? magic_for((u32)sa.Hs) : 0u;   // (the magic of the table's columns)
    sa.front_per_read = dp.front_per_read; sa.fr_stride = dp.front_per_read ? 3 : 0;
    sa.slabs = ctx->d_st_slabs; sa.slab_dwords = ctx->st_slab_dwords;
    LaneArgs& la = ctx->t_lane;
    la.l = ctx->ln_lds;
    la.post1 = ctx->d_ctr + cl.stats[1];
    la.st_qual_hist = cl.st_qual_hist; la.st_kmer = cl.st_kmer; la.st_cycle = cl.st_cycle; la.cycles = cl.cycles;
    FrontStatsArgs& fs = ctx->t_front;
    CorrStatsArgs& cs = ctx->t_corr;
    fs.paired = cs.paired = dp.paired;
    fs.sw_g = cs.sw_g = dp.sw_g;
    fs.qw_g = cs.qw_g = dp.qw_g;
    for (int m = 0; m < 2; m++) {
        fs.post[m] = ctx->d_ctr + cl.stats[2 * m + 1];
        cs.post[m] = ctx->d_ctr + cl.stats[dp.merge_lane ? 1 : 2 * m + 1];
    }
    fs.front0[0] = dp.lane_front1; fs.front0[1] = dp.lane_front2;
    fs.st_cycle = cl.st_cycle; fs.cycles = cl.cycles;
    cs.merge = dp.merge_lane;
    cs.front[0] = dp.front_lane ? dp.lane_front1 : 0; cs.front[1] = dp.front_lane ? dp.lane_front2 : 0;
    cs.st_qual_hist = cl.st_qual_hist; cs.st_kmer = cl.st_kmer; cs.st_cycle = cl.st_cycle; cs.cycles = cl.cycles;
}

// debugging aid: what the runtime allocates the Stats kernel this context launches and the tail stream's small kernels -
// out[0] the instantiation of form 5 (ST5_*; -1: form 4), then {VGPRs, max threads per workgroup, static LDS bytes} of the
// Stats kernel, fq_reduce_kernel, fq_dup_losers_kernel, fq_dup_winners_kernel, fq_dup_finish_kernel.  Whether a wave of a tail
// kernel fits beside the Stats kernel's four per SIMD is arithmetic on these (granules of 8 of a 512-entry file per SIMD).
// The emulator has no such attributes: zeros behind out[0].
enum { KERNEL_REGS_N = 16 };
extern "C" int fastp_gpu_debug_kernel_regs(fastp_gpu_ctx* ctx, int32_t* out, int32_t n) {
    if (!ctx || !out || n < KERNEL_REGS_N) return FASTP_GPU_E_INVALID;
    for (int i = 0; i < n; i++) out[i] = 0;
    out[0] = ctx->split && ctx->st_form == 5 ? ctx->st5_inst : -1;
#ifndef FQ_HOSTSIM
    const void* fns[5] = {ctx->st_form == 5 && ctx->st5_fn ? (const void*)ctx->st5_fn : (const void*)fq_stats_kernel, (const void*)fq_reduce_kernel,
                          (const void*)fq_dup_losers_kernel, (const void*)fq_dup_winners_kernel, (const void*)fq_dup_finish_kernel};
    for (int k = 0; k < 5; k++) {
        hipFuncAttributes fa;
        HIP_TRY(ctx, hipFuncGetAttributes(&fa, fns[k]));
        out[1 + 3 * k] = fa.numRegs;
        out[2 + 3 * k] = fa.maxThreadsPerBlock;
        out[3 + 3 * k] = (int32_t)fa.sharedSizeBytes;
    }
#endif
    return FASTP_GPU_OK;
}

// ---------------------------------------------------------------------------
// fastp_gpu_create, step by step.  Every step is `static int step(fastp_gpu_ctx*)`: it returns a FASTP_GPU_* code and leaves its
// message through fail() / HIP_TRY.  fastp_gpu_create owns the context from `new` to its last line, so a step that fails just
// returns: whatever the steps before it made goes with the context (fastp_gpu_destroy).
// ---------------------------------------------------------------------------

// own copies of the strings ctx->params points to: the caller's may go away
static int own_param_strings(fastp_gpu_ctx* ctx) {
    fastp_gpu_params& p = ctx->params;
    if (p.adapter_seq_r1) ctx->adapter1 = p.adapter_seq_r1;
    if (p.adapter_seq_r2) ctx->adapter2 = p.adapter_seq_r2;
    p.adapter_seq_r1 = ctx->adapter1.c_str();
    p.adapter_seq_r2 = ctx->adapter2.c_str();
    if (p.n_adapter_fasta > 0 && p.adapter_fasta) {
        for (int i = 0; i < p.n_adapter_fasta; i++) ctx->fasta_strings.push_back(p.adapter_fasta[i] ? p.adapter_fasta[i] : "");
        for (auto& f : ctx->fasta_strings) ctx->fasta_ptrs.push_back(f.c_str());
        p.adapter_fasta = ctx->fasta_ptrs.data();
    }
    if (p.overrep_enabled) {  // the seed strings
        const char* const* lists[2] = {p.overrep_seqs1, p.overrep_seqs2};
        const int ns[2] = {p.n_overrep_seqs1, p.n_overrep_seqs2};
        for (int m = 0; m < 2; m++) {
            for (int i = 0; i < ns[m] && lists[m]; i++) ctx->ovr_strings[m].push_back(lists[m][i] ? lists[m][i] : "");
            for (auto& q : ctx->ovr_strings[m]) ctx->ovr_ptrs[m].push_back(q.c_str());
        }
        p.overrep_seqs1 = ctx->ovr_ptrs[0].data();
        p.overrep_seqs2 = ctx->ovr_ptrs[1].data();
    }
    return 0;
}

// the options as the device code takes them (fq_host.cpp) and the device's properties
static int read_params_and_device(fastp_gpu_ctx* ctx) {
    std::string err;
    const int rc = build_dev_params(ctx->params, ctx->dp, ctx->luts, err);
    if (rc) return fail(ctx, rc, err);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, FASTP_GPU_E_HIP, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return fail(ctx, FASTP_GPU_E_HIP, "hipGetDeviceProperties failed");
    ctx->cus = prop.multiProcessorCount;
    ctx->lds_bytes = (int)std::min<size_t>(prop.sharedMemPerBlock, (size_t)1 << 30);
    return 0;
}

// The plan and the tile kernel's geometry (tunable without a rebuild).
// The split plan (per-read kernel as 256-lane workgroups, several per CU, + the streaming Stats kernel) whenever no
// option moves or edits a kept base; FASTP_GPU_SPLIT=0 keeps Stats inside the one-workgroup-per-CU fused kernel.
// the Stats kernel as its own launch: options that leave every kept base where it was, or (lane plan only) move it by the
// same front for every read that is written out (DevParams::front_lane)
static int choose_plan(fastp_gpu_ctx* ctx) {
    const Switches& sw = ctx->sw;
    const int lds_max = ctx->lds_bytes;
    const int lds_kb_default = lds_max / 1024 >= 160 ? 160 : lds_max / 1024;
    if (sw.hash_generic) {  // tests: the multiply form of the duplicate hash (what B = 8 uses; the lane plan has none)
        ctx->luts.dup_planes.clear();
        ctx->luts.dup_nq = 0;
    }
    const bool lane_wanted = sw.lane != 0 && lane_plan_supported(ctx->dp, ctx->luts, lds_max);
    ctx->split = (ctx->dp.stats_one_pass || ((ctx->dp.front_lane || ctx->dp.corr_lane || ctx->dp.merge_lane) && lane_wanted)) && sw.split != 0;
    ctx->lane = ctx->split && lane_wanted;
    ctx->cfg.split = ctx->split ? 1 : 0;
    ctx->cfg.threads = sw.threads ? sw.threads : (ctx->split ? 256 : 1024);
    ctx->cfg.P = sw.tile;
    // (FASTP_GPU_LDS_KB above what the device has is clamped to it: a budget the card cannot give would only fail the launch)
    ctx->cfg.lds_budget = std::min(sw.lds_kb ? sw.lds_kb : (ctx->split ? std::min(40, lds_kb_default) : lds_kb_default), lds_max / 1024) * 1024;
    if (ctx->cfg.threads < 64 || ctx->cfg.threads > 1024 || (ctx->cfg.threads & 63))
        return fail(ctx, FASTP_GPU_E_INVALID, "FASTP_GPU_THREADS must be a multiple of 64 in 64..1024");
    std::string err;
    int rc = compute_lds_layout(ctx->dp, ctx->cfg, ctx->L, err, ctx->luts.dup_nq);
    if (rc && ctx->split && !sw.lds_kb) {  // long reads (or a tile size asked for): the small budget holds no such tile
        ctx->cfg.lds_budget = lds_kb_default * 1024;
        rc = compute_lds_layout(ctx->dp, ctx->cfg, ctx->L, err, ctx->luts.dup_nq);
    }
    if (rc) return fail(ctx, rc, err);
    int blocks_per_cu = std::max(1, (int)(lds_max / (ctx->L.total * 4)));
    blocks_per_cu = std::max(1, std::min(blocks_per_cu, 2048 / ctx->cfg.threads));   // 32 wavefronts per CU
#ifndef FQ_HOSTSIM
    {
        // persistent workgroups: the grid must not exceed what is resident at once (registers bound it, not only LDS)
        int nb = 0;
        const void* kfn = tile_kernel_for(ctx);
        (void)hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->L.total * 4);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kfn, ctx->cfg.threads, (size_t)ctx->L.total * 4) == hipSuccess && nb > 0)
            blocks_per_cu = std::min(blocks_per_cu, nb);
        (void)hipGetLastError();
    }
#endif
    ctx->blocks = ctx->cus * blocks_per_cu;
    // a workgroup's packed per-cycle counters hold CYC_MAX_READS reads per Stats slot
    ctx->tiles_per_block = CYC_MAX_READS / ctx->L.P;
    if (sw.max_tiles_per_block > 0 && sw.max_tiles_per_block < ctx->tiles_per_block) ctx->tiles_per_block = sw.max_tiles_per_block;  // tests: force several launches
    if (ctx->tiles_per_block < 1) return fail(ctx, FASTP_GPU_E_INVALID, "tile too large for the packed counters");
    return 0;
}

// the Stats kernel of a split plan: form 5 where its joint table fits the device's LDS and the options allow it (stats5_copies), else form 4
static int plan_stats_kernel(fastp_gpu_ctx* ctx) {
    if (!ctx->split) return 0;
    const int lds_max = ctx->lds_bytes;
    StatsArgs& sa = ctx->t_stats;
    sa.H = ctx->dp.qw_g / 2;
    int hb = 0;
    const int kc5 = stats5_copies(ctx->dp, lds_max, &hb);
    if (kc5) {
        ctx->st_form = 5;
        sa.H16 = (ctx->dp.qw_g + 3) / 4;
        sa.kc = kc5;
        sa.Hs = hb;                     // the table's columns: all of a read's (H16), or a block of them
        ctx->st_lds_dwords = stats5_lds_layout(sa, ctx->L.Cp, hb, kc5);
        ctx->st5_inst = stats5_inst_for(sa.Hs, sa.kc, sa.H16, stats5_no_front(ctx->dp));
        ctx->st5_fn = stats5_kernel_for(ctx->st5_inst);
        ctx->st_max_reads = CYC_MAX_READS;   // (a list entry holds the trip in 10 bits: 16 wavefronts x (64 / hb >= 4) units per trip, <= 256 trips)
    } else {
        ctx->st_form = 4;
        ctx->st_lds_dwords = stats4_lds_layout(sa, lds_max);
        ctx->st_max_reads = ST4_MAX_READS;
    }
    ctx->st_slab_dwords = 4 * ctx->L.Cp * N_CLS * 2 + 4 * KMER_BINS + 4 * 128;
    ctx->st_threads = 1024;
    if (ctx->st_lds_dwords * 4 > lds_max) return fail(ctx, FASTP_GPU_E_INVALID, "reads too long for the Stats kernel's LDS");
    const int st_per_cu = ctx->sw.stats_blocks_per_cu ? ctx->sw.stats_blocks_per_cu : std::min(2048 / ctx->st_threads, lds_max / (ctx->st_lds_dwords * 4));
    ctx->st_blocks = ctx->cus * std::max(1, st_per_cu);
    return 0;
}

// the lane kernel of a lane plan: its LDS layout, as many wavefronts per workgroup as that leaves room for, its grid
static int plan_lane_kernel(fastp_gpu_ctx* ctx) {
    if (!ctx->lane) return 0;
    // --cut_front on the lane plan (a front per read) has its POST Stats only in form 5 of the Stats kernel
    if (ctx->dp.front_per_read && ctx->st_form != 5)
        return fail(ctx, FASTP_GPU_E_INVALID, "a front per read on the lane plan needs form 5 of the Stats kernel, which was not chosen");
    ctx->ln_swm = ctx->dp.sw_g <= 10 ? 10 : 16;
    LaneLds& l = ctx->ln_lds;
    int o = 0;
    l.n_misc = MISC_ISIZE + ctx->dp.isize_max + 1;
    l.jkmer = 0;
    if (ctx->dp.merge_lane) {   // the merged reads' junction 5-mers: counters behind the MISC_* ones (ReduceArgs::merge_tail)
        l.jkmer = o + l.n_misc;
        l.n_misc += KMER_BINS;
    }
    l.misc = o; o += l.n_misc;
    const int lw = (ctx->dp.cycles + 2) / 2;
    l.lut_ov = o; o += lw;
    l.lut_lowq = o; o += lw;
    l.lut_cplx = o; o += lw;
    l.val4 = o; o += 256;
    o = (o + 1) & ~1;
    l.planes = o;
    l.n_planes = ctx->dp.dup_enabled ? (int)ctx->luts.dup_planes.size() : 0;
    o += l.n_planes;
    o = (o + 3) & ~3;
    l.stage = o;
    l.stage_dwords = (64 * std::max(ctx->dp.qw_g, ctx->dp.sw_g) + 4 * ctx->ln_swm + 3) & ~3;   // + the over-read of the last row
    l.part_dwords = ctx->dp.paired ? (ctx->ln_swm / 2) * 64 : 0;   // read 1 of a pair: [ln_swm / 2 words][64 lanes]
    // as many wavefronts per workgroup as the LDS holds (up to three per SIMD for reads <= 160 bases, two above)
    const int max_waves = (ctx->ln_swm > 10 ? 512 : 256 * FQ_LANE_WAVES) / 64;
    l.clist_dwords = (ctx->dp.corr_lane && ctx->dp.paired) ? (ctx->ln_swm / 2) * 64 : 0;   // -c: read 1's edited positions, a bit mask per lane
    // the workgroup's chunk counter (l.ctr below) and the reserve come out of the LDS before it is divided into
    // wavefronts (o and every per-wavefront size are multiples of 4 dwords: no padding in front of l.ctr)
    const int tail_dwords = LANE_CTR_DWORDS + LANE_RESERVED_DWORDS;
    int waves = (int)(((long long)ctx->lds_bytes / 4 - o - tail_dwords) / (l.stage_dwords + l.part_dwords + l.clist_dwords));
    waves = std::max(1, std::min(waves, max_waves));
    ctx->ln_threads = waves * 64;
    o += waves * l.stage_dwords;
    l.part = o;
    o += waves * l.part_dwords;
    l.clist = o;
    o += waves * l.clist_dwords;
    o = (o + 3) & ~3;
    l.ctr = o;
    o += tail_dwords;
    l.total = o;
    int per_cu = 0;
#ifndef FQ_HOSTSIM
    {
        int nb = 0;
        lane_kernel_fn fn = lane_kernel_for(ctx->ln_swm, ctx->dp.dup_enabled ? ctx->dp.dup_bufnum : 0, ctx->dp.paired != 0, lane_ext(ctx->dp));
        (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, l.total * 4);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, ctx->ln_threads, (size_t)l.total * 4) == hipSuccess && nb > 0) per_cu = nb;
        (void)hipGetLastError();
    }
#endif
    if (per_cu <= 0) per_cu = 4;
    ctx->ln_blocks = ctx->cus * per_cu;
    return 0;
}

// Every kernel with dynamic LDS the context may launch: what its layout needs and what its attribute is set to.  The rows with a
// check stay in this order: check_kernel_lds names the first that does not fit.
static std::vector<KernelLds> kernel_lds_table(const fastp_gpu_ctx* ctx) {
    const DevParams& dp = ctx->dp;
    const char* tile_name = nullptr;
    const void* tile = tile_kernel_for(ctx, &tile_name);
    const int tile_bytes = ctx->L.total * 4, st_bytes = ctx->st_lds_dwords * 4, ln_bytes = ctx->ln_lds.total * 4;
    std::vector<KernelLds> t = {
        {tile_name, tile, tile_bytes, tile_bytes},
        {"hash kernel", (const void*)fq_hash_kernel, tile_bytes, tile_bytes},
        {"text kernel", (const void*)fq_text_kernel, (long long)TEXT_WAVES * text_wave_bytes((dp.max_len + 8 + 7) & ~7), aux_lds_cap(ctx)},
        {"deflate kernel", (const void*)fq_deflate_kernel, (long long)sizeof(DefLds), (int)sizeof(DefLds)},
        {"deflate kernel (levels 5 to 9)", (const void*)fq_deflate_chain_kernel, (long long)sizeof(DefChainLds), (int)sizeof(DefChainLds)},
        {"inflate kernel", (const void*)fq_inflate_kernel, inflate_lane_lds_bytes(), inflate_lane_lds_bytes()}};
    if (ctx->split) {   // (form 4's kernel has its attribute in a form 5 context as well)
        if (ctx->st_form == 5) t.push_back({"Stats kernel (form 5)", (const void*)ctx->st5_fn, st_bytes, st_bytes});
        t.push_back({"Stats kernel", (const void*)fq_stats_kernel, ctx->st_form == 5 ? LDS_NO_CHECK : st_bytes, st_bytes});
#ifdef FQ_PROFILE_ABLATION
        if (ctx->st_form == 5) t.push_back({"Stats kernel (ablation)", (const void*)stats5_kernel_for(ST5_ABLATION), LDS_NO_CHECK, st_bytes});
#endif
    }
    if (ctx->lane) {   // the instantiation that hashes nothing, and the one that hashes for Duplicate
        t.push_back({"lane kernel", (const void*)lane_kernel_for(ctx->ln_swm, 0, dp.paired != 0, lane_ext(dp)), ln_bytes, ln_bytes});
        if (dp.dup_enabled)
            t.push_back({"lane kernel", (const void*)lane_kernel_for(ctx->ln_swm, dp.dup_bufnum, dp.paired != 0, lane_ext(dp)), LDS_NO_CHECK, ln_bytes});
    }
    if (ctx->split && dp.front_per_read)
        t.push_back({"front Stats kernel", (const void*)fq_front_stats_kernel, (long long)front_stats_lds_bytes(ctx), (int)front_stats_lds_bytes(ctx)});
    if (ctx->split && dp.corr_lane)
        t.push_back({"correction Stats kernel", (const void*)fq_corr_stats_kernel, (long long)corr_stats_lds_bytes(ctx), (int)corr_stats_lds_bytes(ctx)});
    // attribute only: the count kernel sizes its tables to aux_lds_cap at each launch like the text kernel; a card with less LDS
    // than the wave inflate kernel takes inflates with the lane kernel only
    t.push_back({"overrepresentation count kernel", (const void*)fq_ovr_count_kernel, LDS_NO_CHECK, aux_lds_cap(ctx)});
    if ((int)sizeof(IwLds) <= ctx->lds_bytes) t.push_back({"inflate wave kernel", (const void*)fq_inflate_wave_kernel, LDS_NO_CHECK, (int)sizeof(IwLds)});
    return t;
}

// every kernel's dynamic LDS against what the device gives a workgroup: a layout that does not fit fails here, never at a launch
static int check_kernel_lds(fastp_gpu_ctx* ctx) {
    ctx->kernel_lds = kernel_lds_table(ctx);
    for (const KernelLds& k : ctx->kernel_lds)
        if (k.need > ctx->lds_bytes)
            return fail(ctx, FASTP_GPU_E_INVALID, std::string(k.name) + ": " + std::to_string(k.need) + " bytes of LDS per workgroup, the device has " +
                                                      std::to_string(ctx->lds_bytes));
    return 0;
}

// the most units one launch takes, and the Stats slabs such a launch needs
static int plan_launch_size(fastp_gpu_ctx* ctx) {
    const int cap_tiles = ctx->sw.max_tiles_per_block;
    long long mp = (long long)ctx->blocks * ctx->tiles_per_block * ctx->L.P;
    if (ctx->split) {   // the per-read kernel has no packed counters; a Stats workgroup takes <= CYC_MAX_READS units
        mp = (long long)ctx->st_blocks * CYC_MAX_READS;   // (form 4 takes such a launch as several rounds of workgroups)
        if (ctx->st_form == 5) mp *= 2;                   // (one workgroup per CU: two rounds, as many units per launch as before)
        if (cap_tiles > 0) mp = std::min(mp, (long long)ctx->blocks * cap_tiles * ctx->L.P);
    }
    if (mp > (1ll << DUP_IDX_BITS) - 1) mp = (1ll << DUP_IDX_BITS) - 1;
    if (ctx->split && ctx->dp.corr_lane) {   // the launch's correction list (fill_launch_buffers): an entry for every base of every pair
        // 2^29 entries (6 GiB with the chains) - or, on a card with 64 GiB to spare, just under 2^30: a -c / --merge step of 4 Mi
        // pairs of 2x150 is then ONE launch instead of two (2 * index + 1 still fits an int)
        long long entries = 1ll << 29;
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree >= ((size_t)64 << 30)) entries = (1ll << 30) - 64;
        (void)hipGetLastError();
        mp = std::min(mp, entries / std::max(1, ctx->dp.max_len));
    }
    mp = mp / ctx->L.P * ctx->L.P;
    ctx->max_pairs_per_launch = (int)mp;
    // a slab per workgroup of the largest launch: rounds of st_blocks for form 4, two rounds for form 5
    if (ctx->split)
        ctx->st_max_grid = ctx->st_form == 4 ? (ctx->max_pairs_per_launch + ST4_MAX_READS - 1) / ST4_MAX_READS + ctx->st_blocks : 2 * ctx->st_blocks + 2;
    ctx->slab_dwords = ctx->L.acc_end - ctx->L.acc_cyc;
    return 0;
}

// FASTP_GPU_VERBOSE=1: the geometry lines on stderr
static int print_geometry(fastp_gpu_ctx* ctx) {
    if (!ctx->sw.verbose) return 0;
    if (ctx->exact_all) fprintf(stderr, "fastp_gpu: FASTP_GPU_EXACT=1, every unit takes the text kernel\n");
    fprintf(stderr, "fastp_gpu: %s, tile P=%d (%d rows), %d threads, LDS %d bytes, %d workgroups, %d units/launch; stats kernel form %d, %d x %d threads, LDS %d bytes\n",
            ctx->lane ? "lane plan" : (ctx->split ? "split plan" : "fused plan"), ctx->L.P, ctx->L.NR, ctx->cfg.threads, ctx->L.total * 4, ctx->blocks,
            ctx->max_pairs_per_launch, ctx->st_form, ctx->st_blocks, ctx->st_threads, ctx->st_lds_dwords * 4);
    if (ctx->lane)
        fprintf(stderr, "fastp_gpu: lane kernel %d x %d threads (%d per CU), LDS %d bytes per workgroup (stage %d + read-1 sums %d per wavefront), SWM %d, ext %d\n",
                ctx->ln_blocks, ctx->ln_threads, ctx->ln_blocks / std::max(1, ctx->cus), ctx->ln_lds.total * 4, ctx->ln_lds.stage_dwords * 4,
                ctx->ln_lds.part_dwords * 4, ctx->ln_swm, (int)lane_ext(ctx->dp));
    return 0;
}

#ifndef FQ_HOSTSIM
// a second stream that really runs beside the first (fq_probe_wait_kernel): up to six candidates, the ones that share the
// first stream's queue are held until the search ends (the next one is then given another queue) and closed afterwards
static int probe_tail_stream(fastp_gpu_ctx* ctx) {
    int* d_flag = nullptr;
    std::vector<hipStream_t> held;   // the candidates so far: all but the chosen one are closed on the way out
    const int tries = 6;
    auto search = [&]() -> int {
        HIP_TRY(ctx, hipMalloc((void**)&d_flag, 2 * sizeof(int)));
        for (int t = 0, beside = 0; t < tries && !beside; t++) {
            hipStream_t cand = nullptr;
            HIP_TRY(ctx, hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
            held.push_back(cand);
            HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 2 * sizeof(int), ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            hipLaunchKernelGGL(fq_probe_wait_kernel, dim3(1), dim3(64), 0, ctx->stream, d_flag, 2000000ll);
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(fq_probe_set_kernel, dim3(1), dim3(64), 0, cand, d_flag);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(cand));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            int h[2] = {0, 0};
            HIP_TRY(ctx, hipMemcpy(h, d_flag, sizeof(h), hipMemcpyDeviceToHost));
            beside = h[1];
        }
        ctx->tail = held.back();   // (if none runs beside the first, the last one: correct, one behind the other)
        held.pop_back();
        if (ctx->sw.verbose) fprintf(stderr, "fastp_gpu: second stream: candidate %d of %d runs beside the first\n", (int)held.size() + 1, tries);
        return 0;
    };
    const int rc = search();
    if (rc) (void)hipDeviceSynchronize();   // a probe kernel may still be running: it reads and writes d_flag
    for (hipStream_t s : held) (void)hipStreamDestroy(s);
    if (d_flag) (void)hipFree(d_flag);
    return rc;
}
#endif

// the launch stream and, in the split plans, the tail stream with the two events that order them
static int create_streams(fastp_gpu_ctx* ctx) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    fq::timeline("create: launch stream created");
    if (!ctx->split) return 0;
#ifdef FQ_HOSTSIM
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->tail, hipStreamNonBlocking));
#else
    const int rc = probe_tail_stream(ctx);
    if (rc) return rc;
#endif
    fq::timeline("create: second stream probed");
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_k1, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_tail, hipEventDisableTiming));
    return 0;
}

static int set_kernel_attributes(fastp_gpu_ctx* ctx) {
    for (const KernelLds& k : ctx->kernel_lds) {
        const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.set);
        if (e != hipSuccess)
            return fail(ctx, FASTP_GPU_E_HIP, std::string("hipFuncSetAttribute(") + k.name + ", MaxDynamicSharedMemorySize, " + std::to_string(k.set) + "): " + hipGetErrorString(e));
    }
    fq::timeline("create: kernel attributes set");
    return 0;
}

static int upload(fastp_gpu_ctx* ctx, void** dptr, const void* src, size_t bytes) {
    if (bytes == 0) { *dptr = nullptr; return 0; }
    HIP_TRY(ctx, hipMalloc(dptr, bytes));
    HIP_TRY(ctx, hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

// the buffers whose size create knows (slabs, bloom filter) and the tables the kernels read
static int upload_tables(fastp_gpu_ctx* ctx) {
    const HostLuts& luts = ctx->luts;
    if (ctx->split) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_st_slabs, (size_t)ctx->st_max_grid * ctx->st_slab_dwords * 4));
    if (ctx->lane) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_ln_slabs, (size_t)ctx->ln_blocks * ctx->ln_lds.n_misc * 4));
    struct { void** dptr; const void* src; size_t bytes; } tables[] = {
        {(void**)&ctx->d_ov_limit, luts.ov_limit.data(), luts.ov_limit.size() * 2},
        {(void**)&ctx->d_lowq, luts.lowq_limit.data(), luts.lowq_limit.size() * 2},
        {(void**)&ctx->d_cplx, luts.cplx_min.data(), luts.cplx_min.size() * 2},
        {(void**)&ctx->d_primes, luts.dup_primes.data(), luts.dup_primes.size() * 4},
        {(void**)&ctx->d_planes, luts.dup_planes.data(), luts.dup_planes.size() * 4},
        {(void**)&ctx->d_posum, luts.dup_posum.data(), luts.dup_posum.size() * 8},
        {(void**)&ctx->d_fasta_words, luts.fasta_words.data(), luts.fasta_words.size() * 4},
        {(void**)&ctx->d_fasta_len, luts.fasta_len.data(), luts.fasta_len.size() * 4}};
    int rc = 0;
    for (const auto& t : tables)
        if ((rc = upload(ctx, t.dptr, t.src, t.bytes))) return rc;
    if (ctx->dp.overrep) {
        for (int m = 0; m < 2; m++) {
            if ((rc = upload(ctx, (void**)&ctx->d_ovr_table[m], luts.ovr_table[m].data(), luts.ovr_table[m].size() * 4))) return rc;
            if ((rc = upload(ctx, (void**)&ctx->d_ovr_sym[m], luts.ovr_sym[m].data(), luts.ovr_sym[m].size()))) return rc;
            if ((rc = upload(ctx, (void**)&ctx->d_ovr_len[m], luts.ovr_len[m].data(), luts.ovr_len[m].size() * 4))) return rc;
        }
        const uint64_t zero = 0;
        if ((rc = upload(ctx, (void**)&ctx->d_post_seen, &zero, sizeof(zero)))) return rc;
    }
    std::vector<int64_t> zero((size_t)ctx->cl.total, 0);
    zero[0] = FASTP_GPU_ABI_VERSION;
    zero[1] = ctx->cl.cycles;
    zero[2] = ctx->dp.isize_max;
    if ((rc = upload(ctx, (void**)&ctx->d_ctr, zero.data(), zero.size() * 8))) return rc;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_slabs, (size_t)ctx->blocks * ctx->slab_dwords * 4));
    if (ctx->dp.dup_enabled) {
        const size_t bytes = (size_t)(ctx->dp.dup_bits >> 3) * ctx->dp.dup_bufnum;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_bitmap, bytes));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_bitmap, 0, bytes, ctx->stream));
    }
    if (ctx->sw.phase_timing) {
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_phase, 16 * sizeof(u64)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_phase, 0, 16 * sizeof(u64), ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// form 5 contexts: what stays free beside the Stats kernel's waves, and for whom
static int choose_finish_threads(fastp_gpu_ctx* ctx) {
#ifndef FQ_HOSTSIM
    if (!(ctx->split && ctx->st_form == 5)) return 0;
    int32_t kr[KERNEL_REGS_N];
    const int rc = fastp_gpu_debug_kernel_regs(ctx, kr, KERNEL_REGS_N);
    if (rc) return rc;
    const int waves = ctx->st_threads / 64 / 4, alloc = (kr[1] + 7) & ~7, left = 512 - waves * alloc;
    // Duplicate's finish is a grid-stride loop over the units: any workgroup size does.  As 1024 lanes (four waves per SIMD) it
    // never fitted what the Stats kernel leaves, waited for that kernel's workgroups to go and ended the step behind it; the
    // largest size that fits runs beside it like losers and winners do.  Nothing fits beside a 128-VGPR instantiation: 1024 stays.
    // Paired contexts only: a single-end unit has half the bases, the Stats kernel ends BEFORE Duplicate's chain does (10 M reads:
    // 540 us against 40 + 230 + 320), and alone on the chip finish is slower in small workgroups - 234 us against 67, four times
    // the workgroups and as many adds to one counter (profiles/r08_a_step_tail.txt: the single-end step was 8 - 10 % slower).
    const int finish_a8 = (kr[13] + 7) & ~7;
    for (int t = 1024; t >= 256 && ctx->dp.paired; t >>= 1)
        if (kr[13] > 0 && t <= kr[14] && (t / 256) * finish_a8 <= left) { ctx->finish_threads = t; break; }
    if (ctx->sw.verbose) {
        const char* names[4] = {"fq_reduce_kernel", "fq_dup_losers_kernel", "fq_dup_winners_kernel", "fq_dup_finish_kernel"};
        std::string fits;
        for (int k = 0; k < 4; k++) {   // a workgroup of the kernel as launched (256 lanes = a wave per SIMD, 1024 = four) in what is left
            const int a8 = (kr[4 + 3 * k] + 7) & ~7, wg_waves = std::max(1, (k == 3 ? ctx->finish_threads : kr[5 + 3 * k]) / 64 / 4);
            if (a8 * wg_waves <= left)
                fits += std::string(fits.empty() ? "" : ", ") + names[k] + " (" + std::to_string(wg_waves) + " x " + std::to_string(a8) + ")";
        }
        fprintf(stderr, "fastp_gpu: stats kernel instantiation %d: %d VGPRs (allocated %d), %d waves per SIMD, %d registers per SIMD left; a workgroup fits beside it of: %s; fq_dup_finish_kernel runs as %d lanes\n",
                ctx->st5_inst, kr[1], alloc, waves, left, fits.empty() ? "none" : fits.c_str(), ctx->finish_threads);
    }
#endif
    return 0;
}

extern "C" int fastp_gpu_create(const fastp_gpu_params* params, int device, fastp_gpu_ctx** out) {
    if (!params || !out) return fail(nullptr, FASTP_GPU_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    fq::timeline("create: begin");
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, FASTP_GPU_E_NO_DEVICE, "no HIP device visible - the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, FASTP_GPU_E_NO_DEVICE, "device ordinal out of range");
    // the one owner until the last line: a failing step returns its code, the message is fastp_gpu_last_error(nullptr)'s
    std::unique_ptr<fastp_gpu_ctx, void (*)(fastp_gpu_ctx*)> owner(new fastp_gpu_ctx(), fastp_gpu_destroy);
    fastp_gpu_ctx* ctx = owner.get();
    ctx->sw = read_switches();
    ctx->params = *params;
    ctx->device = device;
    ctx->exact_all = ctx->sw.exact != 0;   // tests: every unit through the text kernel (fq_text.h)
    int rc;
    if ((rc = own_param_strings(ctx)) || (rc = read_params_and_device(ctx)) || (rc = choose_plan(ctx)) || (rc = plan_stats_kernel(ctx)) ||
        (rc = plan_lane_kernel(ctx)) || (rc = check_kernel_lds(ctx)) || (rc = plan_launch_size(ctx)))
        return rc;
    fastp_gpu_counter_layout_for_params(&ctx->params, &ctx->cl);
    if ((rc = print_geometry(ctx))) return rc;
    fq::timeline("create: plan chosen (device properties, occupancy queries)");
    if ((rc = create_streams(ctx)) || (rc = set_kernel_attributes(ctx)) || (rc = upload_tables(ctx))) return rc;
    fill_arg_templates(ctx);
    if ((rc = choose_finish_threads(ctx))) return rc;
    fq::timeline("create: end (tables uploaded, bloom filter cleared)");
    *out = owner.release();
    return FASTP_GPU_OK;
}

// debugging aid (not part of the drop-in surface): cycles spent per phase of the fused kernel,
// summed over workgroups, when the context was created with FASTP_GPU_PHASE_TIMING=1
extern "C" int fastp_gpu_debug_phase_cycles(fastp_gpu_ctx* ctx, uint64_t* out16) {
    if (!ctx || !out16 || !ctx->d_phase) return FASTP_GPU_E_INVALID;
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out16, ctx->d_phase, 16 * sizeof(u64), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemset(ctx->d_phase, 0, 16 * sizeof(u64)));
    return FASTP_GPU_OK;
}

// debugging aid: the LDS plan of the context's most recent overrepresentation launch as launch_overrep chose it - out[0] how many
// such launches the context has made (0: the rest is {0, -1, -1}), out[1] sym_cap (0: the reads are not staged), out[2] / out[3]
// table_lds[0] / table_lds[1] (the dword offset of the mate's seed table in LDS; -1: the table is probed in global memory).
// Which branch of ovr_count_body ran follows from these; the emulator reports what it chose the same way.
extern "C" int fastp_gpu_debug_overrep_plan(fastp_gpu_ctx* ctx, int32_t* out, int32_t n) {
    if (!ctx || !out || n < 4) return FASTP_GPU_E_INVALID;
    out[0] = ctx->ovr_launches;
    for (int k = 0; k < 3; k++) out[1 + k] = ctx->ovr_plan[k];
    return FASTP_GPU_OK;
}

static int ensure(fastp_gpu_ctx* ctx, void** buf, size_t* cap, size_t need) {
    if (*cap >= need) return 0;
    if (*buf) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(*buf)); *buf = nullptr; *cap = 0; }
    size_t want = need + need / 4;
    HIP_TRY(ctx, hipMalloc(buf, want));
    *cap = want;
    return 0;
}

// A scratch buffer's layout, stated once: the pieces in order, each `bytes` rounded up to `align` long.  A site runs its takes
// on a null base first - nothing is handed out, `off` ends as the size to `ensure` - and again on the buffer for the pointers.
struct Carve {
    u8* base;
    size_t off = 0;
    explicit Carve(void* b) : base((u8*)b) {}
    template <class T = u8> T* take(size_t bytes, size_t align = 1) {
        const size_t at = off;
        off += (bytes + align - 1) / align * align;
        return base ? (T*)(base + at) : nullptr;
    }
};

static int get_events(fastp_gpu_ctx* ctx, hipEvent_t* a, hipEvent_t* b) {
    if (ctx->pending_events.size() >= 64) drain_events(ctx);
    if (!ctx->free_events.empty()) {
        *a = ctx->free_events.back().first;
        *b = ctx->free_events.back().second;
        ctx->free_events.pop_back();
        return 0;
    }
    HIP_TRY(ctx, hipEventCreate(a));
    HIP_TRY(ctx, hipEventCreate(b));
    return 0;
}

// one launch: at most ctx->max_pairs_per_launch units
// Stats::statRead's overrepresentation analysis (stats.cpp:270-288) of one launch, after its records exist
static int launch_overrep(fastp_gpu_ctx* ctx, const KernelArgs& a, int n, hipStream_t st, const fastp_gpu_batch* b = nullptr) {
    const fastp_gpu_counter_layout& cl = ctx->cl;
    int rc;
    if (ctx->dp.overrep) {
        OvrArgs o;
        memset(&o, 0, sizeof(o));
        o.n = n;
        o.paired = ctx->dp.paired;
        o.dedup = ctx->dp.dedup;
        o.sampling = ctx->dp.overrep_sampling;
        o.pre_mod = (u32)(ctx->units_seen % (uint64_t)o.sampling);
        o.sw_g = ctx->dp.sw_g;
        o.qw_g = ctx->dp.qw_g;
        o.merge = ctx->dp.merge;
        o.merge_include_unmerged = ctx->dp.merge_include_unmerged;
        o.pair = a.pair;
        for (int m = 0; m < 2; m++) { o.seq[m] = a.seq[m]; o.qual[m] = a.qual[m]; o.len[m] = a.len[m]; o.res[m] = a.res[m]; }
        if (b && b->n_exotic > 0) {   // units with letters outside ACGTN: the counting kernel reads their symbols from the text
            o.first = a.first;
            o.x_unit = ctx->d_x_unit;
            o.x_n = b->n_exotic;
            o.x_dense = b->exotic_dense;
            for (int m = 0; m < 2; m++) { o.x_text[m] = b->exotic_text[m]; o.x_off[m] = b->exotic_off[m]; }
        }
        const int nb = (n + 255) / 256;
        const int task_cap = 4 * (n / o.sampling + 2);
        rc = ensure(ctx, (void**)&ctx->d_ovr_work, &ctx->ovr_work_cap, ((size_t)2 * nb + 1 + task_cap) * 4);
        if (rc) return rc;
        o.blocksum = ctx->d_ovr_work;
        o.blockbase = ctx->d_ovr_work + nb;
        o.n_tasks = ctx->d_ovr_work + 2 * nb;
        o.tasks = ctx->d_ovr_work + 2 * nb + 1;
        o.task_cap = task_cap;
        o.post_seen = ctx->d_post_seen;
        for (int m = 0; m < 2; m++) {
            OvrMate& M = o.mate[m];
            M.n_seeds = m == 0 ? ctx->params.n_overrep_seqs1 : (ctx->dp.paired ? ctx->params.n_overrep_seqs2 : 0);
            M.eval_len = m == 0 ? ctx->params.eval_seq_len1 : ctx->params.eval_seq_len2;
            for (int k = 0; k < OVR_STEPS; k++) { M.steps[k] = ctx->luts.ovr_steps[m][k]; M.pw[k] = ctx->luts.ovr_pw[m][k]; }
            M.table = ctx->d_ovr_table[m];
            M.table_mask = (u32)(ctx->luts.ovr_table[m].size() / 2 - 1);
            M.seed_sym = ctx->d_ovr_sym[m];
            M.seed_len = ctx->d_ovr_len[m];
        }
        o.ctr = ctx->d_ctr;
        for (int k = 0; k < 4; k++) { o.o_count[k] = cl.overrep_count[k]; o.o_dist[k] = cl.overrep_dist[k]; }
        // the post-filtering Stats analyse the corrected reads: from the engine's own list of this launch where it keeps one (-c with
        // the Stats kernel as its own launch: sized for an edit at every base, it cannot overflow), else from the caller's
        // (a launch with units for the text kernel: that kernel's edits are in the caller's list only - it counts its units' POST
        // Stats itself, fq_corr_stats_kernel must not see them - so such a launch reads the caller's list as before)
        const bool own_list = a.corr_int != nullptr && a.corr_int_cap > 0 && !(b && b->n_exotic > 0) && !ctx->exact_all;
        if (ctx->dp.correction && !own_list && !(a.corrections && a.corr_capacity > 0))
            return fail(ctx, FASTP_GPU_E_INVALID, "overrepresentation analysis with correction needs the correction list in the results");
        if (own_list || (a.corrections && a.corr_capacity > 0)) {
            const size_t reads = (size_t)(ctx->dp.paired ? 2 : 1) * n;
            const int list_cap = own_list ? a.corr_int_cap : a.corr_capacity;
            rc = ensure(ctx, (void**)&ctx->d_ovr_corr, &ctx->ovr_corr_cap, (reads + (size_t)list_cap) * 4);
            if (rc) return rc;
            o.corr = own_list ? a.corr_int : a.corrections;
            o.n_corr = own_list ? a.n_corr_int : a.n_corrections;
            o.corr_cap = list_cap;
            o.first = a.first;
            o.corr_head = ctx->d_ovr_corr;
            o.corr_next = ctx->d_ovr_corr + reads;
            HIP_TRY(ctx, hipMemsetAsync(o.corr_head, 0, reads * 4, st));
            if (own_list)   // (capacity far above the fill: a grid-stride walk over what the list holds)
                hipLaunchKernelGGL(fq_corr_link_kernel, dim3(std::min(4096, (list_cap + 255) / 256)), dim3(256), 0, st, o);
            else
                hipLaunchKernelGGL(fq_ovr_corr_link_kernel, dim3((list_cap + 255) / 256), dim3(256), 0, st, o);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemsetAsync(o.n_tasks, 0, 4, st));
        hipLaunchKernelGGL(fq_ovr_pass_kernel, dim3(nb), dim3(256), 16, st, o);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(fq_ovr_scan_kernel, dim3(1), dim3(1024), 1024 * 4, st, o, nb);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(fq_ovr_tasks_kernel, dim3(nb), dim3(256), 64, st, o);
        HIP_TRY(ctx, hipGetLastError());
        {   // LDS plan of the counting kernel: symbols of one task per lane, then the seed tables that still fit
            const int longest = ctx->dp.max_len * (ctx->dp.merge ? 2 : 1);
            int lds_bytes = (((longest + 4) * OVR_SYM_STRIDE + 15) / 16) * 16;   // (+ 4 rows: a trip's four slides read unguarded)
            o.sym_cap = longest;
            if (lds_bytes > std::min(120 * 1024, aux_lds_cap(ctx))) { o.sym_cap = 0; lds_bytes = 0; }   // reads too long to stage: the global path
            for (int m = 0; m < 2; m++) {
                const size_t tb = ctx->luts.ovr_table[m].size() * 4;
                o.table_lds[m] = -1;
                if (o.mate[m].n_seeds > 0 && tb > 0 && lds_bytes + (int)tb <= aux_lds_cap(ctx)) {
                    o.table_lds[m] = lds_bytes / 4;
                    lds_bytes += (int)tb;
                }
            }
            ctx->ovr_launches++;
            ctx->ovr_plan[0] = o.sym_cap; ctx->ovr_plan[1] = o.table_lds[0]; ctx->ovr_plan[2] = o.table_lds[1];
            hipLaunchKernelGGL(fq_ovr_count_kernel, dim3((task_cap + OVR_TPB - 1) / OVR_TPB), dim3(OVR_BLOCK), (size_t)lds_bytes, st, o);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->units_seen += (uint64_t)n;
    return FASTP_GPU_OK;
}

// what a launch does with Duplicate::checkPair/checkRead
enum ChunkMode {
    CHUNK_STREAM,    // one stream: decide inside this launch (the normal path)
    CHUNK_PASS1,     // sharded run, pass 1: insert + scan state, no decision (--dedup: nothing else; otherwise
                     // the worker loop runs here, its records just lack the RF_DUP flag)
    CHUNK_PASS2,     // sharded run, pass 2: decide from the scan state and the prefix bitmaps (--dedup: then the
                     // worker loop; otherwise the decision is patched into pass 1's records)
    CHUNK_OVERREP,   // the deferred overrepresentation analysis only
};

// the four row arrays of a launch (read 1's twice for single reads) on 16-byte boundaries: what 16-byte row copies need
static bool rows_aligned16(bool paired, const void* seq1, const void* qual1, const void* seq2, const void* qual2) {
    const void* ptrs[4] = {seq1, qual1, paired ? seq2 : seq1, paired ? qual2 : qual1};
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15u) return false;
    return true;
}

enum PerReadKernel { K_LANE, K_SCAN_WIDE, K_SCAN, K_FUSED };
enum TextPlace { TEXT_NONE, TEXT_BESIDE_LANE, TEXT_BEHIND_ON_TAIL, TEXT_INLINE };
enum DupPlace { DUP_NOWHERE, DUP_BEFORE_STATS, DUP_ON_TAIL, DUP_AT_END };
enum MiscFold { MISC_WITH_STATS, MISC_FIRST_ON_TAIL, MISC_LAST_ON_TAIL, MISC_ON_LAUNCH_STREAM };
enum OvrPlace { OVR_EARLY_ON_TAIL, OVR_AT_END, OVR_DEFERRED };

// Every decision of one launch: what runs, in which form and on which of the two streams (the launch stream - the caller's or
// the context's own - and ctx->tail).  plan_launch decides once, from the context, the mode and the batch; launch_chunk is the
// schedule that reads it, and nothing is decided after it.
struct LaunchPlan {
    ChunkMode mode = CHUNK_STREAM;
    // Units with letters outside ACGTN (fastp_gpu_batch::exotic_*; FASTP_GPU_EXACT=1: every unit) take the text kernel
    // (fq_text.h).  The plan's kernels still run over the whole launch, on a copy of the length arrays in which those units
    // are EMPTY; the text kernel then runs once over the listed units: it takes back what an empty unit added to the
    // counters (the same loop on an empty unit, sign -1), adds the real unit, and overwrites the unit's records and hash
    // values.  Duplicate's kernels run once over the whole launch afterwards: input order holds across both kinds.
    bool exact = false;
    int xk0 = 0, xk1 = 0;      // the launch's entries of the batch's list
    bool xskip = false;        // the lane plan runs the text kernel BESIDE its kernels: the units not to write are listed (KernelArgs::xskip)
    // the lane kernel copies rows with 16-byte accesses: a batch whose arrays are not 16-byte aligned takes the tile kernel -
    // but --merge has this plan only in its lane form: there the launch's rows move to 16-byte aligned arrays of the engine
    PerReadKernel kernel = K_FUSED;
    bool align_rows = false;
    // the text kernel of the listed units in front of Duplicate's hash pre-pass as well: it leaves their hash values, nothing else
    bool text_prepass = false;
    // TEXT_BESIDE_LANE (round 5): on the tail stream from in front of the lane kernel on, BESIDE the lane kernel (which counts such a
    // unit as the empty unit it sees and writes nothing of it, KernelArgs::xskip) and the Stats kernel (to which it is an empty
    // read); Duplicate's kernels wait for both.  A launch with a handful of such units used to wait 2.6 - 3.1 ms for one lane's
    // walk between the two kernels.
    // TEXT_BEHIND_ON_TAIL: behind the plan's kernel (the records and hash values of its units are overwritten) - and, in the split
    // plans, BESIDE the Stats kernel (round 5): the Stats kernel needs nothing of it (the listed units are empty reads to it, the
    // text kernel adds their Stats itself), only Duplicate's kernels do, so both go to the tail stream.
    // TEXT_INLINE: behind the plan's kernel on the launch stream.
    TextPlace text = TEXT_NONE;
    // the engine's own correction list of this launch (fill_launch_buffers)
    bool corr_list = false;
    // Duplicate::checkPair/checkRead over this chunk, in input order.
    // dedup_prepass: --dedup: hash pass -> duplicate decision -> the per-read kernel reads the decision
    // dedup_folded: --dedup without the hash pre-pass (round 5, lane plan, plain stream mode): the lane kernel hashes and claims as
    // without --dedup, Duplicate's tail decides, fq_dedup_apply_kernel takes the duplicates out again before the Stats kernel counts
    // (not in merge mode: a pair that merges is written out whatever Duplicate says, peprocessor.cpp:523-535)
    bool dedup_prepass = false, dedup_folded = false;
    // the claim step inside the per-read kernel (dup_prepare in front of it, dup_tail behind it; otherwise dup_claim_chain):
    // plain stream mode, one or two bloom buffers (the lane kernel: four as well), the context's own stream order
    // ... and a launch with units for the text kernel when that kernel runs beside the lane kernel (TEXT_BESIDE_LANE): the lane kernel
    // claims nothing for such a unit (KernelArgs::xskip), the text kernel claims its units' bits itself (fq_text.h t_claim) and
    // Duplicate's tail - which orders the claims by unit index, whoever fired them first - runs behind both
    bool claim_fused = false;
    // dup_prepare's clears (128 MB of table for 4 Mi pairs: 21 + 6 us) are needed by the kernels of dup_tail only, not by the kernel
    // that claims: where dup_tail will run on the tail stream they go there, beside the per-read kernel instead of in front of it
    // (that stream is past the previous launch's tail by then; the launch stream joins it at the end of every launch)
    bool clears_on_tail = false;
    // where what is left of Duplicate behind the per-read kernel runs (dup_tail with the claim fused, else dup_claim_chain):
    // DUP_BEFORE_STATS: --dedup folded: the decisions are needed before the Stats kernel classifies a base as kept - on the launch stream,
    //   dedup_apply behind it
    // DUP_ON_TAIL: the claim ran inside the per-read kernel: what is left of Duplicate (losers / winners / finish) needs nothing of
    //   the Stats kernel and runs beside it on its own stream; the launch stream joins it before anything else touches the records.
    //   (Beside it as far as the Stats kernel's registers leave room - misc_fold below: losers' and winners' 256-lane workgroups fit
    //   next to the instantiations without a front trim; finish's 1024-lane workgroup, four waves per SIMD, never does and runs
    //   when the Stats kernel's workgroups leave, beside the Stats fold.)
    //   Or: behind the text kernel, on its stream (the claim is not fused into a launch that has such units inline or behind).
    // DUP_AT_END: on the launch stream behind the folds (the fused plan; the forms that do not use the tail stream)
    DupPlace dup_place = DUP_NOWHERE;
    // the tail stream carries Duplicate's kernels or the text kernel: it records ev_tail, the launch stream waits for it at the end
    bool join_tail = false;
    // the slab folds.  The Stats fold: behind the Stats kernel on the launch stream.  The per-read kernel's MISC_* fold needs that
    // kernel only:
    // MISC_WITH_STATS: the fused plan has one set of slabs, one fold
    // MISC_FIRST_ON_TAIL: FIRST on the tail stream, in front of Duplicate's kernels.  How much of that stream runs BESIDE the Stats
    //   kernel is a matter of registers: its 1024-lane workgroup is four waves per SIMD, and where the launched instantiation is
    //   allocated 128 VGPRs (form 5 with a front trim; all of form 5 while it was one kernel with every instantiation as a branch)
    //   that is the whole 512-entry file - a tail kernel gets through when one of the Stats kernel's two rounds of workgroups ends,
    //   ONE kernel per such moment (profiles/r06_s_step_timeline.txt, r06_t_step_timeline.txt: each "takes" 0.43 - 0.50 ms, 0.01 -
    //   0.03 alone), and the rest of the chain is the end of the step with nothing else on the chip.  The instantiations without a
    //   front trim leave room (120 of 128 at the 2x150 default: 32 registers per SIMD, a 256-lane workgroup of this fold, of losers
    //   or of winners per CU; ~100 for the general forms) and the chain runs through while the Stats kernel does
    //   (profiles/r07_a_step_timeline.txt; fastp_gpu_debug_kernel_regs and FASTP_GPU_VERBOSE's line at create say what fits).
    //   The order stays: behind Duplicate's kernels the fold was 27 + 9 us at the very end of every step.
    // MISC_LAST_ON_TAIL: beside the Stats kernel, behind Duplicate's chain / the text kernel, when that stream is in use
    // MISC_ON_LAUNCH_STREAM: behind the Stats fold
    MiscFold misc_fold = MISC_WITH_STATS;
    // The overrepresentation analysis needs the records (and --dedup's decisions), nothing of the Stats kernel: OVR_EARLY_ON_TAIL, on
    // the tail stream BESIDE it (round 5; behind Duplicate's tail / the text kernel when they are there - they write record flags),
    // joined at the end; OVR_AT_END: the last thing on the launch stream; OVR_DEFERRED: the caller asks for it later
    // (FASTP_GPU_BATCH_DEFER_OVERREP, fastp_gpu_overrep_device)
    OvrPlace overrep = OVR_AT_END;
    bool stats = false;         // the Stats kernel as its own launch
    bool front_stats = false;   // --cut_front on the lane plan: the reads whose own front is beyond the mate's common one (fq_stats5.h, front_stats_body)
    bool corr_stats = false;    // -c: the corrected positions' share of the POST Stats moves from the original base / quality to the corrected one
    // scan state of the whole batch: positions [b->n][B] u64, then masks [b->n] u8
    u64* scan_pos = nullptr;
    u8* scan_mask = nullptr;
};

static LaunchPlan plan_launch(const fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, int first, int n, ChunkMode mode, u8* scan_state) {
    const Switches& sw = ctx->sw;
    const DevParams& dp = ctx->dp;
    const bool stream = mode == CHUNK_STREAM;
    LaunchPlan p;
    p.mode = mode;
    if (b->n_exotic > 0) {
        p.xk0 = (int)(std::lower_bound(b->exotic_unit, b->exotic_unit + b->n_exotic, first) - b->exotic_unit);
        p.xk1 = (int)(std::lower_bound(b->exotic_unit, b->exotic_unit + b->n_exotic, first + n) - b->exotic_unit);
    }
    p.exact = n > 0 && (ctx->exact_all || p.xk1 > p.xk0);
    p.xskip = p.exact && ctx->lane && stream && !dp.dedup;
    const size_t so = (size_t)first * dp.sw_g * 4, qo = (size_t)first * dp.qw_g * 4;
    const bool aligned = rows_aligned16(dp.paired, (const char*)b->seq1 + so, (const char*)b->qual1 + qo, (const char*)b->seq2 + so, (const char*)b->qual2 + qo);
    p.align_rows = ctx->lane && !aligned && dp.merge_lane;
    const bool use_lane = ctx->lane && (aligned || p.align_rows);
    p.kernel = use_lane ? K_LANE : !ctx->split ? K_FUSED : ctx->cfg.threads > 256 ? K_SCAN_WIDE : K_SCAN;
    p.dedup_folded = dp.dedup && use_lane && stream && !p.exact && !dp.merge_lane && sw.dedup_fold &&
                     sw.claim_fused;   // (the fold IS the fused claim: without it the hash pre-pass decides)
    p.dedup_prepass = dp.dedup && !p.dedup_folded && stream;
    p.text_prepass = p.exact && (p.dedup_prepass || (mode == CHUNK_PASS1 && dp.dedup));
    const bool exact_early = p.xskip && use_lane;
    p.text = !p.exact ? TEXT_NONE : exact_early ? TEXT_BESIDE_LANE : (ctx->split && stream && !dp.dedup) ? TEXT_BEHIND_ON_TAIL : TEXT_INLINE;
    const bool text_on_tail = p.text == TEXT_BESIDE_LANE || p.text == TEXT_BEHIND_ON_TAIL;
    p.corr_list = ctx->split && dp.corr_lane && mode != CHUNK_OVERREP && !(mode == CHUNK_PASS1 && dp.dedup);
    p.claim_fused = dp.dup_enabled && (!dp.dedup || p.dedup_folded) && stream && (dp.dup_bufnum <= 2 || p.dedup_folded) &&
                    sw.claim_fused && (!p.exact || exact_early);
    p.clears_on_tail = ctx->split && !p.dedup_folded && n > 0;
    if (p.dedup_folded && p.claim_fused && n > 0) p.dup_place = DUP_BEFORE_STATS;
    else if (ctx->split && p.claim_fused && n > 0) p.dup_place = DUP_ON_TAIL;
    else if (text_on_tail) p.dup_place = dp.dup_enabled ? DUP_ON_TAIL : DUP_NOWHERE;
    else if (dp.dup_enabled && !dp.dedup) p.dup_place = DUP_AT_END;
    p.join_tail = p.dup_place == DUP_ON_TAIL || (text_on_tail && p.dup_place == DUP_NOWHERE);
    p.misc_fold = !ctx->split ? MISC_WITH_STATS : !p.join_tail ? MISC_ON_LAUNCH_STREAM : (p.claim_fused ? MISC_FIRST_ON_TAIL : MISC_LAST_ON_TAIL);
    p.overrep = (dp.overrep && !(b->flags & FASTP_GPU_BATCH_DEFER_OVERREP) && ctx->split && stream && n > 0) ? OVR_EARLY_ON_TAIL
                : (b->flags & FASTP_GPU_BATCH_DEFER_OVERREP) ? OVR_DEFERRED : OVR_AT_END;
    p.stats = ctx->split && n > 0;
    p.front_stats = p.stats && dp.front_per_read && ctx->lane;
    p.corr_stats = p.stats && p.corr_list;
    if (scan_state) {
        p.scan_pos = (u64*)scan_state + (size_t)first * dp.dup_bufnum;
        p.scan_mask = scan_state + (size_t)b->n * dp.dup_bufnum * 8 + first;
    }
    return p;
}

struct Launch {   // one launch: what its stage functions share
    fastp_gpu_ctx* ctx;
    const fastp_gpu_batch* b;
    int first, n;
    hipStream_t st;              // the launch stream (ctx->tail is the other one)
    const LaunchPlan p;
    KernelArgs a;
    const u16* true_len[2];      // a.len[] before the text kernel's units were emptied in it
    int grid, ln_grid, st_grid;  // workgroups (= slabs to fold) of the tile kernel, the lane kernel, the Stats kernel
};

static int fill_kernel_args(Launch& l, const fastp_gpu_results* res) {
    fastp_gpu_ctx* ctx = l.ctx;
    const fastp_gpu_batch* b = l.b;
    const int first = l.first;
    KernelArgs& a = l.a;
    memset(&a, 0, sizeof(a));
    a.p = ctx->dp;
    a.lut.ov_limit = (const u16*)ctx->d_ov_limit;
    a.lut.lowq_limit = ctx->d_lowq;
    a.lut.cplx_min = ctx->d_cplx;
    a.lut.dup_primes = ctx->d_primes;
    a.lut.dup_planes = ctx->d_planes;
    a.lut.dup_posum = ctx->d_posum;
    a.lut.fasta_words = ctx->d_fasta_words;
    a.lut.fasta_len = ctx->d_fasta_len;
    a.L = ctx->L;
    a.magic_sw = magic_for((u32)ctx->L.SW);
    a.magic_qwg = magic_for((u32)ctx->dp.qw_g);
    a.magic_swg = magic_for((u32)ctx->dp.sw_g);
    {   // vector (16-byte) tile copies need aligned rows and a tile that fits the registers
        const size_t qchunks = (size_t)ctx->L.NR * ctx->dp.qw_g / 4, schunks = (size_t)ctx->L.NR * ctx->dp.sw_g / 4;
        const size_t tile_threads = (size_t)ctx->cfg.threads;
        const bool ok = (ctx->L.P % 2 == 0) && (first % 2 == 0) && qchunks <= (size_t)PF_Q * tile_threads &&
                        schunks <= (size_t)PF_S * tile_threads && (size_t)ctx->L.NR <= tile_threads &&
                        rows_aligned16(ctx->dp.paired, b->seq1, b->qual1, b->seq2, b->qual2);
        a.prefetch = ok ? 2 : 0;
    }
    a.n = l.n;
    a.first = first;
    a.batch_flags = b->flags;
    const size_t swg = ctx->dp.sw_g, qwg = ctx->dp.qw_g;
    a.seq[0] = (const u32*)b->seq1 + (size_t)first * swg;
    a.qual[0] = (const u32*)b->qual1 + (size_t)first * qwg;
    a.len[0] = b->len1 + first;
    if (res) a.res[0] = (u32*)res->r1 + (size_t)first * 3;
    if (ctx->dp.paired) {
        a.seq[1] = (const u32*)b->seq2 + (size_t)first * swg;
        a.qual[1] = (const u32*)b->qual2 + (size_t)first * qwg;
        a.len[1] = b->len2 + first;
        if (res) {
            a.res[1] = (u32*)res->r2 + (size_t)first * 3;
            a.pair = (u32*)res->pair + (size_t)first * 2;
        }
    }
    if (res) {
        a.corrections = (ctx->dp.correction && res->corrections && res->n_corrections) ? (u32*)res->corrections : nullptr;
        a.corr_capacity = res->corrections_capacity;
        a.n_corrections = res->n_corrections;
        a.adapter_events = (ctx->dp.n_fasta && res->adapter_events && res->n_adapter_events) ? (u32*)res->adapter_events : nullptr;
        a.adapter_events_capacity = res->adapter_events_capacity;
        a.n_adapter_events = res->n_adapter_events;
    }
    l.true_len[0] = a.len[0];
    l.true_len[1] = a.len[1];
    a.split = ctx->split ? 1 : 0;
    a.phase_cycles = ctx->d_phase;
    // The product library has no switch that changes a result: FASTP_GPU_DEBUG_SKIP (steps left out of the kernels, for the measured
    // floors under profiles/) exists only in a library built with -DFQ_PROFILE_ABLATION (tools/build_ablation.sh).  Bit 512 is a TEST
    // switch that leaves every result as it is (each merged read's second part counted by the lane kernel, fq_lane.h).
#ifdef FQ_PROFILE_ABLATION
    a.debug_skip = (u32)ctx->sw.debug_skip & ~512u;
#else
    a.debug_skip = 0;
#endif
    if (ctx->sw.test_merge_slow) a.debug_skip |= 512u;
    a.slabs = ctx->d_slabs;
    a.slab_dwords = ctx->slab_dwords;
    a.tiles = (l.n + ctx->L.P - 1) / ctx->L.P;
    l.grid = a.tiles < ctx->blocks ? a.tiles : ctx->blocks;
    return 0;
}

// the plan's kernels see the text kernel's units as EMPTY: the launch's copies of the length arrays, and the lane kernel's list of
// the units not to write
static int mask_exotic_units(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    const int n = l.n, mates = ctx->dp.paired ? 2 : 1;
    int rx = ensure(ctx, (void**)&ctx->d_x_len, &ctx->x_len_cap, (size_t)2 * n * sizeof(u16));
    if (rx) return rx;
    for (int m = 0; m < mates; m++) {
        u16* copy = ctx->d_x_len + (size_t)m * n;
        if (ctx->exact_all) HIP_TRY(ctx, hipMemsetAsync(copy, 0, (size_t)n * sizeof(u16), l.st));
        else HIP_TRY(ctx, hipMemcpyAsync(copy, l.a.len[m], (size_t)n * sizeof(u16), hipMemcpyDeviceToDevice, l.st));
        l.a.len[m] = copy;
    }
    u8* skip = nullptr;
    if (l.p.xskip) {
        rx = ensure(ctx, (void**)&ctx->d_x_skip, &ctx->x_skip_cap, (size_t)n);
        if (rx) return rx;
        skip = ctx->d_x_skip;
        HIP_TRY(ctx, hipMemsetAsync(skip, ctx->exact_all ? 1 : 0, (size_t)n, l.st));
        if (l.p.text == TEXT_BESIDE_LANE) l.a.xskip = skip;
    }
    if (!ctx->exact_all) {
        TextMaskArgs mk;
        mk.units = ctx->d_x_unit + l.p.xk0;
        mk.count = l.p.xk1 - l.p.xk0;
        mk.first = l.first;
        mk.skip = skip;
        mk.len[0] = ctx->d_x_len;
        mk.len[1] = mates == 2 ? ctx->d_x_len + n : nullptr;
        hipLaunchKernelGGL(fq_text_mask_kernel, dim3((mk.count + 255) / 256), dim3(256), 0, l.st, mk);
        HIP_TRY(ctx, hipGetLastError());
    }
    return 0;
}

// the engine's buffers a launch of n units needs, whatever the mode
static int fill_launch_buffers(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    KernelArgs& a = l.a;
    const int n = l.n;
    int rc;
    if (ctx->dp.dup_enabled && l.p.mode != CHUNK_OVERREP) {
        rc = ensure(ctx, (void**)&ctx->d_dup_pos, &ctx->dup_pos_cap, (size_t)n * ctx->dp.dup_bufnum * 8);
        if (rc) return rc;
        a.dup_pos = ctx->d_dup_pos;
    }
    if (l.p.corr_list) {
        // the engine's own correction list of this launch.  A pair can have as many edits as its overlap is long (only the first
        // 50 bases are held to the mismatch limit, overlapanalysis.cpp:34-44): the list is sized for that - it cannot overflow,
        // and set_launch_size keeps it below 2^29 entries (2^30 where the card has the memory to spare: laid out for 288 GB of HBM)
        const size_t cap = (size_t)n * (size_t)ctx->dp.max_len;
        rc = ensure(ctx, (void**)&ctx->d_corr_int, &ctx->corr_int_cap, (cap * 2 + 4) * 4);
        if (rc) return rc;
        a.n_corr_int = (int*)ctx->d_corr_int;
        a.corr_int = ctx->d_corr_int + 4;
        a.corr_int_cap = (int)std::min<size_t>(cap, 0x7FFFFFFF);
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_corr_int, 0, 16, l.st));
    }
    if (ctx->split)
        for (int m = 0; m < 2; m++) {
            rc = ensure(ctx, (void**)&ctx->d_swin[m], &ctx->swin_cap[m], ((size_t)n * 4 + 255) & ~(size_t)255);
            if (rc) return rc;
            a.swin_out[m] = ctx->d_swin[m];
        }
    if (l.p.align_rows)
        for (int k = 0; k < 4; k++) {
            const size_t bytes = (size_t)n * (size_t)((k & 1) ? ctx->dp.qw_g : ctx->dp.sw_g) * 4;
            rc = ensure(ctx, (void**)&ctx->d_al[k], &ctx->al_cap[k], bytes + 256);
            if (rc) return rc;
            const u32* src = (k & 1) ? a.qual[k >> 1] : a.seq[k >> 1];
            if (bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_al[k], src, bytes, hipMemcpyDeviceToDevice, l.st));
            if (k & 1) a.qual[k >> 1] = ctx->d_al[k]; else a.seq[k >> 1] = ctx->d_al[k];
        }
    return 0;
}

// the text kernel (fq_text.h): a wavefront per listed unit, its texts in the wavefront's stretch of LDS, Stats' per-base
// counters in the workgroup's LDS tables (added to d_ctr once), everything else straight into d_ctr
static int launch_text(Launch& l, int hash_only, hipStream_t st) {
    fastp_gpu_ctx* ctx = l.ctx;
    const fastp_gpu_batch* b = l.b;
    TextArgs e;
    memset(&e, 0, sizeof(e));
    e.k = l.a;
    e.c = ctx->t_text_ctr;
    e.ctr = ctx->d_ctr;
    e.k.len[0] = l.true_len[0];
    e.k.len[1] = l.true_len[1];
    e.x_n = b->n_exotic;
    e.x_unit = ctx->d_x_unit;
    e.x_all = ctx->exact_all ? 1 : 0;
    e.x_k0 = l.p.xk0;
    e.x_count = ctx->exact_all ? l.n : l.p.xk1 - l.p.xk0;
    e.x_dense = b->exotic_dense;
    for (int m = 0; m < 2; m++) { e.x_text[m] = b->exotic_text[m]; e.x_off[m] = b->exotic_off[m]; }
    e.ML = (ctx->dp.max_len + 8 + 7) & ~7;
    e.hash_only = hash_only;
    // Stats' per-base tables of a workgroup in LDS when they fit beside the wavefronts' texts (not the hash pre-pass, which
    // counts nothing; reads too long for it add to the block with global atomics)
    const size_t text_bytes = (size_t)TEXT_WAVES * text_wave_bytes(e.ML);
    const int slot_dwords = 34 * (int)ctx->cl.cycles + 1024 + 128;
    const int slots = !ctx->dp.paired ? 2 : ctx->dp.merge ? 3 : 4;   // the Stats objects a unit can reach
    const bool lds_tables = !hash_only && (size_t)slots * slot_dwords * 4 + text_bytes <= (size_t)aux_lds_cap(ctx);
    e.lds_slot_dwords = lds_tables ? slot_dwords : 0;
    e.lds_slots = lds_tables ? slots : 0;
    const int blocks = std::max(1, std::min((e.x_count + TEXT_WAVES - 1) / TEXT_WAVES, ctx->cus));
    hipLaunchKernelGGL(fq_text_kernel, dim3(blocks), dim3(64 * TEXT_WAVES), (size_t)e.lds_slots * e.lds_slot_dwords * 4 + text_bytes, st, e);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// Duplicate's kernels of a launch share one argument block and the buffers behind it
static int dup_args(Launch& l, u8* dupflag, bool scan, DupArgs* out) {
    fastp_gpu_ctx* ctx = l.ctx;
    DupArgs& d = *out;
    memset(&d, 0, sizeof(d));
    if (scan) { d.scan_pos = l.p.scan_pos; d.scan_mask = l.p.scan_mask; }
    d.dup_pos = ctx->dp.dup_enabled && l.p.mode != CHUNK_OVERREP ? ctx->d_dup_pos : nullptr;
    d.posum = ctx->d_posum;
    d.len[0] = l.a.len[0];
    d.len[1] = l.a.len[1];
    d.n = l.n;
    d.B = ctx->dp.dup_bufnum;
    d.bits = ctx->dp.dup_bits;
    d.bitmap = ctx->d_bitmap;
    int lg = 10;
    while ((1ull << lg) < (size_t)l.n * d.B * 2) lg++;
    int rc = ensure(ctx, (void**)&ctx->d_table, &ctx->table_cap, (size_t)8 << lg);
    if (rc) return rc;
    rc = ensure(ctx, (void**)&ctx->d_need, &ctx->need_cap, (size_t)l.n);
    if (rc) return rc;
    d.table = ctx->d_table;
    d.table_log2 = lg;
    d.need = ctx->d_need;
    d.res[0] = l.a.res[0];
    d.res[1] = l.a.res[1];
    d.dupflag = dupflag;
    d.paired = ctx->dp.paired;
    d.ctr_total = ctx->d_ctr + ctx->cl.dup_total;
    d.ctr_dups = ctx->d_ctr + ctx->cl.dup_count;
    rc = ensure(ctx, (void**)&ctx->d_setw, &ctx->setw_cap, (size_t)l.n);
    if (rc) return rc;
    if (!ctx->d_cfilter) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cfilter, (size_t)1 << (DUP_CF_LOG2 - 3)));
    d.setw = ctx->d_setw;
    d.cfilter = ctx->d_cfilter;
    return 0;
}
// the buffers + clears in front of a per-read kernel that claims
static int dup_prepare(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    DupArgs d;
    const int rc = dup_args(l, nullptr, false, &d);
    if (rc) return rc;
    hipStream_t cst = l.p.clears_on_tail ? ctx->tail : l.st;
    HIP_TRY(ctx, hipMemsetAsync(d.table, 0xFF, (size_t)8 << d.table_log2, cst));
    HIP_TRY(ctx, hipMemsetAsync(d.cfilter, 0, (size_t)1 << (DUP_CF_LOG2 - 3), cst));
    l.a.claim_won = ctx->d_need;
    l.a.dup_bitmap = ctx->d_bitmap;
    l.a.dup_bits = ctx->dp.dup_bits;
    return 0;
}
// losers (behind a per-read kernel that claimed) or claim, then winners and finish
static int dup_decide(Launch& l, const DupArgs& d, bool claimed, hipStream_t st) {
    fastp_gpu_ctx* ctx = l.ctx;
    const int g2 = std::max(1, (l.n + 255) / 256);  // one unit per lane: the kernels are chains of dependent random accesses
    if (claimed) hipLaunchKernelGGL(fq_dup_losers_kernel, dim3(g2), dim3(256), 0, st, d);
    else hipLaunchKernelGGL(fq_dup_claim_kernel, dim3(g2), dim3(256), 0, st, d);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_dup_winners_kernel, dim3(g2), dim3(256), 0, st, d);
    HIP_TRY(ctx, hipGetLastError());
    // (1024 unless a smaller workgroup is what fits beside the Stats kernel, fastp_gpu_create - and this launch's finish runs there:
    // on the tail stream, in front of a Stats kernel; alone on the chip the large workgroup is the faster one)
    const int ft = st == ctx->tail && l.p.stats ? ctx->finish_threads : 1024;
    hipLaunchKernelGGL(fq_dup_finish_kernel, dim3(std::max(1, (l.n + ft - 1) / ft)), dim3(ft), 16, st, d);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
// what follows that kernel
static int dup_tail(Launch& l, u8* dupflag, hipStream_t st) {
    DupArgs d;
    const int rc = dup_args(l, dupflag, false, &d);
    return rc ? rc : dup_decide(l, d, true, st);
}
// everything, with the claim as its own kernel (scan: pass 1 of a sharded run keeps the scan state)
static int dup_claim_chain(Launch& l, u8* dupflag, bool scan, hipStream_t st) {
    fastp_gpu_ctx* ctx = l.ctx;
    DupArgs d;
    const int rc = dup_args(l, dupflag, scan, &d);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d.table, 0xFF, (size_t)8 << d.table_log2, st));
    HIP_TRY(ctx, hipMemsetAsync(d.cfilter, 0, (size_t)1 << (DUP_CF_LOG2 - 3), st));
    return dup_decide(l, d, false, st);
}
// the hash pass in front of the worker loop -> Duplicate's chain (--dedup: with dupflag, its decisions; pass 1 of a sharded
// run: the scan state)
static int hash_prepass(Launch& l, u8* dupflag, bool scan) {
    fastp_gpu_ctx* ctx = l.ctx;
    hipLaunchKernelGGL(fq_hash_kernel, dim3(l.grid), dim3(ctx->cfg.threads), (size_t)ctx->L.total * 4, l.st, l.a);
    HIP_TRY(ctx, hipGetLastError());
    if (l.p.text_prepass) {
        const int rc = launch_text(l, 1, l.st);
        if (rc) return rc;
    }
    return dup_claim_chain(l, dupflag, scan, l.st);
}
// pass 2 of a sharded run: the decision comes from pass 1's scan state + the preceding shards' bitmaps; nothing is hashed again
static int pass2_decide(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    DupFinalArgs d;
    memset(&d, 0, sizeof(d));
    d.scan_pos = l.p.scan_pos;
    d.scan_mask = l.p.scan_mask;
    d.prefix = ctx->has_prefix ? ctx->d_prefix : nullptr;
    d.bits = ctx->dp.dup_bits;
    d.n = l.n;
    d.B = ctx->dp.dup_bufnum;
    d.dupflag = ctx->dp.dedup ? ctx->d_dupflag : nullptr;
    d.res[0] = l.a.res[0];
    d.res[1] = l.a.res[1];
    d.paired = ctx->dp.paired;
    d.ctr_total = ctx->d_ctr + ctx->cl.dup_total;
    d.ctr_dups = ctx->d_ctr + ctx->cl.dup_count;
    hipLaunchKernelGGL(fq_dup_final_kernel, dim3((l.n + 255) / 256), dim3(256), 16, l.st, d);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
// --dedup folded: Duplicate's decisions taken out of the records and the POST Stats' read counts before the Stats kernel counts
static int dedup_apply(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    DedupApplyArgs da;
    memset(&da, 0, sizeof(da));
    da.n = l.n;
    da.paired = ctx->dp.paired;
    da.dupflag = ctx->d_dupflag;
    for (int m = 0; m < 2; m++) {
        da.res[m] = l.a.res[m];
        da.swin[m] = ctx->d_swin[m];
        da.st_reads[m] = ctx->d_ctr + ctx->cl.stats[2 * m + 1] + ctx->cl.st_reads;
        da.st_lensum[m] = ctx->d_ctr + ctx->cl.stats[2 * m + 1] + ctx->cl.st_length_sum;
    }
    hipLaunchKernelGGL(fq_dedup_apply_kernel, dim3((l.n + 255) / 256), dim3(256), 16, l.st, da);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the overrepresentation analysis reads the rows by their TRUE lengths, and the listed units' symbols from their text
static int overrep(Launch& l, hipStream_t st) {
    KernelArgs ao = l.a;
    ao.len[0] = l.true_len[0];
    ao.len[1] = l.true_len[1];
    return launch_overrep(l.ctx, ao, l.n, st, l.b);
}

static int launch_per_read(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    const KernelArgs& a = l.a;
    hipStream_t st = l.st;
    const int n = l.n;
    if (l.p.kernel == K_LANE) {
        LaneArgs la = ctx->t_lane;
        la.k = a;
        la.k.slabs = ctx->d_ln_slabs;
        la.k.slab_dwords = ctx->ln_lds.n_misc;
        const int Bh = (ctx->dp.dup_enabled && (a.dup_pos || a.claim_won) && !(a.debug_skip & 2u)) ? ctx->dp.dup_bufnum : 0;
        lane_kernel_fn fn = lane_kernel_for(ctx->ln_swm, Bh, ctx->dp.paired != 0, lane_ext(ctx->dp));
        l.ln_grid = std::max(1, std::min(ctx->ln_blocks, (n + 255) / 256));
        hipLaunchKernelGGL(fn, dim3(l.ln_grid), dim3(ctx->ln_threads), (size_t)ctx->ln_lds.total * 4, st, la);
    } else if (l.p.kernel == K_SCAN_WIDE) hipLaunchKernelGGL(fq_scan_wide_kernel, dim3(l.grid), dim3(ctx->cfg.threads), (size_t)ctx->L.total * 4, st, a);
    else if (l.p.kernel == K_SCAN) hipLaunchKernelGGL(fq_scan_kernel, dim3(l.grid), dim3(ctx->cfg.threads), (size_t)ctx->L.total * 4, st, a);
    else hipLaunchKernelGGL(fq_fused_kernel, dim3(l.grid), dim3(ctx->cfg.threads), (size_t)ctx->L.total * 4, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// Stats::statRead of the launch's units: a workgroup takes a run of consecutive units (at most CYC_MAX_READS:
// packed counters; at least 64 so that small launches do not pay a 43 KB slab per handful of reads)
static int launch_stats(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    const int n = l.n;
    StatsArgs sa = ctx->t_stats;
    sa.n = n;
    // whole rounds of the resident workgroups: 4.19 M pairs = 3 rounds of 512 workgroups with 2731 units each in form 4
    const int rounds = (int)(((long long)n + (long long)ctx->st_blocks * ctx->st_max_reads - 1) / ((long long)ctx->st_blocks * ctx->st_max_reads));
    int upb = (n + ctx->st_blocks * rounds - 1) / (ctx->st_blocks * rounds);
    upb = std::max(upb, std::min(n, 64));
    if (upb > ctx->st_max_reads) return fail(ctx, FASTP_GPU_E_INVALID, "launch too large for the Stats kernel");
    sa.units_per_block = upb;
    const int st_grid = (n + upb - 1) / upb;
    if (st_grid > ctx->st_max_grid) return fail(ctx, FASTP_GPU_E_INVALID, "launch too large for the Stats kernel's slabs");
    for (int m = 0; m < 2; m++) {
        sa.seq[m] = l.a.seq[m];
        sa.qual[m] = l.a.qual[m];
        sa.swin[m] = ctx->d_swin[m];
        sa.fr_rec[m] = ctx->dp.front_per_read ? (const u32*)l.a.res[m] : ctx->d_swin[m];
    }
    sa.debug_skip = l.a.debug_skip;
    if (l.a.debug_skip & 16u) return 0;   // (profiling builds: no Stats kernel, nothing of it to fold)
    if (ctx->st_form == 5) {
        stats5_kernel_fn fq_stats5_kernel = ctx->st5_fn;   // (form 5 under its one name, whichever instantiation: what a launch trace shows)
#ifdef FQ_PROFILE_ABLATION
        if ((sa.debug_skip & 0xC0u) && sa.Hs == 10 && sa.kc == 2) fq_stats5_kernel = stats5_kernel_for(ST5_ABLATION);
#endif
        hipLaunchKernelGGL(fq_stats5_kernel, dim3(st_grid), dim3(ctx->st_threads), (size_t)ctx->st_lds_dwords * 4, l.st, sa);
    } else hipLaunchKernelGGL(fq_stats_kernel, dim3(st_grid), dim3(ctx->st_threads), (size_t)ctx->st_lds_dwords * 4, l.st, sa);
    HIP_TRY(ctx, hipGetLastError());
    l.st_grid = st_grid;
    return 0;
}

static int launch_front_stats(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    FrontStatsArgs fs = ctx->t_front;
    fs.n = l.n;
    for (int m = 0; m < 2; m++) {
        fs.seq[m] = l.a.seq[m];
        fs.qual[m] = l.a.qual[m];
        fs.swin[m] = ctx->d_swin[m];
        fs.rec[m] = (const u32*)l.a.res[m];
    }
    const size_t reads = (size_t)l.n * (ctx->dp.paired ? 2 : 1);
    const int fgrid = (int)std::max<size_t>(1, std::min<size_t>((size_t)ctx->cus * 4, (reads + 255) / 256));
    hipLaunchKernelGGL(fq_front_stats_kernel, dim3(fgrid), dim3(256), front_stats_lds_bytes(ctx), l.st, fs);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

static int launch_corr_stats(Launch& l) {
    fastp_gpu_ctx* ctx = l.ctx;
    const KernelArgs& a = l.a;
    const size_t reads = (size_t)l.n * (ctx->dp.paired ? 2 : 1);
    const int rc = ensure(ctx, (void**)&ctx->d_corr_chain, &ctx->corr_chain_cap, (reads + (size_t)a.corr_int_cap) * 4);
    if (rc) return rc;
    OvrArgs lo;
    memset(&lo, 0, sizeof(lo));
    lo.n = l.n;
    lo.first = a.first;
    lo.paired = ctx->dp.paired;
    lo.corr = a.corr_int;
    lo.n_corr = a.n_corr_int;
    lo.corr_cap = a.corr_int_cap;
    lo.corr_head = ctx->d_corr_chain;
    lo.corr_next = ctx->d_corr_chain + reads;
    HIP_TRY(ctx, hipMemsetAsync(lo.corr_head, 0, reads * 4, l.st));
    // (one lane per possible entry would be n x limit lanes; the list is short - a grid-stride walk over what it holds)
    hipLaunchKernelGGL(fq_corr_link_kernel, dim3(std::min(4096, (a.corr_int_cap + 255) / 256)), dim3(256), 0, l.st, lo);
    HIP_TRY(ctx, hipGetLastError());
    CorrStatsArgs cs = ctx->t_corr;
    cs.n = l.n;
    for (int m = 0; m < 2; m++) { cs.seq[m] = a.seq[m]; cs.qual[m] = a.qual[m]; cs.swin[m] = ctx->d_swin[m]; }
    cs.corr = a.corr_int;
    cs.corr_head = lo.corr_head;
    cs.corr_next = lo.corr_next;
    // persistent workgroups: the deltas of a workgroup's reads meet in its LDS tables first (corr_stats_body)
    const int cgrid = (int)std::max<size_t>(1, std::min<size_t>((size_t)ctx->cus * 2, (reads + 1023) / 1024));
    hipLaunchKernelGGL(fq_corr_stats_kernel, dim3(cgrid), dim3(1024), corr_stats_lds_bytes(ctx), l.st, cs);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// The slab folds.  FOLD_STATS in a split plan: the Stats kernel's slabs (per-cycle u64s, k-mer counters, one histogram counter per
// (slot, character)); FOLD_MISC: the per-read kernel's slabs, the MISC_* counters only; both at once: the fused kernel's slabs
// Which kernel: FOLD_GROUPS is fq_reduce_kernel (a lane per slab element and group of REDUCE_GROUP slabs, a serial walk), FOLD_WIDE
// fq_reduce_wide_kernel (the same item over a larger group, split over a workgroup's waves, WIDE_UNROLL loads in flight; Stats slabs only).  FOLD_AUTO, what a launch asks for:
// the wide one where the Stats fold has more than one slab group, i.e. where the serial walk is REDUCE_GROUP loads long and the
// grid under a wave per SIMD; every smaller fold and every MISC fold is fq_reduce_kernel as before.
enum { FOLD_STATS = 1, FOLD_MISC = 2 };
enum { FOLD_AUTO = -1, FOLD_GROUPS = 0, FOLD_WIDE = 1 };
// stats_slabs / nblocks: the slabs of a FOLD_STATS fold (the launch's own, or a caller's: fastp_gpu_debug_stats_fold)
static int fold_slabs(fastp_gpu_ctx* ctx, int parts, bool lane, const u32* stats_slabs, int nblocks, hipStream_t st, int which) {
    ReduceArgs r = ctx->t_reduce;
    r.parts = parts;
    if (parts == FOLD_STATS) {
        r.slabs = stats_slabs;
        r.slab_dwords = ctx->st_slab_dwords;
        r.nblocks = nblocks;
        r.off_kmer = 4 * N_CLS * ctx->L.Cp * 2;
        r.off_qh = r.off_kmer + 4 * KMER_BINS;
        r.qh_stride = 1;
        r.qh_count = 0;
    } else {
        r.slabs = lane ? ctx->d_ln_slabs : ctx->d_slabs;
        r.slab_dwords = lane ? ctx->ln_lds.n_misc : ctx->slab_dwords;
        r.nblocks = nblocks;
        r.off_misc = lane ? 0 : ctx->L.acc_misc - ctx->L.acc_cyc;
        r.off_kmer = ctx->L.acc_kmer - ctx->L.acc_cyc;
        r.off_qh = ctx->L.acc_qh - ctx->L.acc_cyc;
        r.qh_stride = QT_DWORDS;
        r.qh_count = QT_COUNT;
    }
    if (r.nblocks <= 0) return 0;
    const int n_stats = 4 * N_CLS * ctx->L.Cp + 4 * KMER_BINS + 4 * 128, n_misc = MISC_ISIZE + r.isize_max + 1 + (r.merge_tail ? (int)KMER_BINS : 0);
    const int items = ((parts & FOLD_STATS) ? n_stats : 0) + ((parts & FOLD_MISC) ? n_misc : 0);
    const bool wide = parts == FOLD_STATS && (which == FOLD_WIDE || (which == FOLD_AUTO && r.nblocks > REDUCE_GROUP));
    if (parts == FOLD_STATS) ctx->last_stats_fold = wide ? FOLD_WIDE : FOLD_GROUPS;
    if (wide) {
        const int wgroups = (r.nblocks + WIDE_GROUP - 1) / WIDE_GROUP;
        hipLaunchKernelGGL(fq_reduce_wide_kernel, dim3(((items + WIDE_ITEMS - 1) / WIDE_ITEMS) * wgroups), dim3(WIDE_THREADS), (size_t)WIDE_LDS_DWORDS * 4, st, r);
    } else {
        const int rgroups = (r.nblocks + REDUCE_GROUP - 1) / REDUCE_GROUP;
        hipLaunchKernelGGL(fq_reduce_kernel, dim3(((items + 255) / 256) * rgroups), dim3(256), 0, st, r);
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}
static int fold(Launch& l, int parts, hipStream_t st) {
    const bool lane = l.p.kernel == K_LANE;
    return fold_slabs(l.ctx, parts, lane, l.ctx->d_st_slabs, parts == FOLD_STATS ? l.st_grid : lane ? l.ln_grid : l.grid, st, FOLD_AUTO);
}

// debugging aid (not part of the drop-in surface): the Stats fold on its own, and what the context chose for the step's tail.
// slabs != nullptr: fold `nblocks` device slabs of this context's Stats-slab layout ([nblocks][info[2]] dwords, 8-byte aligned: per
// slot, cycle (info[3] of them, the first info[4] in use) and class one packed u64, then 4 x KMER_BINS and 4 x 128 counters) into
// the context's counter block, on the context's stream, through fold_slabs as a launch does: which = 0 fq_reduce_kernel, 1 the wide
// fold, -1 what a launch of that many slabs takes.  The slabs stay the caller's and must outlive the fold (fastp_gpu_synchronize).
// info (n >= 9): {fq_dup_finish_kernel's workgroup size, the fold the most recent Stats fold took (0 / 1 as above, -1: none yet),
// slab dwords, Cp, C, REDUCE_GROUP, WIDE_GROUP, WIDE_UNROLL, WIDE_PARTS}.
extern "C" int fastp_gpu_debug_stats_fold(fastp_gpu_ctx* ctx, const void* slabs, int32_t nblocks, int32_t which, int32_t* info, int32_t n) {
    if (!ctx || !info || n < 9) return FASTP_GPU_E_INVALID;
    if (slabs) {
        if (!ctx->split || ctx->st_slab_dwords <= 0) return fail(ctx, FASTP_GPU_E_INVALID, "the context has no Stats slabs");
        if (nblocks < 0 || which < FOLD_AUTO || which > FOLD_WIDE || ((size_t)slabs & 7)) return fail(ctx, FASTP_GPU_E_INVALID, "bad slab fold arguments");
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const int rc = fold_slabs(ctx, FOLD_STATS, false, (const u32*)slabs, nblocks, ctx->stream, which);
        if (rc) return rc;
    }
    const int32_t out[9] = {ctx->finish_threads, ctx->last_stats_fold, ctx->st_slab_dwords, ctx->L.Cp, ctx->L.C, REDUCE_GROUP, WIDE_GROUP, WIDE_UNROLL, WIDE_PARTS};
    for (int i = 0; i < 9; i++) info[i] = out[i];
    return FASTP_GPU_OK;
}

// the tail stream goes on from where the launch stream is now
static int tail_follows(Launch& l) {
    HIP_TRY(l.ctx, hipEventRecord(l.ctx->ev_k1, l.st));
    HIP_TRY(l.ctx, hipStreamWaitEvent(l.ctx->tail, l.ctx->ev_k1, 0));
    return 0;
}

#define STEP(call)              \
    do {                        \
        const int rc_ = (call); \
        if (rc_) return rc_;    \
    } while (0)

// One launch: the schedule.  What runs, and where, is the plan's (LaunchPlan has the reasons); the order is this function's.
static int launch_chunk(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, int first, int n, const fastp_gpu_results* res,
                        hipStream_t st, ChunkMode mode = CHUNK_STREAM, u8* scan_state = nullptr) {
    Launch l{ctx, b, first, n, st, plan_launch(ctx, b, first, n, mode, scan_state)};
    const LaunchPlan& p = l.p;
    // every mode: the argument block, the text kernel's units emptied in it, the launch's buffers
    STEP(fill_kernel_args(l, res));
    if (p.exact) STEP(mask_exotic_units(l));
    STEP(fill_launch_buffers(l));

    // what runs in front of the worker loop, or instead of it
    if (mode == CHUNK_OVERREP) return overrep(l, st);
    if (mode == CHUNK_PASS1 && ctx->dp.dedup) return hash_prepass(l, nullptr, true);
    if (mode == CHUNK_PASS2 || p.dedup_prepass) {
        if (ctx->dp.dedup) STEP(ensure(ctx, (void**)&ctx->d_dupflag, &ctx->dupflag_cap, (size_t)n));
        if (mode == CHUNK_PASS2) STEP(pass2_decide(l));
        else STEP(hash_prepass(l, ctx->d_dupflag, false));
        if (!ctx->dp.dedup) return FASTP_GPU_OK;  // (pass 2 without --dedup) the records are pass 1's
        l.a.dup_pos = nullptr;   // --dedup: the per-read kernel reads the decision instead of hashing
        l.a.dupflag = ctx->d_dupflag;
    }

    // the worker loop: the per-read kernel, the text kernel around it
    if (p.claim_fused) STEP(dup_prepare(l));
    if (p.text == TEXT_BESIDE_LANE) {
        STEP(tail_follows(l));
        STEP(launch_text(l, 0, ctx->tail));
    }
    hipEvent_t e0, e1;
    STEP(get_events(ctx, &e0, &e1));
    HIP_TRY(ctx, hipEventRecord(e0, st));
    STEP(launch_per_read(l));
    if (p.text == TEXT_BESIDE_LANE) {
        // (launched in front of the plan's kernel) Duplicate's kernels need that kernel's hash values as well: the tail stream joins it
        STEP(tail_follows(l));
    } else if (p.text == TEXT_BEHIND_ON_TAIL) {
        STEP(tail_follows(l));
        STEP(launch_text(l, 0, ctx->tail));
    } else if (p.text == TEXT_INLINE) {
        STEP(launch_text(l, 0, st));
    }

    // Duplicate behind the per-read kernel, the MISC_* fold, the overrepresentation analysis: beside the Stats kernel where they can be
    if (p.dup_place == DUP_BEFORE_STATS) {
        STEP(ensure(ctx, (void**)&ctx->d_dupflag, &ctx->dupflag_cap, (size_t)n));
        STEP(dup_tail(l, ctx->d_dupflag, st));
        STEP(dedup_apply(l));
    }
    if (p.misc_fold == MISC_FIRST_ON_TAIL) {
        STEP(tail_follows(l));
        STEP(fold(l, FOLD_MISC, ctx->tail));
    }
    if (p.dup_place == DUP_ON_TAIL) STEP(p.claim_fused ? dup_tail(l, nullptr, ctx->tail) : dup_claim_chain(l, nullptr, false, ctx->tail));
    if (p.join_tail) HIP_TRY(ctx, hipEventRecord(ctx->ev_tail, ctx->tail));
    if (p.overrep == OVR_EARLY_ON_TAIL) {
        STEP(tail_follows(l));
        STEP(overrep(l, ctx->tail));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_tail, ctx->tail));   // (the launch stream waits for the tail stream below)
    }

    // the Stats kernel and what corrects its counts
    if (p.stats) STEP(launch_stats(l));
    if (p.front_stats && l.st_grid > 0) STEP(launch_front_stats(l));
    if (p.corr_stats && l.st_grid > 0) STEP(launch_corr_stats(l));
    HIP_TRY(ctx, hipEventRecord(e1, st));
    ctx->pending_events.push_back({e0, e1});

    // the folds; the launch stream joins the tail stream
    if (p.misc_fold == MISC_WITH_STATS) {
        STEP(fold(l, FOLD_STATS | FOLD_MISC, st));
    } else {
        STEP(fold(l, FOLD_STATS, st));
        if (p.misc_fold != MISC_FIRST_ON_TAIL) STEP(fold(l, FOLD_MISC, p.misc_fold == MISC_LAST_ON_TAIL ? ctx->tail : st));
        if (p.join_tail) HIP_TRY(ctx, hipEventRecord(ctx->ev_tail, ctx->tail));
    }
    if (p.join_tail) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_tail, 0));
    else if (p.dup_place == DUP_AT_END) STEP(p.claim_fused ? dup_tail(l, nullptr, st) : dup_claim_chain(l, nullptr, mode == CHUNK_PASS1, st));
    if (p.overrep == OVR_EARLY_ON_TAIL && !p.join_tail) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_tail, 0));
    return p.overrep == OVR_AT_END ? overrep(l, st) : FASTP_GPU_OK;
}


static int submit_chunks(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, const fastp_gpu_results* res, void* hip_stream,
                         ChunkMode mode, u8* scan_state) {
    if (!ctx || !b) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    const bool need_res = !(mode == CHUNK_PASS1 && ctx->dp.dedup);
    if (need_res && !res) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    if (b->n < 0) return fail(ctx, FASTP_GPU_E_INVALID, "negative batch size");
    if (!b->seq1 || !b->qual1 || !b->len1 || (need_res && !res->r1)) {
        if (b->n > 0) return fail(ctx, FASTP_GPU_E_INVALID, "missing read-1 buffers");
    }
    if (ctx->dp.paired && b->n > 0 && (!b->seq2 || !b->qual2 || !b->len2 || (need_res && (!res->r2 || !res->pair))))
        return fail(ctx, FASTP_GPU_E_INVALID, "paired engine needs read-2 buffers and pair results");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    const bool worker_loop = mode == CHUNK_STREAM || (mode == CHUNK_PASS1 && !ctx->dp.dedup) || (mode == CHUNK_PASS2 && ctx->dp.dedup);
    if (worker_loop) {
        ctx->last_corr = res->corrections;
        ctx->last_corr_cap = res->corrections ? res->corrections_capacity : 0;
        if (res->n_corrections) HIP_TRY(ctx, hipMemsetAsync(res->n_corrections, 0, sizeof(int32_t), st));
        if (ctx->dp.n_fasta && b->n > 0 && (!res->adapter_events || !res->n_adapter_events))
            return fail(ctx, FASTP_GPU_E_INVALID, "adapter_fasta needs an adapter event list in the results");
        if (res->n_adapter_events) HIP_TRY(ctx, hipMemsetAsync(res->n_adapter_events, 0, sizeof(int32_t), st));
    }
    if (b->n_exotic > 0) {
        // units with letters outside ACGTN: the text kernel (fq_text.h) takes them, launch by launch (launch_chunk)
        if (!b->exotic_unit || !b->exotic_text[0] || !b->exotic_off[0] || (ctx->dp.paired && (!b->exotic_text[1] || !b->exotic_off[1])))
            return fail(ctx, FASTP_GPU_E_INVALID, "n_exotic > 0 needs exotic_unit, exotic_text and exotic_off");
        for (int k = 0; k < b->n_exotic; k++)
            if (b->exotic_unit[k] < 0 || b->exotic_unit[k] >= b->n || (k && b->exotic_unit[k] <= b->exotic_unit[k - 1]))
                return fail(ctx, FASTP_GPU_E_INVALID, "exotic_unit must be ascending unit indexes of the batch");
        int rc = ensure(ctx, (void**)&ctx->d_x_unit, &ctx->x_unit_cap, (size_t)b->n_exotic * sizeof(int));
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_x_unit, b->exotic_unit, (size_t)b->n_exotic * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));   // the list is the caller's (pageable) memory
    }
    // split into equally sized launches (each a multiple of the tile size)
    const int launches = (b->n + ctx->max_pairs_per_launch - 1) / ctx->max_pairs_per_launch;
    int per = launches ? (b->n + launches - 1) / launches : 0;
    per = (per + ctx->L.P - 1) / ctx->L.P * ctx->L.P;
    for (int first = 0; first < b->n; first += per) {
        const int n = std::min(per, b->n - first);
        int rc = launch_chunk(ctx, b, first, n, res, st, mode, scan_state);
        if (rc) return rc;
    }
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_submit_device(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, fastp_gpu_results* res,
                                       void* hip_stream) {
    return submit_chunks(ctx, b, res, hip_stream, CHUNK_STREAM, nullptr);
}

// ---- sharded runs (include/fastp_gpu.h "Sharded runs") -------------------------------------
extern "C" int64_t fastp_gpu_dup_scan_bytes(const fastp_gpu_ctx* ctx, int32_t n) {
    if (!ctx || n < 0) return -1;
    return (int64_t)n * ctx->dp.dup_bufnum * 8 + (((int64_t)n + 15) & ~(int64_t)15);
}

extern "C" int fastp_gpu_submit_pass1_device(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, void* scan_state,
                                             fastp_gpu_results* res, void* hip_stream) {
    if (!ctx) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    if (!ctx->dp.dup_enabled) return submit_chunks(ctx, b, res, hip_stream, CHUNK_STREAM, nullptr);  // nothing depends on earlier units
    if (!scan_state || ((uintptr_t)scan_state & 7u)) return fail(ctx, FASTP_GPU_E_INVALID, "scan state must be an 8-byte aligned device buffer");
    return submit_chunks(ctx, b, res, hip_stream, CHUNK_PASS1, (u8*)scan_state);
}

extern "C" int fastp_gpu_submit_pass2_device(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, const void* scan_state,
                                             fastp_gpu_results* res, void* hip_stream) {
    if (!ctx) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    if (!ctx->dp.dup_enabled) return FASTP_GPU_OK;  // pass 1 did everything
    if (!scan_state || ((uintptr_t)scan_state & 7u)) return fail(ctx, FASTP_GPU_E_INVALID, "scan state must be an 8-byte aligned device buffer");
    return submit_chunks(ctx, b, res, hip_stream, CHUNK_PASS2, (u8*)scan_state);
}

extern "C" int fastp_gpu_overrep_device(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, const fastp_gpu_results* res,
                                        void* hip_stream) {
    return submit_chunks(ctx, b, res, hip_stream, CHUNK_OVERREP, nullptr);
}

extern "C" int64_t fastp_gpu_dup_bitmap_bytes(const fastp_gpu_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->dp.dup_enabled ? (int64_t)ctx->dp.dup_bufnum * (int64_t)(ctx->dp.dup_bits / 8) : 0;
}

extern "C" int fastp_gpu_dup_bitmap_export(fastp_gpu_ctx* ctx, void* dst_device) {
    if (!ctx) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    const int64_t bytes = fastp_gpu_dup_bitmap_bytes(ctx);
    if (bytes == 0) return FASTP_GPU_OK;
    if (!dst_device) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst_device, ctx->d_bitmap, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

// the counterpart of the export: this engine's bitmaps <- an image (a context that takes over another's stream,
// fastp_gpu_stream.h's re-plan; Duplicate's state is nothing but these bits, duplicate.h:34-37)
extern "C" int fastp_gpu_dup_bitmap_import(fastp_gpu_ctx* ctx, const void* src_device) {
    if (!ctx) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    const int64_t bytes = fastp_gpu_dup_bitmap_bytes(ctx);
    if (bytes == 0) return FASTP_GPU_OK;
    if (!src_device) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bitmap, src_device, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_dup_prefix_set(fastp_gpu_ctx* ctx, const void* images_device, int32_t n_images) {
    if (!ctx || n_images < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    const int64_t bytes = fastp_gpu_dup_bitmap_bytes(ctx);
    if (bytes == 0 || n_images == 0) {
        ctx->has_prefix = false;
        return FASTP_GPU_OK;
    }
    if (!images_device || ((uintptr_t)images_device & 15u)) return fail(ctx, FASTP_GPU_E_INVALID, "bitmap images must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_prefix) {
        if (hipMalloc((void**)&ctx->d_prefix, (size_t)bytes) != hipSuccess) return fail(ctx, FASTP_GPU_E_NOMEM, "hipMalloc(prefix bitmaps) failed");
    }
    OrArgs o;
    o.images = (u32x4*)images_device;
    o.dst = (u32x4*)ctx->d_prefix;
    o.chunks = (u64)bytes / 16;
    o.n_images = n_images;
    hipLaunchKernelGGL(fq_or_images_kernel, dim3(ctx->cus * 8), dim3(256), 0, ctx->stream, o);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->has_prefix = true;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_prefix_or_images(fastp_gpu_ctx* ctx, void* images_device, int32_t n_images, int64_t bytes_each) {
    if (!ctx || n_images < 0 || bytes_each < 0 || (bytes_each & 15)) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (n_images == 0 || bytes_each == 0) return FASTP_GPU_OK;
    if (!images_device || ((uintptr_t)images_device & 15u)) return fail(ctx, FASTP_GPU_E_INVALID, "images must be 16-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    OrArgs o;
    o.images = (u32x4*)images_device;
    o.dst = nullptr;
    o.chunks = (u64)bytes_each / 16;
    o.n_images = n_images;
    hipLaunchKernelGGL(fq_or_images_kernel, dim3(ctx->cus * 8), dim3(256), 0, ctx->stream, o);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_host_writes_overlapped(fastp_gpu_ctx* ctx, int on) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    ctx->host_overlapped = on != 0;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_format_interleaved(fastp_gpu_ctx* ctx, int on) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    if (!ctx->dp.paired) return fail(ctx, FASTP_GPU_E_INVALID, "interleaved output (--stdout) needs paired input: out1 is the stream of a single-end run");
    if (ctx->dp.merge) return fail(ctx, FASTP_GPU_E_INVALID, "interleaved output (--stdout) in merge mode: the merged stream goes to standard output");
    ctx->fmt_interleaved = on != 0;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_format_pack_cuts(fastp_gpu_ctx* ctx, const fastp_gpu_pack_cuts* plan) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    ctx->cuts_armed = false;
    if (!plan) return FASTP_GPU_OK;
    if (plan->first_unit < 0 || plan->pack_size < 1 || plan->max_packs < 1 || !plan->cut || !plan->passed)
        return fail(ctx, FASTP_GPU_E_INVALID, "pack cuts: first_unit >= 0, pack_size >= 1, max_packs >= 1 and both device arrays are needed");
    ctx->cuts = *plan;
    ctx->cuts_armed = true;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_phred64_to_33(fastp_gpu_ctx* ctx, int32_t n, uint8_t* text, const uint32_t* line_off, const uint32_t* line_len, uint8_t* qual_rows) {
    if (!ctx || n < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (n == 0) return FASTP_GPU_OK;
    if (!text || !line_off || !line_len || !qual_rows) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Phred64Args a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.qs = (int)fastp_gpu_qual_stride(ctx->dp.max_len);
    a.text = text;
    a.line_off = line_off;
    a.line_len = line_len;
    a.qual = qual_rows;
    hipLaunchKernelGGL(fq_phred64_kernel, dim3(std::min((n + 3) / 4, ctx->cus * 32)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_stream_set_origin(fastp_gpu_ctx* ctx, int64_t units_before, int64_t post_reads_before) {
    if (!ctx || units_before < 0 || post_reads_before < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->units_seen = (uint64_t)units_before;
    const u64 v = (u64)post_reads_before;
    if (!ctx->d_post_seen) return FASTP_GPU_OK;  // no overrepresentation analysis: nothing else reads positions
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_post_seen, &v, sizeof(v), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_parse_fastq(fastp_gpu_ctx* ctx, const uint8_t* text, int64_t nbytes, int is_last_chunk,
                                     int32_t max_records, uint8_t* seq_out, uint8_t* qual_out, uint16_t* len_out,
                                     uint32_t* line_off, uint32_t* line_len, fastp_gpu_parse_info* info) {
    if (!ctx || !info || nbytes < 0 || max_records < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    memset(info, 0, sizeof(*info));
    info->first_bad = -1;
    ctx->parse_exotic.clear();  // also when nothing is parsed: fastp_gpu_parse_exotic answers for THIS call
    if (nbytes == 0 || max_records == 0) return FASTP_GPU_OK;
    if (!text || !seq_out || !qual_out || !len_out || !line_off || !line_len) return fail(ctx, FASTP_GPU_E_INVALID, "null buffer");
    if (((uintptr_t)text & 15u) != 0) return fail(ctx, FASTP_GPU_E_INVALID, "text must be 16-byte aligned (and padded to 16 bytes)");
    if (nbytes >= (1ll << 32)) return fail(ctx, FASTP_GPU_E_INVALID, "chunk of 4 GiB or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ParseArgs p;
    memset(&p, 0, sizeof(p));
    p.text = text;
    p.nbytes = (u32)nbytes;
    p.is_last = is_last_chunk ? 1 : 0;
    p.max_lines = 4u * (u32)max_records + 1u;
    p.max_len = ctx->dp.max_len;
    p.sw_g = ctx->dp.sw_g;
    p.qw_g = ctx->dp.qw_g;
    p.max_records = max_records;
    p.seq_out = (u32*)seq_out;
    p.qual_out = (u32*)qual_out;
    p.len_out = len_out;
    p.line_off = line_off;
    p.line_len = line_len;
    const int per_block = PARSE_BLOCK * PARSE_BYTES_PER_LANE * PARSE_SUB;
    const int nblocks = (int)((nbytes + per_block - 1) / per_block);
    const size_t dwords = 8 + (size_t)2 * nblocks + p.max_lines + (p.max_lines + 3) / 4 + 4 + (size_t)max_records;
    int rc = ensure(ctx, (void**)&ctx->d_parse, &ctx->parse_cap, dwords * 4);
    if (rc) return rc;
    p.totals = ctx->d_parse;
    p.blockcount = ctx->d_parse + 8;
    p.blockbase = p.blockcount + nblocks;
    p.term_pos = p.blockbase + nblocks;
    p.term_len = (u8*)(p.term_pos + p.max_lines);
    p.exotic_list = p.term_pos + p.max_lines + (p.max_lines + 3) / 4 + 1;
    p.exotic_cap = (u32)max_records;
    const u32 init[8] = {0, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(p.totals, init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fq_parse_count_kernel, dim3(nblocks), dim3(PARSE_BLOCK), 16, st, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_parse_scan_kernel, dim3(1), dim3(1024), 1024 * 4, st, p, nblocks);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_parse_index_kernel, dim3(nblocks), dim3(PARSE_BLOCK), 64, st, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_parse_finish_kernel, dim3(1), dim3(64), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    u32 totals[8];
    // the record count comes back before the packer is launched: its grid then covers the records that exist, not the
    // caller's capacity (a 16 MiB chunk of 150-base reads holds 50 K records of the 512 K it may hold)
    HIP_TRY(ctx, hipMemcpyAsync(totals, p.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const u32 nrec = totals[3];
    if (nrec > 0) {
        hipLaunchKernelGGL(fq_parse_pack_kernel, dim3((nrec + 15) / 16), dim3(256), 0, st, p);  // 4 records per wavefront
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, p.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    info->n_records = (int32_t)totals[3];
    info->consumed = (int64_t)totals[4];
    info->n_lines = (int64_t)totals[2];
    info->first_bad = totals[1] == 0xFFFFFFFFu ? -1 : (int32_t)(totals[1] >> 2);
    info->bad_kind = totals[1] == 0xFFFFFFFFu ? 0 : (int32_t)(totals[1] & 3u);
    info->max_seq_len = (int32_t)totals[5];
    if (totals[6] > 0 && nrec > 0) {   // records with letters outside ACGTN: their indexes, ascending (fastp_gpu_parse_exotic)
        const u32 cnt = std::min(totals[6], p.exotic_cap);
        ctx->parse_exotic.resize(cnt);
        HIP_TRY(ctx, hipMemcpy(ctx->parse_exotic.data(), p.exotic_list, (size_t)cnt * 4, hipMemcpyDeviceToHost));
        std::sort(ctx->parse_exotic.begin(), ctx->parse_exotic.end());
    }
    info->n_exotic = (int32_t)ctx->parse_exotic.size();
    if (info->first_bad >= 0)
        return fail(ctx, FASTP_GPU_E_INVALID,
                    info->bad_kind == FASTP_GPU_PARSE_BAD_TOO_LONG ? "a read of the chunk is longer than the context's max_len (see first_bad, max_seq_len)"
                    : info->bad_kind == FASTP_GPU_PARSE_BAD_ALPHABET ? "a record of the chunk has a quality character outside '!'..'~' (see first_bad)"
                                                                     : "malformed FASTQ record in the chunk (see first_bad)");
    return FASTP_GPU_OK;
}

extern "C" int32_t fastp_gpu_parse_exotic(const fastp_gpu_ctx* ctx, int32_t* units, int32_t capacity) {
    if (!ctx) return 0;
    const int32_t n = (int32_t)ctx->parse_exotic.size();
    for (int32_t k = 0; units && k < n && k < capacity; k++) units[k] = ctx->parse_exotic[k];
    return n;
}

// BgzfMtReader::readerLoop's header walk (src/bgzf.h:29-32, 150-200): gzip member header with the BC extra
// subfield, BSIZE = member size - 1; deflate payload; CRC32; ISIZE
extern "C" int fastp_gpu_bgzf_index(const uint8_t* h, int64_t nbytes, int32_t max_blocks, int64_t max_text_bytes,
                                    uint32_t* pay_off, uint32_t* pay_len, uint32_t* isize, uint32_t* crc, uint64_t* out_off,
                                    fastp_gpu_inflate_info* info) {
    if (!info) return FASTP_GPU_E_INVALID;
    info->n_blocks = 0;
    info->first_bad = -1;
    info->consumed = 0;
    info->out_bytes = 0;
    if (!h || nbytes < 0 || max_blocks < 0 || !pay_off || !pay_len || !isize || !crc || !out_off) return FASTP_GPU_E_INVALID;
    int64_t pos = 0, text = 0;
    int32_t k = 0;
    while (k < max_blocks && pos + 18 <= nbytes) {
        const uint8_t* p = h + pos;
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) { info->first_bad = k; break; }
        const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
        if (pos + 12 + xlen > nbytes) break;  // header not complete yet
        // find the BC subfield among the extra subfields (bgzip writes it first; others may precede it)
        int64_t bsize = -1;
        for (uint32_t o = 0; o + 4 <= xlen;) {
            const uint8_t* e = p + 12 + o;
            const uint32_t slen = (uint32_t)e[2] | ((uint32_t)e[3] << 8);
            if (e[0] == 'B' && e[1] == 'C' && slen == 2 && o + 6 <= xlen) { bsize = ((int64_t)e[4] | ((int64_t)e[5] << 8)) + 1; break; }
            o += 4 + slen;
        }
        if (bsize < 0 || (p[3] & ~4)) { info->first_bad = k; break; }  // not BGZF (or name/comment/hcrc fields: bgzip never writes them)
        const int64_t hdr = 12 + (int64_t)xlen;
        if (bsize < hdr + 8) { info->first_bad = k; break; }
        if (pos + bsize > nbytes) break;  // member not complete yet
        if (pos + bsize > 0xFFFFFFFFll) break;  // payload offsets are 32 bit: the caller indexes the rest from `consumed`
        const uint8_t* t = p + bsize - 8;
        const uint32_t c = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t n = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (n > 65536u) { info->first_bad = k; break; }
        if (text + n > max_text_bytes) break;
        pay_off[k] = (uint32_t)(pos + hdr);
        pay_len[k] = (uint32_t)(bsize - hdr - 8);
        isize[k] = n;
        crc[k] = c;
        out_off[k] = (uint64_t)text;
        text += n;
        pos += bsize;
        k++;
    }
    info->n_blocks = k;
    info->consumed = pos;
    info->out_bytes = text;
    return info->first_bad >= 0 ? FASTP_GPU_E_INVALID : FASTP_GPU_OK;
}

extern "C" int fastp_gpu_inflate_bgzf(fastp_gpu_ctx* ctx, const uint8_t* comp, int32_t n_blocks, const uint32_t* pay_off,
                                      const uint32_t* pay_len, const uint32_t* isize, const uint32_t* crc, const uint64_t* out_off,
                                      uint8_t* out, int64_t out_capacity, int check_crc, int32_t* first_bad) {
    if (first_bad) *first_bad = -1;
    if (!ctx || n_blocks < 0 || out_capacity < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (n_blocks == 0) return FASTP_GPU_OK;
    if (!comp || !pay_off || !pay_len || !isize || !crc || !out_off || !out) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t scratch = (size_t)n_blocks * INF_SCRATCH, status = (size_t)n_blocks * 4;
    int rc = ensure(ctx, (void**)&ctx->d_inf, &ctx->inf_cap, scratch + status + 16);
    if (rc) return rc;
    InflateArgs a;
    memset(&a, 0, sizeof(a));
    a.comp = comp;
    a.pay_off = pay_off; a.pay_len = pay_len; a.isize = isize; a.crc = crc; a.out_off = out_off;
    a.n = n_blocks;
    a.out = out;
    a.out_cap = (u64)out_capacity;
    a.scratch = ctx->d_inf;
    a.status = (u32*)(ctx->d_inf + scratch);
    a.first_bad = (u32*)(ctx->d_inf + scratch + status);
    a.check_crc = check_crc;
    HIP_TRY(ctx, hipMemsetAsync(a.first_bad, 0xFF, 4, st));
    // one wavefront per block (fq_inflate_wave.h: 4.6 ms per launch whatever the size, 2 blocks per CU in flight) up to
    // 6144 blocks; beyond that blocks in flight decide and one lane per block (fq_inflate.h: ~50 ms per launch, 64 blocks
    // per wavefront) overtakes it (profiles/r02l_inflate.txt).  FASTP_GPU_INFLATE=lane|wave forces one.
    const int how = ctx->sw.inflate;   // 0: by size, 1: lane, 2: wave
    const bool wave_fits = (int)sizeof(IwLds) <= ctx->lds_bytes;
    if (how == 2 && !wave_fits) return fail(ctx, FASTP_GPU_E_INVALID, "FASTP_GPU_INFLATE=wave: the wave kernel's LDS does not fit this device");
    const bool lane_kernel = how ? how == 1 || !wave_fits : n_blocks > 6144 || !wave_fits;
    if (lane_kernel) {
        hipLaunchKernelGGL(fq_inflate_kernel, dim3((n_blocks + INF_LANES - 1) / INF_LANES), dim3(INF_LANES), inflate_lane_lds_bytes(), st, a);
    } else {
        const int per_cu = std::max(1, ctx->lds_bytes / (int)sizeof(IwLds));
        hipLaunchKernelGGL(fq_inflate_wave_kernel, dim3(std::min(n_blocks, ctx->cus * per_cu)), dim3(64), sizeof(IwLds), st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    u32 bad = 0xFFFFFFFFu;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, a.first_bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (bad != 0xFFFFFFFFu) {
        if (first_bad) *first_bad = (int32_t)bad;
        return fail(ctx, FASTP_GPU_E_INVALID, "a BGZF block failed to inflate (see first_bad)");
    }
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_format_fastq(fastp_gpu_ctx* ctx, int32_t n, const fastp_gpu_format_in* m1, const fastp_gpu_format_in* m2,
                                      const fastp_gpu_correction* corrections, const int32_t* n_corrections, uint8_t* out1,
                                      int64_t out1_capacity, uint8_t* out2, int64_t out2_capacity, int64_t out_len[2]) {
    if (!ctx || !m1 || !out_len || n < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    out_len[0] = out_len[1] = 0;
    const bool paired = ctx->dp.paired != 0;
    if (paired != (m2 != nullptr)) return fail(ctx, FASTP_GPU_E_INVALID, "mate 2 must be given exactly for a paired engine");
    if (ctx->dp.merge) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "merge mode writes the merged stream on the host");
    if (ctx->dp.umi_len1 || ctx->dp.umi_len2) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "UMI name edits are host logic");
    if (n == 0) return FASTP_GPU_OK;
    if (!out1 || (paired && !out2) || out1_capacity < 0 || out2_capacity < 0) return fail(ctx, FASTP_GPU_E_INVALID, "null output buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FmtArgs f;
    memset(&f, 0, sizeof(f));
    f.n = n;
    f.paired = paired ? 1 : 0;
    f.dedup = ctx->dp.dedup;
    f.nblocks = (n + FMT_BLOCK - 1) / FMT_BLOCK;
    const size_t words = (size_t)4 * f.nblocks + 2 + (size_t)2 * n;
    int rc = ensure(ctx, (void**)&ctx->d_fmt, &ctx->fmt_cap, words * 8);
    if (rc) return rc;
    f.blocksum = ctx->d_fmt;
    f.blockbase = f.blocksum + (size_t)2 * f.nblocks;
    f.totals = f.blockbase + (size_t)2 * f.nblocks;
    const fastp_gpu_format_in* ins[2] = {m1, m2};
    uint8_t* outs[2] = {out1, out2};
    const int64_t caps[2] = {out1_capacity, out2_capacity};
    for (int m = 0; m < (paired ? 2 : 1); m++) {
        if (!ins[m]->text || !ins[m]->line_off || !ins[m]->line_len || !ins[m]->res) return fail(ctx, FASTP_GPU_E_INVALID, "null input");
        f.m[m].text = ins[m]->text;
        f.m[m].line_off = ins[m]->line_off;
        f.m[m].line_len = ins[m]->line_len;
        f.m[m].res = (const u32*)ins[m]->res;
        f.m[m].out = outs[m];
        f.m[m].out_cap = (u64)caps[m];
        f.m[m].unit_off = f.totals + 2 + (size_t)m * n;
    }
    f.corrections = (const u32*)corrections;
    f.n_corrections = n_corrections;
    HIP_TRY(ctx, hipMemsetAsync(f.totals, 0, 16, st));
    hipLaunchKernelGGL(fq_fmt_len_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), 16, st, f);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_fmt_scan_kernel, dim3(paired ? 2 : 1), dim3(1024), 1024 * 8, st, f);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_fmt_write_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), 128, st, f);
    HIP_TRY(ctx, hipGetLastError());
    int32_t ncorr = 0;
    if (corrections && n_corrections) HIP_TRY(ctx, hipMemcpyAsync(&ncorr, n_corrections, 4, hipMemcpyDeviceToHost, st));
    u64 totals[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(totals, f.totals, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ncorr > 0) {
        hipLaunchKernelGGL(fq_fmt_fix_kernel, dim3((ncorr + 255) / 256), dim3(256), 0, st, f);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    out_len[0] = (int64_t)totals[0];
    out_len[1] = (int64_t)totals[1];
    if (out_len[0] > out1_capacity || (paired && out_len[1] > out2_capacity))
        return fail(ctx, FASTP_GPU_E_OVERFLOW, "output buffer too small (see out_len for the needed sizes)");
    return FASTP_GPU_OK;
}

// fastp_gpu_format_streams (ns = 6: the (6, 2) kernels) and fastp_gpu_format_all_streams (ns = 7: the (7, 3) kernels); out,
// out_capacity and out_len hold ns entries
static int format_streams_impl(fastp_gpu_ctx* ctx, const int ns, int32_t n, const fastp_gpu_format_io* m1, const fastp_gpu_format_io* m2,
                               const fastp_gpu_pair_result* pair, const fastp_gpu_correction* corrections, const int32_t* n_corrections,
                               const fastp_gpu_format_options* opts, uint8_t* const* out, const int64_t* out_capacity, int64_t* out_len) {
    if (!ctx || !m1 || !out || !out_capacity || !out_len || n < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    for (int q = 0; q < ns; q++) out_len[q] = 0;
    // fastp_gpu_format_pack_cuts arms one call: this one
    const bool cuts_on = ctx->cuts_armed;
    const fastp_gpu_pack_cuts cuts = ctx->cuts;
    ctx->cuts_armed = false;
    u32 slices = 0;
    if (cuts_on) {
        if (n > 0) slices = (u32)((cuts.first_unit + n - 1) / cuts.pack_size - cuts.first_unit / cuts.pack_size + 1);
        if (slices > (u32)cuts.max_packs) return fail(ctx, FASTP_GPU_E_INVALID, "pack cuts: the call's units span more packs than max_packs");
    }
    const bool paired = ctx->dp.paired != 0;
    if (paired != (m2 != nullptr)) return fail(ctx, FASTP_GPU_E_INVALID, "mate 2 must be given exactly for a paired engine");
    if (paired && !pair) return fail(ctx, FASTP_GPU_E_INVALID, "a paired engine needs the pair records");
    const bool all = ns == FMTS_ALL_STREAMS;
    if (!all && ctx->dp.overlapped_out && !ctx->host_overlapped)
        return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "--overlapped_out's stream is written by the host (fastp_gpu_host.h, or fastp_gpu_host_writes_overlapped)");
    FmtsArgs f;
    memset(&f, 0, sizeof(f));
    f.n = n;
    f.overlapped_out = (all && paired && ctx->dp.overlapped_out) ? 1 : 0;
    f.paired = paired ? 1 : 0;
    f.dedup = ctx->dp.dedup;
    f.merge = paired ? ctx->dp.merge : 0;
    f.merge_include_unmerged = ctx->dp.merge_include_unmerged;
    f.delim[0] = ':';
    f.delim_len = 1;
    if (opts) {
        f.want_failed = opts->want_failed != 0;
        f.want_u1 = opts->want_unpaired1 != 0;
        f.want_u2 = opts->want_unpaired2 != 0;
        const int loc = opts->umi_loc & 0xFF;
        if (opts->umi_loc < 0 || (opts->umi_loc & ~(0xFF | FASTP_GPU_NAME_FIX_MGI)) || loc > FASTP_GPU_UMI_PER_INDEX)
            return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "unknown UMI location or name option in umi_loc");
        f.umi_loc = loc;
        f.fix_mgi = (opts->umi_loc & FASTP_GPU_NAME_FIX_MGI) ? 1 : 0;
        f.name_scan = (f.fix_mgi || loc >= FASTP_GPU_UMI_INDEX1) ? 1 : 0;
        f.umi_len = opts->umi_len;
        if (opts->umi_delimiter) {
            const size_t dl = strlen(opts->umi_delimiter);
            if (dl > sizeof(f.delim)) return fail(ctx, FASTP_GPU_E_INVALID, "UMI delimiter longer than 8 characters");
            memcpy(f.delim, opts->umi_delimiter, dl);
            f.delim_len = (u32)dl;
        }
        if (opts->umi_prefix) {
            const size_t pl = strlen(opts->umi_prefix);
            if (pl > sizeof(f.prefix)) return fail(ctx, FASTP_GPU_E_INVALID, "UMI prefix longer than 32 characters");
            memcpy(f.prefix, opts->umi_prefix, pl);
            f.prefix_len = (u32)pl;
        }
    }
    f.interleaved = (paired && !f.merge && ctx->fmt_interleaved) ? 1 : 0;
    if (n == 0) {
        if (cuts_on) {   // the closing entry alone
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            for (int q = 0; q < 2; q++) HIP_TRY(ctx, hipMemsetAsync(cuts.cut + (size_t)q * (cuts.max_packs + 1), 0, 8, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return FASTP_GPU_OK;
    }
    // the streams this configuration can write to need a buffer
    const bool need[FMTS_ALL_STREAMS] = {true, paired && !f.interleaved, f.want_failed != 0, f.merge != 0, paired && f.want_u1, paired && f.want_u2, f.overlapped_out != 0};
    for (int q = 0; q < ns; q++) {
        if (out_capacity[q] < 0 || (need[q] && !out[q])) return fail(ctx, FASTP_GPU_E_INVALID, "null output buffer for a stream the options ask for");
        f.out[q] = out[q];
        f.out_cap[q] = out[q] ? (u64)out_capacity[q] : 0;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    f.nblocks = (n + FMT_BLOCK - 1) / FMT_BLOCK;
    const size_t words = (size_t)2 * ns * f.nblocks + ns;
    int rc = ensure(ctx, (void**)&ctx->d_fmt, &ctx->fmt_cap, words * 8);
    if (rc) return rc;
    f.blocksum = ctx->d_fmt;
    f.blockbase = f.blocksum + (size_t)ns * f.nblocks;
    f.totals = f.blockbase + (size_t)ns * f.nblocks;
    const fastp_gpu_format_io* ins[2] = {m1, m2};
    for (int m = 0; m < (paired ? 2 : 1); m++) {
        if (!ins[m]->text || !ins[m]->line_off || !ins[m]->line_len || !ins[m]->res) return fail(ctx, FASTP_GPU_E_INVALID, "null input");
        f.m[m].text = ins[m]->text;
        f.m[m].line_off = ins[m]->line_off;
        f.m[m].line_len = ins[m]->line_len;
        f.m[m].res = (const u32*)ins[m]->res;
    }
    f.pair = (const u32*)pair;
    f.corrections = (const u32*)corrections;
    f.n_corrections = n_corrections;
    if (cuts_on) {   // (a single-end call never touches stream 1's offsets: they are zero)
        f.cut[0] = cuts.cut;
        f.cut[1] = cuts.cut + (size_t)cuts.max_packs + 1;
        f.passed = cuts.passed;
        f.first_unit = (u64)cuts.first_unit;
        f.pack_size = (u32)cuts.pack_size;
        HIP_TRY(ctx, hipMemsetAsync(f.passed, 0, (size_t)slices * 4, st));
    }
    int32_t ncorr = 0;
    if (corrections && n_corrections) {
        HIP_TRY(ctx, hipMemcpyAsync(&ncorr, n_corrections, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        // the engine's counter keeps counting past the list's capacity: such a list is incomplete and reading
        // n_corrections entries would run behind the buffer
        int32_t cap = (opts && opts->corrections_capacity > 0) ? opts->corrections_capacity
                                                                : (corrections == ctx->last_corr ? ctx->last_corr_cap : 0);
        if (cap > 0 && ncorr > cap) return fail(ctx, FASTP_GPU_E_OVERFLOW, "correction list capacity exceeded: the list is incomplete");
        if (ncorr > 0) {
            hipLaunchKernelGGL(fq_fmts_corr_kernel, dim3((ncorr + 255) / 256), dim3(256), 0, st, f);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    // LDS: a block sum per stream; then wave sums per stream + a u64 offset per (unit, emission slot)
    if (all) hipLaunchKernelGGL(fq_fmts7_len_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), FMTS_ALL_STREAMS * 4, st, f);
    else hipLaunchKernelGGL(fq_fmts_len_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), FMTS_STREAMS * 4, st, f);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_fmts_scan_kernel, dim3(ns), dim3(1024), 1024 * 8, st, f);
    HIP_TRY(ctx, hipGetLastError());
    if (all) hipLaunchKernelGGL(fq_fmts7_write_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), FMTS_ALL_STREAMS * 16 * 4 + FMT_BLOCK * 3 * 8, st, f);
    else hipLaunchKernelGGL(fq_fmts_write_kernel, dim3(f.nblocks), dim3(FMT_BLOCK), FMTS_STREAMS * 16 * 4 + FMT_BLOCK * 16, st, f);
    HIP_TRY(ctx, hipGetLastError());
    u64 totals[FMTS_ALL_STREAMS];
    HIP_TRY(ctx, hipMemcpyAsync(totals, f.totals, (size_t)ns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    bool overflow = false;
    for (int q = 0; q < ns; q++) {
        out_len[q] = (int64_t)totals[q];
        if (totals[q] > f.out_cap[q]) overflow = true;
    }
    if (overflow) return fail(ctx, FASTP_GPU_E_OVERFLOW, "output buffer too small (see out_len for the needed sizes)");
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_format_streams(fastp_gpu_ctx* ctx, int32_t n, const fastp_gpu_format_io* m1, const fastp_gpu_format_io* m2,
                                        const fastp_gpu_pair_result* pair, const fastp_gpu_correction* corrections,
                                        const int32_t* n_corrections, const fastp_gpu_format_options* opts,
                                        uint8_t* const out[FASTP_GPU_N_OUTPUTS], const int64_t out_capacity[FASTP_GPU_N_OUTPUTS],
                                        int64_t out_len[FASTP_GPU_N_OUTPUTS]) {
    return format_streams_impl(ctx, FMTS_STREAMS, n, m1, m2, pair, corrections, n_corrections, opts, out, out_capacity, out_len);
}

extern "C" int fastp_gpu_format_all_streams(fastp_gpu_ctx* ctx, int32_t n, const fastp_gpu_format_io* m1, const fastp_gpu_format_io* m2,
                                            const fastp_gpu_pair_result* pair, const fastp_gpu_correction* corrections,
                                            const int32_t* n_corrections, const fastp_gpu_format_options* opts,
                                            uint8_t* const out[FASTP_GPU_N_HOST_OUTPUTS], const int64_t out_capacity[FASTP_GPU_N_HOST_OUTPUTS],
                                            int64_t out_len[FASTP_GPU_N_HOST_OUTPUTS]) {
    return format_streams_impl(ctx, FMTS_ALL_STREAMS, n, m1, m2, pair, corrections, n_corrections, opts, out, out_capacity, out_len);
}

// ---- adapter census (fq_census.h) -----------------------------------------------------------------------------------------
// One persistent table per map in one allocation: ehash | ecount | index | eoff | elen | ctl | arena (a key is at most
// FASTP_GPU_MAX_READ_LEN bytes: a piece of a sequence line or of an adapter sequence).
static const size_t CS_KEY_MAX = FASTP_GPU_MAX_READ_LEN;
static u64 cs_hash_mask(const fastp_gpu_ctx* ctx) {
    const int k = ctx->sw.census_hash_bits;
    return (k <= 0 || k >= 64) ? ~(u64)0 : (((u64)1 << k) - 1);
}
static u64 cs_host_hash(const u8* p, u32 len, u64 mask) {
    u64 sum = 0;
    for (u32 k = 0; k < len; k++) sum += cs_term(k, p[k], 0);
    return cs_finish(sum, len, 0, mask);
}
static size_t cs_map_header_bytes() {
    return (size_t)CS_MAX_ENTRIES * 16 + (size_t)CS_INDEX_SLOTS * 4 + (size_t)CS_MAX_ENTRIES * 8 + 16;
}
static int cs_ensure_maps(fastp_gpu_ctx* ctx) {
    if (ctx->d_cs_map[0]) return 0;
    const size_t E = CS_MAX_ENTRIES, head = cs_map_header_bytes(), arena = E * CS_KEY_MAX;
    for (int w = 0; w < 2; w++) {
        HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cs_map[w], head + arena));
        u8* b = ctx->d_cs_map[w];
        CsMap& m = ctx->cs_map[w];
        m.ehash = (u64*)b;
        m.ecount = m.ehash + E;
        m.index = (u32*)(m.ecount + E);
        m.eoff = m.index + CS_INDEX_SLOTS;
        m.elen = m.eoff + E;
        m.ctl = m.elen + E;
        m.arena = (u8*)(m.ctl + 4);
        m.arena_cap = (u32)arena;
        HIP_TRY(ctx, hipMemsetAsync(b, 0, head, ctx->stream));
        ctx->cs_entries[w] = 0;
    }
    // the adapter sequences a string with adapter_pos < 0 is cut from: -a, --adapter_sequence_r2, the --adapter_fasta entries
    std::vector<const std::string*> seqs = {&ctx->adapter1, &ctx->adapter2};
    for (auto& f : ctx->fasta_strings) seqs.push_back(&f);
    std::vector<u32> off(seqs.size()), len(seqs.size());
    std::string bytes;
    for (size_t k = 0; k < seqs.size(); k++) {
        off[k] = (u32)bytes.size();
        len[k] = (u32)seqs[k]->size();
        bytes += *seqs[k];
    }
    const size_t tab = seqs.size() * 4, total = 2 * tab + bytes.size() + 8;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_cs_blob, total));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cs_blob, off.data(), tab, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cs_blob + tab, len.data(), tab, hipMemcpyHostToDevice, ctx->stream));
    if (!bytes.empty()) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cs_blob + 2 * tab, bytes.data(), bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the host vectors go out of scope)
    return 0;
}
static int cs_clear_map(fastp_gpu_ctx* ctx, int w) {
    if (ctx->d_cs_map[w]) HIP_TRY(ctx, hipMemsetAsync(ctx->d_cs_map[w], 0, cs_map_header_bytes(), ctx->stream));
    ctx->cs_entries[w] = 0;
    return 0;
}
static int cs_read_words(fastp_gpu_ctx* ctx, const u32* dev, u32* host, int n) {
    HIP_TRY(ctx, hipMemcpyAsync(host, dev, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
#define CS_LAUNCH(kernel, threads, args)                                                                               \
    do {                                                                                                               \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(((size_t)(threads) + CS_BLOCK - 1) / CS_BLOCK)), dim3(CS_BLOCK), 0, ctx->stream, args); \
        HIP_TRY(ctx, hipGetLastError());                                                                               \
    } while (0)

// the K-th smallest (K >= 1) first occurrence among the dedupe slots with key >= lo [whose string is not low complexity]:
// one 8-bit digit per pass from the top.  *total = how many such slots there are; fewer than K: *key is not set.
static int cs_select(fastp_gpu_ctx* ctx, CsArgs a, u64 K, u64 lo, int nonlc, u64* total, u64* key) {
    u64 prefix = 0;
    u32 hist[256];
    a.sel_lo = lo;
    a.sel_nonlc = nonlc;
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)a.n_slots + 255) / 256, 1024);
    for (int shift = 56; shift >= 0; shift -= 8) {
        a.sel_shift = shift;
        a.sel_top = shift == 56;
        a.sel_prefix = prefix;
        HIP_TRY(ctx, hipMemsetAsync(a.hist, 0, sizeof(hist), ctx->stream));
        hipLaunchKernelGGL(fq_census_hist_kernel, dim3(grid), dim3(256), 256 * 4, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
        int rc = cs_read_words(ctx, a.hist, hist, 256);
        if (rc) return rc;
        if (shift == 56) {
            u64 t = 0;
            for (u32 v : hist) t += v;
            *total = t;
            if (t < K) return 0;
        }
        u64 run = 0;
        int d = 0;
        for (; d < 256; d++) {
            if (run + hist[d] >= K) break;
            run += hist[d];
        }
        if (d == 256) return fail(ctx, FASTP_GPU_E_HIP, "adapter census: the select lost its key");
        K -= run;
        prefix = (prefix << 8) | (u64)d;
    }
    *key = prefix;
    return 0;
}

// phases 2 - 4 for one map: look-up, candidate dedupe, admission
static int cs_run_map(fastp_gpu_ctx* ctx, CsArgs& a, int w) {
    a.which = w;
    a.map = ctx->cs_map[w];
    a.salt = 0;
    u32 ctl[CS_CTL_WORDS];
    HIP_TRY(ctx, hipMemsetAsync(a.ctl + CS_CTL_CAND, 0, 3 * 4, ctx->stream));   // candidates, unresolved, slots
    CS_LAUNCH(fq_census_lookup_kernel, (size_t)a.n_items * CS_GROUP, a);
    int rc = cs_read_words(ctx, a.ctl, ctl, CS_CTL_WORDS);
    if (rc) return rc;
    const u32 ncand = ctl[CS_CTL_CAND];
    if (ncand == 0) return 0;
    // the dedupe table: a power of two of at least twice the candidates
    size_t ns = 64;
    while (ns < 2 * (size_t)ncand) ns <<= 1;
    rc = ensure(ctx, (void**)&ctx->d_cs_slots, &ctx->cs_slots_cap, ns * 28);
    if (rc) return rc;
    a.n_slots = (int)ns;
    a.s_word = (u64*)ctx->d_cs_slots;
    a.s_first = a.s_word + ns;
    a.s_item = (u32*)(a.s_first + ns);
    a.s_count = a.s_item + ns;
    a.s_verdict = a.s_count + ns;
    HIP_TRY(ctx, hipMemsetAsync(a.s_word, 0, ns * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.s_first, 0xFF, ns * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(a.s_item, 0, ns * 12, ctx->stream));
    // every round settles at least the string of each claimed slot's first item, so there are at most ncand rounds
    for (u32 round = 0;; round++) {
        if (round > ncand) return fail(ctx, FASTP_GPU_E_HIP, "adapter census: the candidate dedupe did not converge");
        HIP_TRY(ctx, hipMemsetAsync(a.ctl + CS_CTL_UNRESOLVED, 0, 4, ctx->stream));
        CS_LAUNCH(fq_census_insert_kernel, a.n_items, a);
        CS_LAUNCH(fq_census_first_kernel, a.n_items, a);
        CS_LAUNCH(fq_census_verify_kernel, (size_t)a.n_items * CS_GROUP, a);
        rc = cs_read_words(ctx, a.ctl, ctl, CS_CTL_WORDS);
        if (rc) return rc;
        if (ctl[CS_CTL_UNRESOLVED] == 0) break;
        a.salt = round + 1;   // two strings shared a hash: the ones that lost are hashed again, under another salt
        a.want_state = CS_CAND;
        CS_LAUNCH(fq_census_hash_kernel, (size_t)a.n_items * CS_GROUP, a);
    }
    // admission: everything while size <= 5000, then what is not low complexity while size <= 20000 - as two bounds on the
    // order key of the first occurrence (key < x1, or not low complexity and key < x2)
    const u64 D = ctl[CS_CTL_SLOTS], S0 = ctx->cs_entries[w], ALL = ~(u64)0;
    const u64 KA = S0 <= CS_LOW_COMPLEXITY_SKIP ? (u64)CS_LOW_COMPLEXITY_SKIP + 1 - S0 : 0;
    a.x1 = ALL;
    a.x2 = 0;
    if (KA < D) {
        a.x1 = 0;
        u64 total = 0, key = 0;
        if (KA > 0) {
            rc = cs_select(ctx, a, KA, 0, 0, &total, &key);
            if (rc) return rc;
            if (total < KA) return fail(ctx, FASTP_GPU_E_HIP, "adapter census: fewer dedupe slots than were claimed");
            a.x1 = key + 1;
        }
        const u64 s = S0 + KA, KB = s <= CS_MAX_ADAPTER_REC ? (u64)CS_MAX_ADAPTER_REC + 1 - s : 0;
        if (KB > 0) {
            rc = cs_select(ctx, a, KB, a.x1, 1, &total, &key);
            if (rc) return rc;
            a.x2 = total < KB ? ALL : key + 1;
        }
    }
    CS_LAUNCH(fq_census_admit_kernel, ns * CS_GROUP, a);
    u32 mctl[2];
    rc = cs_read_words(ctx, a.map.ctl, mctl, 2);
    if (rc) return rc;
    if (mctl[0] > CS_MAX_ENTRIES) return fail(ctx, FASTP_GPU_E_HIP, "adapter census: more keys admitted than the caps allow");
    ctx->cs_entries[w] = mctl[0];
    return 0;
}

extern "C" int fastp_gpu_adapter_census(fastp_gpu_ctx* ctx, int32_t n, const fastp_gpu_format_io* m1, const fastp_gpu_format_io* m2,
                                        const fastp_gpu_correction* corrections, const int32_t* n_corrections, int32_t corrections_capacity,
                                        const fastp_gpu_adapter_event* events, const int32_t* n_events, int32_t events_capacity) {
    if (!ctx || !m1 || n < 0 || corrections_capacity < 0 || events_capacity < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    const bool paired = ctx->dp.paired != 0;
    if (paired != (m2 != nullptr)) return fail(ctx, FASTP_GPU_E_INVALID, "mate 2 must be given exactly for a paired engine");
    if (n == 0) return FASTP_GPU_OK;
    const fastp_gpu_format_io* ins[2] = {m1, m2};
    for (int m = 0; m < (paired ? 2 : 1); m++)
        if (!ins[m]->text || !ins[m]->line_off || !ins[m]->line_len || !ins[m]->res) return fail(ctx, FASTP_GPU_E_INVALID, "null input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = cs_ensure_maps(ctx);
    if (rc) return rc;
    // the lists' counters keep counting past the capacity: such a list is incomplete, and nothing is read behind the buffer
    int32_t ncorr = 0, nev = 0;
    if (corrections && n_corrections) HIP_TRY(ctx, hipMemcpyAsync(&ncorr, n_corrections, 4, hipMemcpyDeviceToHost, st));
    if (events && n_events) HIP_TRY(ctx, hipMemcpyAsync(&nev, n_events, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (ncorr < 0 || nev < 0) return fail(ctx, FASTP_GPU_E_INVALID, "negative list counter");
    if (ncorr > corrections_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "correction list capacity exceeded: the list is incomplete");
    if (nev > events_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "adapter event list capacity exceeded: the list is incomplete");
    if (ncorr > 0) {   // the formatter's own patch kernel: the text is the same whether the formatter has run on it or not
        FmtsArgs f;
        memset(&f, 0, sizeof(f));
        f.n = n;
        f.paired = paired ? 1 : 0;
        for (int m = 0; m < (paired ? 2 : 1); m++) {
            f.m[m].text = ins[m]->text;
            f.m[m].line_off = ins[m]->line_off;
            f.m[m].line_len = ins[m]->line_len;
            f.m[m].res = (const u32*)ins[m]->res;
        }
        f.corrections = (const u32*)corrections;
        f.n_corrections = n_corrections;
        hipLaunchKernelGGL(fq_fmts_corr_kernel, dim3((ncorr + 255) / 256), dim3(256), 0, st, f);
        HIP_TRY(ctx, hipGetLastError());
    }
    const int nf = (int)ctx->fasta_strings.size();
    const size_t cap_items = (size_t)(paired ? 2 : 1) * (size_t)n + (size_t)nev;
    rc = ensure(ctx, (void**)&ctx->d_cs_items, &ctx->cs_items_cap, cap_items * sizeof(CsItem) + (CS_CTL_WORDS + 256) * 4);
    if (rc) return rc;
    CsArgs a;
    memset(&a, 0, sizeof(a));
    for (int m = 0; m < (paired ? 2 : 1); m++) {
        a.m[m].text = ins[m]->text;
        a.m[m].line_off = ins[m]->line_off;
        a.m[m].line_len = ins[m]->line_len;
        a.m[m].res = (const u32*)ins[m]->res;
    }
    a.events = (const u32*)events;
    a.blob_off = (const u32*)ctx->d_cs_blob;
    a.blob_len = a.blob_off + (2 + nf);
    a.blob = (const u8*)(a.blob_len + (2 + nf));
    a.items = (CsItem*)ctx->d_cs_items;
    a.ctl = (u32*)(ctx->d_cs_items + cap_items * sizeof(CsItem));
    a.hist = a.ctl + CS_CTL_WORDS;
    a.hash_mask = cs_hash_mask(ctx);
    a.n = n;
    a.paired = paired ? 1 : 0;
    a.n_events = nev;
    a.n_fasta = nf;
    a.max_str = (int)CS_KEY_MAX;
    a.map = ctx->cs_map[0];
    HIP_TRY(ctx, hipMemsetAsync(a.ctl, 0, CS_CTL_WORDS * 4, st));
    CS_LAUNCH(fq_census_gather_kernel, n, a);
    if (nev > 0) CS_LAUNCH(fq_census_events_kernel, nev, a);
    u32 ctl[CS_CTL_WORDS];
    rc = cs_read_words(ctx, a.ctl, ctl, CS_CTL_WORDS);
    if (rc) return rc;
    if (ctl[CS_CTL_TOO_LONG]) return fail(ctx, FASTP_GPU_E_TOO_LONG, "adapter census: a string longer than FASTP_GPU_MAX_READ_LEN");
    if (ctl[CS_CTL_ITEMS] > cap_items) return fail(ctx, FASTP_GPU_E_HIP, "adapter census: the item list overflowed");
    a.n_items = (int)ctl[CS_CTL_ITEMS];
    if (a.n_items == 0) return FASTP_GPU_OK;
    a.which = -1;   // both maps' items
    a.want_state = CS_NEW;
    CS_LAUNCH(fq_census_hash_kernel, (size_t)a.n_items * CS_GROUP, a);
    rc = cs_run_map(ctx, a, 0);
    if (rc) return rc;
    if (paired) {
        CS_LAUNCH(fq_census_pair_kernel, a.n_items, a);   // quirk #8: map 1's verdicts decide which read 2 strings count
        rc = cs_run_map(ctx, a, 1);
        if (rc) return rc;
    }
    return FASTP_GPU_OK;
}

// a map's entries on the host, in the reference's map order (classcomp, filterresult.h:14-23: length, then bytes)
struct CsHostMap {
    std::vector<u32> off, len;
    std::vector<u64> count;
    std::vector<u8> arena;
    std::vector<u32> order;
};
static int cs_download(fastp_gpu_ctx* ctx, int w, CsHostMap& h) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_cs_map[w]) return 0;
    const CsMap& m = ctx->cs_map[w];
    u32 mctl[2];
    int rc = cs_read_words(ctx, m.ctl, mctl, 2);
    if (rc) return rc;
    const size_t e = mctl[0];
    h.off.resize(e); h.len.resize(e); h.count.resize(e); h.arena.resize(mctl[1]);
    if (e) {
        HIP_TRY(ctx, hipMemcpyAsync(h.off.data(), m.eoff, e * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h.len.data(), m.elen, e * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h.count.data(), m.ecount, e * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (mctl[1]) HIP_TRY(ctx, hipMemcpyAsync(h.arena.data(), m.arena, mctl[1], hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    h.order.resize(e);
    for (size_t i = 0; i < e; i++) h.order[i] = (u32)i;
    std::sort(h.order.begin(), h.order.end(), [&](u32 x, u32 y) {
        if (h.len[x] != h.len[y]) return h.len[x] < h.len[y];
        return memcmp(h.arena.data() + h.off[x], h.arena.data() + h.off[y], h.len[x]) < 0;
    });
    return 0;
}

extern "C" int fastp_gpu_adapter_census_size(fastp_gpu_ctx* ctx, int is_r2, int64_t* entries, int64_t* bytes) {
    if (!ctx) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    u32 mctl[2] = {0, 0};
    const int w = is_r2 ? 1 : 0;
    if (ctx->d_cs_map[w]) {
        int rc = cs_read_words(ctx, ctx->cs_map[w].ctl, mctl, 2);
        if (rc) return rc;
    }
    if (entries) *entries = mctl[0];
    if (bytes) *bytes = mctl[1];
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_adapter_census_read(fastp_gpu_ctx* ctx, int is_r2, char* chars, int64_t chars_capacity, int64_t* off, int64_t* counts) {
    if (!ctx || !off || chars_capacity < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    CsHostMap h;
    int rc = cs_download(ctx, is_r2 ? 1 : 0, h);
    if (rc) return rc;
    if ((int64_t)h.arena.size() > chars_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "adapter census: chars_capacity too small (fastp_gpu_adapter_census_size)");
    if (!h.order.empty() && (!chars || !counts)) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    int64_t at = 0;
    for (size_t i = 0; i < h.order.size(); i++) {
        const u32 e = h.order[i];
        off[i] = at;
        memcpy(chars + at, h.arena.data() + h.off[e], h.len[e]);
        at += h.len[e];
        counts[i] = (int64_t)h.count[e];
    }
    off[h.order.size()] = at;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_adapter_census_load(fastp_gpu_ctx* ctx, int is_r2, const char* chars, const int64_t* off, const int64_t* counts, int64_t entries) {
    if (!ctx || entries < 0 || entries > CS_MAX_ENTRIES || (entries && (!chars || !off || !counts))) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = cs_ensure_maps(ctx);
    if (rc) return rc;
    const int w = is_r2 ? 1 : 0;
    const size_t E = CS_MAX_ENTRIES;
    const u64 mask = cs_hash_mask(ctx);
    // the header as the device holds it (cs_ensure_maps): ehash | ecount | index | eoff | elen | ctl
    std::vector<u8> head(cs_map_header_bytes(), 0);
    u64* ehash = (u64*)head.data();
    u64* ecount = ehash + E;
    u32* index = (u32*)(ecount + E);
    u32* eoff = index + CS_INDEX_SLOTS;
    u32* elen = eoff + E;
    u32* mctl = elen + E;
    std::vector<u8> arena;
    for (int64_t i = 0; i < entries; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len <= 0 || len > (int64_t)CS_KEY_MAX || counts[i] < 0) return fail(ctx, FASTP_GPU_E_INVALID, "adapter census load: a key must be 1..FASTP_GPU_MAX_READ_LEN bytes");
        const u8* p = (const u8*)chars + off[i];
        const u64 h = cs_host_hash(p, (u32)len, mask);
        for (u32 step = 0;; step++) {
            u32& at = index[((u32)h + step) & (CS_INDEX_SLOTS - 1)];
            if (at == 0) { at = (u32)i + 1; break; }
            const u32 e = at - 1;
            if (ehash[e] == h && elen[e] == (u32)len && !memcmp(arena.data() + eoff[e], p, (size_t)len))
                return fail(ctx, FASTP_GPU_E_INVALID, "adapter census load: the same key twice");
        }
        ehash[i] = h;
        ecount[i] = (u64)counts[i];
        eoff[i] = (u32)arena.size();
        elen[i] = (u32)len;
        arena.insert(arena.end(), p, p + len);
    }
    mctl[0] = (u32)entries;
    mctl[1] = (u32)arena.size();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cs_map[w], head.data(), head.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!arena.empty()) HIP_TRY(ctx, hipMemcpyAsync(ctx->cs_map[w].arena, arena.data(), arena.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cs_entries[w] = (u32)entries;
    return FASTP_GPU_OK;
}

// ---- Evaluator pre-pass (fq_eval.h) ---------------------------------------------------------------------
// the reads a reference loading loop `while (records < read_limit && bases < base_limit)` admits
static int eval_admit(fastp_gpu_ctx* ctx, const uint16_t* len, int32_t n, int64_t read_limit, int64_t base_limit,
                      std::vector<u16>& lens) {
    const size_t take = (size_t)std::min<int64_t>(n, read_limit);
    lens.resize(take);
    if (take) {
        HIP_TRY(ctx, hipMemcpyAsync(lens.data(), len, take * 2, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    int64_t bases = 0;
    size_t used = 0;
    while (used < take && bases < base_limit) bases += lens[used++];
    lens.resize(used);
    return 0;
}

// The listed reads of a text-aware call (fastp_gpu_eval_text): checked, then turned into EvalText's word per read.
// `on` stays false for NULL or an empty list: the call is the plain one.
static int eval_check_text(fastp_gpu_ctx* ctx, const fastp_gpu_eval_text* x, int32_t n) {
    if (!x || x->n_exotic == 0) return FASTP_GPU_OK;
    if (x->n_exotic < 0 || !x->exotic_unit || !x->exotic_text || !x->exotic_off)
        return fail(ctx, FASTP_GPU_E_INVALID, "n_exotic > 0 needs exotic_unit, exotic_text and exotic_off");
    for (int k = 0; k < x->n_exotic; k++)
        if (x->exotic_unit[k] < 0 || x->exotic_unit[k] >= n || (k && x->exotic_unit[k] <= x->exotic_unit[k - 1]))
            return fail(ctx, FASTP_GPU_E_INVALID, "exotic_unit must be ascending read indexes below n");
    return FASTP_GPU_OK;
}
static int eval_stage_text(fastp_gpu_ctx* ctx, const fastp_gpu_eval_text* x, int32_t n, EvalText& tx, bool& on) {
    on = x && x->n_exotic > 0;
    memset(&tx, 0, sizeof(tx));
    if (!on) return FASTP_GPU_OK;
    hipStream_t st = ctx->stream;
    const size_t b_off = (size_t)n * 4;
    EvalListArgs l;
    memset(&l, 0, sizeof(l));
    auto lay = [&](Carve c) {
        l.rawoff = c.take<u32>(b_off);
        l.unit = c.take<int>((size_t)x->n_exotic * 4);
        return c.off;
    };
    int rc = ensure(ctx, (void**)&ctx->d_eval_x, &ctx->eval_x_cap, lay(Carve(nullptr)));
    if (rc) return rc;
    lay(Carve(ctx->d_eval_x));
    l.n_exotic = x->n_exotic;
    l.dense = x->exotic_dense ? 1 : 0;
    l.off = x->exotic_off;
    HIP_TRY(ctx, hipMemsetAsync(l.rawoff, 0xFF, b_off, st));
    HIP_TRY(ctx, hipMemcpyAsync((void*)l.unit, x->exotic_unit, (size_t)x->n_exotic * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // the list is the caller's (pageable) memory
    hipLaunchKernelGGL(fq_eval_list_kernel, dim3((unsigned)((x->n_exotic + 255) / 256)), dim3(256), 0, st, l);
    HIP_TRY(ctx, hipGetLastError());
    tx.text = x->exotic_text;
    tx.rawoff = l.rawoff;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_eval_seq_len(fastp_gpu_ctx* ctx, const uint16_t* len, int32_t n, int32_t* seq_len) {
    if (!ctx || !seq_len || n < 0 || (n > 0 && !len)) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<u16> lens;
    int rc = eval_admit(ctx, len, n, 1000, INT64_MAX, lens);   // evaluator.cpp:63-74
    if (rc) return rc;
    int best = 0;
    for (u16 v : lens) best = std::max(best, (int)v);
    *seq_len = best;
    return FASTP_GPU_OK;
}

static int eval_adapter_kmers(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n,
                              int32_t trim_tail1, uint32_t* counts, int64_t* records, const fastp_gpu_eval_text* x) {
    if (!ctx || !counts || n < 0 || (n > 0 && (!seq || !qual || !len))) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (int rc = eval_check_text(ctx, x, n)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t READ_LIMIT = 256 * 1024, BASE_LIMIT = 151 * READ_LIMIT;   // evaluator.cpp:313-314
    std::vector<u16> lens;
    int rc = eval_admit(ctx, len, n, READ_LIMIT, BASE_LIMIT, lens);
    if (rc) return rc;
    if (records) *records = (int64_t)lens.size();
    HIP_TRY(ctx, hipMemsetAsync(counts, 0, sizeof(u32) << 20, st));
    EvalKmerArgs a;
    memset(&a, 0, sizeof(a));
    a.r.seq = seq;
    a.r.qual = qual;
    a.r.len = len;
    a.r.n = (int)lens.size();
    a.r.seq_stride = (int)fastp_gpu_seq_stride(ctx->dp.max_len);
    a.r.qual_stride = (int)fastp_gpu_qual_stride(ctx->dp.max_len);
    a.shift_tail = std::max(1, trim_tail1);
    a.span = std::max(1, ctx->dp.max_len - 29);   // positions 20 .. len - 10 - shift_tail
    a.counts = counts;
    const long long lanes = (long long)a.r.n * a.span;
    if (lanes > 0) {
        EvalText tx;
        bool text;
        rc = eval_stage_text(ctx, x, n, tx, text);
        if (rc) return rc;
        const dim3 grid((unsigned)((lanes + 255) / 256));
        if (text) hipLaunchKernelGGL(fq_eval_kmer_x_kernel, grid, dim3(256), 0, st, a, tx);
        else hipLaunchKernelGGL(fq_eval_kmer_kernel, grid, dim3(256), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_eval_adapter_kmers(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                            int32_t n, int32_t trim_tail1, uint32_t* counts, int64_t* records) {
    return eval_adapter_kmers(ctx, seq, qual, len, n, trim_tail1, counts, records, nullptr);
}
// Evaluator::seq2int (evaluator.cpp:577-626) on the listed reads' own letters: a window with anything but A T C G gives -1
extern "C" int fastp_gpu_eval_adapter_kmers_x(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                              int32_t n, int32_t trim_tail1, uint32_t* counts, int64_t* records,
                                              const fastp_gpu_eval_text* x) {
    return eval_adapter_kmers(ctx, seq, qual, len, n, trim_tail1, counts, records, x);
}

static int eval_overrep(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n, int32_t seq_len,
                        char* text, int64_t text_capacity, int64_t* off, int64_t* count, int32_t max_seqs, int32_t* n_seqs,
                        const fastp_gpu_eval_text* x) {
    if (!ctx || !n_seqs || !off || n < 0 || max_seqs < 0 || text_capacity < 0 || (n > 0 && (!seq || !qual || !len)) ||
        (max_seqs > 0 && (!text || !count)))
        return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (int rc = eval_check_text(ctx, x, n)) return rc;
    *n_seqs = 0;
    off[0] = 0;
    if (seq_len < 1) return fail(ctx, FASTP_GPU_E_INVALID, "seq_len (Evaluator::computeSeqLen) must be positive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t BASE_LIMIT = 151 * 10000;   // evaluator.cpp:83
    std::vector<u16> lens;
    int rc = eval_admit(ctx, len, n, (int64_t)(1 << 24) - 2, BASE_LIMIT, lens);
    if (rc) return rc;
    EvalCensusArgs a;
    memset(&a, 0, sizeof(a));
    a.r.seq = seq;
    a.r.qual = qual;
    a.r.len = len;
    a.r.n = (int)lens.size();
    a.r.seq_stride = (int)fastp_gpu_seq_stride(ctx->dp.max_len);
    a.r.qual_stride = (int)fastp_gpu_qual_stride(ctx->dp.max_len);
    const int steps[EVAL_STEPS] = {10, 20, 40, 100, std::min(150, seq_len - 2)};   // :97
    int min_step = 1 << 30;
    for (int i = 0; i < EVAL_STEPS; i++) {
        a.step[i] = steps[i];
        if (steps[i] > 0) min_step = std::min(min_step, steps[i]);
    }
    a.span = std::max(1, ctx->dp.max_len - min_step);
    a.seqlen = seq_len;
    uint64_t items = 0;
    for (u16 l : lens)
        for (int i = 0; i < EVAL_STEPS; i++)
            if (steps[i] > 0 && (int)l > steps[i]) items += (uint64_t)((int)l - steps[i]);
    if (items == 0) return FASTP_GPU_OK;
    uint64_t cap = 1024;
    while (cap < 2 * items) cap <<= 1;
    if (cap > (1ull << 31)) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "substring census larger than 2^30 items");
    // a substring over its threshold occurs >= 3 times
    a.hot_cap = (u32)std::min<uint64_t>(items / 3 + 16, 1u << 22);
    const size_t b_slot = cap * 8, b_count = cap * 4;
    auto lay = [&](Carve c) {
        a.slot = c.take<u64>(b_slot);
        a.count = c.take<u32>(b_count);
        a.hot = c.take<u64>((size_t)a.hot_cap * 8);
        a.hot_count = c.take<u32>((size_t)a.hot_cap * 4);
        a.n_hot = c.take<u32>(16);
        a.text = c.take((size_t)a.hot_cap * 152);
        return c.off;
    };
    rc = ensure(ctx, (void**)&ctx->d_eval, &ctx->eval_cap, lay(Carve(nullptr)));
    if (rc) return rc;
    lay(Carve(ctx->d_eval));
    a.mask = (u32)(cap - 1);
    HIP_TRY(ctx, hipMemsetAsync(a.slot, 0, b_slot + b_count, st));
    HIP_TRY(ctx, hipMemsetAsync(a.n_hot, 0, 16, st));
    const long long lanes = (long long)a.r.n * a.span;
    EvalText tx;
    bool with_text;
    rc = eval_stage_text(ctx, x, n, tx, with_text);
    if (rc) return rc;
    if (with_text) hipLaunchKernelGGL(fq_eval_census_x_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, tx);
    else hipLaunchKernelGGL(fq_eval_census_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_eval_harvest_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    u32 n_hot = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_hot, a.n_hot, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (n_hot > a.hot_cap) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "more than 4 Mi overrepresented substrings");
    std::map<std::string, long> hot;   // Options::overRepSeqs (evaluator.cpp:112-137)
    if (n_hot) {
        const dim3 grid((unsigned)(((size_t)n_hot * 16 + 255) / 256));
        if (with_text) hipLaunchKernelGGL(fq_eval_text_x_kernel, grid, dim3(256), 0, st, a, tx);
        else hipLaunchKernelGGL(fq_eval_text_kernel, grid, dim3(256), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        std::vector<u64> hw(n_hot);
        std::vector<u32> hc(n_hot);
        std::vector<u8> ht((size_t)n_hot * 152);
        HIP_TRY(ctx, hipMemcpyAsync(hw.data(), a.hot, (size_t)n_hot * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(hc.data(), a.hot_count, (size_t)n_hot * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(ht.data(), a.text, ht.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (u32 k = 0; k < n_hot; k++)
            hot[std::string((const char*)&ht[(size_t)k * 152], (size_t)steps[(hw[k] >> 21) & 7u])] = (long)hc[k];
    }
    // "remove substrings" (evaluator.cpp:139-160), erasing while iterating as the reference does
    for (auto it = hot.begin(); it != hot.end();) {
        bool is_sub = false;
        for (auto it2 = hot.begin(); it2 != hot.end(); ++it2)
            if (it->first != it2->first && it2->first.find(it->first) != std::string::npos && it->second / it2->second < 10) {
                is_sub = true;
                break;
            }
        if (is_sub) it = hot.erase(it);
        else ++it;
    }
    *n_seqs = (int32_t)hot.size();
    if ((int64_t)hot.size() > max_seqs) return fail(ctx, FASTP_GPU_E_OVERFLOW, "more sequences than max_seqs");
    int64_t at = 0;
    int32_t i = 0;
    for (const auto& kv : hot) {
        if (at + (int64_t)kv.first.size() > text_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "text buffer too small");
        memcpy(text + at, kv.first.data(), kv.first.size());
        at += (int64_t)kv.first.size();
        count[i] = kv.second;
        off[++i] = at;
    }
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_eval_overrep(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n,
                                      int32_t seq_len, char* text, int64_t text_capacity, int64_t* off, int64_t* count,
                                      int32_t max_seqs, int32_t* n_seqs) {
    return eval_overrep(ctx, seq, qual, len, n, seq_len, text, text_capacity, off, count, max_seqs, n_seqs, nullptr);
}
// computeOverRepSeq's raw substrings (evaluator.cpp:99-110, :115-160): a byte outside ACGTN equals only the same byte;
// thresholds, the containment pass and the map's order work on the bytes
extern "C" int fastp_gpu_eval_overrep_x(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n,
                                        int32_t seq_len, char* text, int64_t text_capacity, int64_t* off, int64_t* count,
                                        int32_t max_seqs, int32_t* n_seqs, const fastp_gpu_eval_text* x) {
    return eval_overrep(ctx, seq, qual, len, n, seq_len, text, text_capacity, off, count, max_seqs, n_seqs, x);
}

// Evaluator::checkKnownAdapters: the match kernel over every (read, adapter), the replay of the loop's state machine over
// the matched pairs, the final choice (:291-305) here.  The list is the caller's; it is walked in std::map order.
static int eval_known_adapters(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n,
                               const char* const* adapters, int32_t n_adapters, int32_t* counts, int32_t* mismatches,
                               int64_t* checked_reads, int32_t* best, const fastp_gpu_eval_text* x) {
    if (!ctx || !checked_reads || !best || n < 0 || n_adapters < 0 || (n > 0 && (!seq || !qual || !len)) ||
        (n_adapters > 0 && (!adapters || !counts || !mismatches)))
        return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (int rc = eval_check_text(ctx, x, n)) return rc;
    *best = -1;
    *checked_reads = 0;
    if (n_adapters > EVAL_MAX_ADAPTERS) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "more than 1024 known adapters");
    const int A = n_adapters;
    std::vector<int> order(A);   // map order -> the caller's index
    int max_alen = 0;
    for (int i = 0; i < A; i++) {
        order[i] = i;
        if (!adapters[i] || !adapters[i][0]) return fail(ctx, FASTP_GPU_E_INVALID, "empty known adapter");
        const size_t l = strlen(adapters[i]);
        if (l > FASTP_GPU_MAX_ADAPTER_LEN) return fail(ctx, FASTP_GPU_E_UNSUPPORTED, "known adapter longer than FASTP_GPU_MAX_ADAPTER_LEN");
        for (size_t k = 0; k < l; k++)
            if (!strchr("ACGT", adapters[i][k])) return fail(ctx, FASTP_GPU_E_INVALID, "known adapter with a letter outside ACGT");
        max_alen = std::max(max_alen, (int)l);
    }
    std::sort(order.begin(), order.end(), [&](int x, int y) { return strcmp(adapters[x], adapters[y]) < 0; });
    for (int i = 1; i < A; i++)
        if (!strcmp(adapters[order[i - 1]], adapters[order[i]]))
            return fail(ctx, FASTP_GPU_E_INVALID, "the same known adapter twice (a std::map holds it once)");
    for (int i = 0; i < A; i++) counts[i] = mismatches[i] = 0;
    // checkedReads without a list: the loop only counts (and the base limit cannot bind, fq_eval.h)
    *checked_reads = n > EVAL_CHECK_READS ? EVAL_CHECK_READS + 1 : n;
    if (A == 0 || n == 0) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    EvalMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.r.seq = seq;
    a.r.qual = qual;
    a.r.len = len;
    a.r.n = std::min<int>(n, EVAL_CHECK_READS);
    a.r.seq_stride = (int)fastp_gpu_seq_stride(ctx->dp.max_len);
    a.r.qual_stride = (int)fastp_gpu_qual_stride(ctx->dp.max_len);
    a.n_all = n;
    a.n_adapters = A;
    a.ad_words = (max_alen + 31) / 32;
    a.bit_words = (A + 31) / 32;
    std::vector<u64> words((size_t)A * a.ad_words, 0ull);
    std::vector<u16> alen((size_t)A);
    for (int i = 0; i < A; i++) {
        const char* s = adapters[order[i]];
        alen[i] = (u16)strlen(s);
        for (int k = 0; s[k]; k++) {
            const u64 code = s[k] == 'A' ? 0u : s[k] == 'T' ? 1u : s[k] == 'C' ? 2u : 3u;   // the packed rows' coding
            words[(size_t)i * a.ad_words + k / 32] |= code << (2 * (k % 32));
        }
    }
    const size_t b_cnt = 8 + (size_t)A * 8;   // checkedReads | possibleCounts, mismatches: they come back in one copy
    auto lay = [&](Carve c) {
        a.words = c.take<u64>(words.size() * 8);
        a.alen = c.take<u16>((size_t)A * 2, 8);
        a.checked = c.take<long long>(8);
        a.counts = c.take<int>((size_t)A * 8);
        a.bits = c.take<u32>((size_t)a.r.n * a.bit_words * 4, 8);
        a.mm = c.take((size_t)a.r.n * A);
        return c.off;
    };
    int rc = ensure(ctx, (void**)&ctx->d_eval, &ctx->eval_cap, lay(Carve(nullptr)));
    if (rc) return rc;
    lay(Carve(ctx->d_eval));
    HIP_TRY(ctx, hipMemcpyAsync((void*)a.words, words.data(), words.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync((void*)a.alen, alen.data(), (size_t)A * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));   // (the staging vectors are pageable)
    EvalText tx;
    bool with_text;
    rc = eval_stage_text(ctx, x, n, tx, with_text);
    if (rc) return rc;
    const dim3 grid((unsigned)((a.r.n + EVAL_MATCH_WAVES - 1) / EVAL_MATCH_WAVES));
    const size_t lds = (size_t)EVAL_MATCH_WAVES * (EVAL_MATCH_LDS + a.bit_words * 32) * 4;
    if (with_text)   // + 512 bytes of a listed read per wavefront
        hipLaunchKernelGGL(fq_eval_match_x_kernel, grid, dim3(64 * EVAL_MATCH_WAVES), lds + (size_t)EVAL_MATCH_WAVES * 512, st, a, tx);
    else hipLaunchKernelGGL(fq_eval_match_kernel, grid, dim3(64 * EVAL_MATCH_WAVES), lds, st, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_eval_replay_kernel, dim3(1), dim3(64), (size_t)A * 8, st, a);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int> res((size_t)2 * A + 2);
    HIP_TRY(ctx, hipMemcpyAsync(res.data(), a.checked, b_cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    long long checked;
    memcpy(&checked, res.data(), 8);
    *checked_reads = checked;
    int top = -1, max_count = 0;   // :291-299: the first in map order with the strictly largest count
    for (int i = 0; i < A; i++) {
        counts[order[i]] = res[2 + i];
        mismatches[order[i]] = res[2 + A + i];
        if (res[2 + i] > max_count) {
            max_count = res[2 + i];
            top = i;
        }
    }
    if (top >= 0 && (max_count > checked / 50 || (max_count > checked / 200 && res[2 + A + top] < checked))) *best = order[top];
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_eval_known_adapters(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                             int32_t n, const char* const* adapters, int32_t n_adapters, int32_t* counts,
                                             int32_t* mismatches, int64_t* checked_reads, int32_t* best) {
    return eval_known_adapters(ctx, seq, qual, len, n, adapters, n_adapters, counts, mismatches, checked_reads, best, nullptr);
}
// checkKnownAdapters' raw != (evaluator.cpp:266-287): a byte outside ACGTN is a mismatch inside the cmplen / 16 allowance
extern "C" int fastp_gpu_eval_known_adapters_x(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                               int32_t n, const char* const* adapters, int32_t n_adapters, int32_t* counts,
                                               int32_t* mismatches, int64_t* checked_reads, int32_t* best,
                                               const fastp_gpu_eval_text* x) {
    return eval_known_adapters(ctx, seq, qual, len, n, adapters, n_adapters, counts, mismatches, checked_reads, best, x);
}

// Evaluator::getAdapterWithSeed's two scans and the two NucleotideTree::getDominantPath walks for one seed
static int eval_adapter_seed(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len, int32_t n,
                             int32_t trim_tail1, uint32_t seed, char* forward, int32_t* forward_len, char* backward,
                             int32_t* backward_len, int32_t* reached_leaf, int64_t* hits, const fastp_gpu_eval_text* x) {
    if (!ctx || !forward || !forward_len || !backward || !backward_len || !reached_leaf || !hits || n < 0 || seed >= (1u << 20) ||
        (n > 0 && (!seq || !qual || !len)))
        return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (int rc = eval_check_text(ctx, x, n)) return rc;
    *forward_len = *backward_len = 0;
    *reached_leaf = 1;
    *hits = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t READ_LIMIT = 256 * 1024, BASE_LIMIT = 151 * READ_LIMIT;   // evaluator.cpp:313-314
    std::vector<u16> lens;
    int rc = eval_admit(ctx, len, n, READ_LIMIT, BASE_LIMIT, lens);
    if (rc) return rc;
    EvalSeedArgs a;
    memset(&a, 0, sizeof(a));
    a.r.seq = seq;
    a.r.qual = qual;
    a.r.len = len;
    a.r.n = (int)lens.size();
    a.r.seq_stride = (int)fastp_gpu_seq_stride(ctx->dp.max_len);
    a.r.qual_stride = (int)fastp_gpu_qual_stride(ctx->dp.max_len);
    a.shift_tail = std::max(1, trim_tail1);
    a.span = std::min(480, std::max(1, ctx->dp.max_len - 29));   // positions 20 .. min(len - 10 - shift_tail, 499)
    a.seed = seed;
    const long long lanes = (long long)a.r.n * a.span;
    if (lanes == 0) return FASTP_GPU_OK;
    EvalText tx;
    bool with_text;
    rc = eval_stage_text(ctx, x, n, tx, with_text);
    if (rc) return rc;
    // count the hits, size the list by the count, list them
    u64 nh = 0;
    for (int pass = 0; pass < 2; pass++) {
        auto lay = [&](Carve c) {   // n_hits | path_len[2], reached_leaf | the two paths | the hit list
            a.n_hits = c.take<u64>(8);
            a.path_len = c.take<int>(16);
            a.path = c.take(1024);
            a.hits = c.take<u32>((size_t)nh * 4);
            return c.off;
        };
        rc = ensure(ctx, (void**)&ctx->d_eval, &ctx->eval_cap, lay(Carve(nullptr)));
        if (rc) return rc;
        lay(Carve(ctx->d_eval));
        if (!pass) a.hits = nullptr;
        a.cap = nh;
        HIP_TRY(ctx, hipMemsetAsync(a.n_hits, 0, 24, st));
        if (with_text) hipLaunchKernelGGL(fq_eval_seed_gather_x_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, tx);
        else hipLaunchKernelGGL(fq_eval_seed_gather_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a);
        HIP_TRY(ctx, hipGetLastError());
        if (pass) break;
        HIP_TRY(ctx, hipMemcpyAsync(&nh, a.n_hits, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        *hits = (int64_t)nh;
        if (nh < 50) return FASTP_GPU_OK;   // NUM_THRESHOLD: both walks end at the root, reachedLeaf stays
    }
    const int one = 1;
    HIP_TRY(ctx, hipMemcpyAsync(a.path_len + 2, &one, 4, hipMemcpyHostToDevice, st));
    if (with_text) hipLaunchKernelGGL(fq_eval_seed_walk_x_kernel, dim3(2), dim3(1024), 64, st, a, tx);   // 8 bins | their creators
    else hipLaunchKernelGGL(fq_eval_seed_walk_kernel, dim3(2), dim3(1024), 16, st, a);
    HIP_TRY(ctx, hipGetLastError());
    u8 out[16 + 1024];
    HIP_TRY(ctx, hipMemcpyAsync(out, a.path_len, sizeof(out), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    int head[4];
    memcpy(head, out, 16);
    *forward_len = head[0];
    *backward_len = head[1];
    *reached_leaf = head[2];
    memcpy(forward, out + 16, (size_t)head[0]);
    memcpy(backward, out + 16 + 512, (size_t)head[1]);
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_eval_adapter_seed(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                           int32_t n, int32_t trim_tail1, uint32_t seed, char* forward, int32_t* forward_len,
                                           char* backward, int32_t* backward_len, int32_t* reached_leaf, int64_t* hits) {
    return eval_adapter_seed(ctx, seq, qual, len, n, trim_tail1, seed, forward, forward_len, backward, backward_len, reached_leaf,
                             hits, nullptr);
}
// the hit search by seq2int (evaluator.cpp:577-626) and NucleotideTree on raw bytes (nucleotidetree.cpp:42-88): eight
// children by byte & 7, only 'N' cuts, a node prints its creator's byte
extern "C" int fastp_gpu_eval_adapter_seed_x(fastp_gpu_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint16_t* len,
                                             int32_t n, int32_t trim_tail1, uint32_t seed, char* forward, int32_t* forward_len,
                                             char* backward, int32_t* backward_len, int32_t* reached_leaf, int64_t* hits,
                                             const fastp_gpu_eval_text* x) {
    return eval_adapter_seed(ctx, seq, qual, len, n, trim_tail1, seed, forward, forward_len, backward, backward_len, reached_leaf,
                             hits, x);
}

// ---- output text -> BGZF-framed gzip members (fq_deflate.h) ------------------------------------------------
// the reference's -z (1..9; 0 = the default) -> the match stage: levels up to 4 are the one-candidate greedy stage, 5..7 and 8..9
// the chain stage at two depths (DESIGN.md 7 has the table and what each tier costs)
// a round = what is in flight at once (a wavefront per block, eight per CU): the scratch is sized by it - 4 bytes of
// tokens per input byte + a member slot per block - so a larger round only costs HBM.  table_entries: room for the block
// table of fastp_gpu_deflate_bgzf_segments behind it (*d_table).
static int deflate_scratch(fastp_gpu_ctx* ctx, int round, bool chain, int chain_grid, size_t table_entries, DeflateArgs& scratch,
                           DefBlockEnt** d_table) {
    memset(&scratch, 0, sizeof(scratch));
    if (round <= 0) return 0;
    auto lay = [&](Carve c) {
        if (d_table) *d_table = c.take<DefBlockEnt>(table_entries * sizeof(DefBlockEnt), 16);   // (in front: its u64 fields stay aligned)
        scratch.slots = c.take((size_t)round * DEF_SLOT);
        scratch.tokens = c.take<u32>((size_t)round * DEF_BLOCK * 4);
        scratch.sizes = c.take<u32>((size_t)round * 4 + 8);
        scratch.offs = c.take<u64>(((size_t)round + 1) * 8);
        if (chain) scratch.prev = c.take<u16>((size_t)chain_grid * DEF_PREV * 2);   // (a chain array per RESIDENT workgroup: 128 KB x 5 per CU)
        return c.off;
    };
    int rc = ensure(ctx, (void**)&ctx->d_def, &ctx->def_cap, lay(Carve(nullptr)));
    if (rc) return rc;
    lay(Carve(ctx->d_def));
    return 0;
}
// the three kernels of one round: members into their slots, their offsets, members to their place in the output
static int deflate_launch_round(fastp_gpu_ctx* ctx, DeflateArgs& a, bool chain, int chain_grid, u32 chain_depth, u32 chain_lazy) {
    hipStream_t st = ctx->stream;
    if (chain) {
        a.depth = chain_depth;
        a.lazy_max = chain_lazy;
        const int grid = std::min(a.nblocks, chain_grid);
        hipLaunchKernelGGL(fq_deflate_chain_kernel, dim3(grid), dim3(64), sizeof(DefChainLds), st, a);
    } else {
        const int grid = std::min(a.nblocks, ctx->cus * std::max(1, ctx->lds_bytes / (int)sizeof(DefLds)));
        hipLaunchKernelGGL(fq_deflate_kernel, dim3(grid), dim3(64), sizeof(DefLds), st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_deflate_scan_kernel, dim3(1), dim3(1024), 1024 * 8, st, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(fq_deflate_gather_kernel, dim3(std::min(a.nblocks, ctx->cus * 16)), dim3(256), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

extern "C" int fastp_gpu_deflate_bgzf_level(fastp_gpu_ctx* ctx, const uint8_t* text, int64_t nbytes, int write_eof, int level, uint8_t* out,
                                            int64_t out_capacity, int64_t* out_len) {
    if (!ctx || !out_len || nbytes < 0 || out_capacity < 0 || (nbytes > 0 && !text) || (out_capacity > 0 && !out))
        return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (level < 0 || level > 9) return fail(ctx, FASTP_GPU_E_INVALID, "compression level outside 0..9");
    const bool chain = level >= 5;
    const u32 chain_depth = level >= 8 ? 16u : 4u, chain_lazy = 32u;
    *out_len = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    static const uint8_t eof_member[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t total_blocks = (nbytes + DEF_BLOCK - 1) / DEF_BLOCK;
    const int round = (int)std::min<int64_t>(total_blocks, (int64_t)ctx->cus * 8);
    const int chain_grid = chain ? std::min(round, ctx->cus * std::max(1, ctx->lds_bytes / (int)sizeof(DefChainLds))) : 0;
    DeflateArgs scratch;
    int rc = deflate_scratch(ctx, round, chain, chain_grid, 0, scratch, nullptr);
    if (rc) return rc;
    u64 written = 0;   // bytes needed so far
    for (int64_t b0 = 0; b0 < total_blocks; b0 += round) {
        DeflateArgs a = scratch;
        a.nblocks = (int)std::min<int64_t>(round, total_blocks - b0);
        a.text = text + (size_t)b0 * DEF_BLOCK;
        a.nbytes = (u64)std::min<int64_t>(nbytes - b0 * DEF_BLOCK, (int64_t)a.nblocks * DEF_BLOCK);
        a.out = out;
        a.out_base = written;
        a.out_cap = (u64)out_capacity;
        rc = deflate_launch_round(ctx, a, chain, chain_grid, chain_depth, chain_lazy);
        if (rc) return rc;
        u64 bytes = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&bytes, a.offs + a.nblocks, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        written += bytes;
    }
    if (write_eof) {
        if (written + sizeof(eof_member) <= (u64)out_capacity) {
            HIP_TRY(ctx, hipMemcpyAsync(out + written, eof_member, sizeof(eof_member), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        written += sizeof(eof_member);
    }
    *out_len = (int64_t)written;
    if (written > (u64)out_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "output buffer too small (see out_len for the needed size)");
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_deflate_bgzf(fastp_gpu_ctx* ctx, const uint8_t* text, int64_t nbytes, int write_eof, uint8_t* out,
                                      int64_t out_capacity, int64_t* out_len) {
    return fastp_gpu_deflate_bgzf_level(ctx, text, nbytes, write_eof, 0, out, out_capacity, out_len);
}

// the same kernels with a block table: the blocks of every segment (DEF_BLOCK bytes from the segment's start on), the
// end-of-file members written by the gather kernel behind the last block of a flagged segment.  The rounds run over the
// table, whatever segment a block belongs to.
extern "C" int fastp_gpu_deflate_bgzf_segments(fastp_gpu_ctx* ctx, const uint8_t* text, int32_t n_segments, const int64_t* seg_off,
                                               const uint8_t* seg_eof, int level, uint8_t* out, int64_t out_capacity, int64_t* seg_out_off) {
    if (!ctx || n_segments < 0 || !seg_off || !seg_out_off || out_capacity < 0 || (out_capacity > 0 && !out))
        return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (level < 0 || level > 9) return fail(ctx, FASTP_GPU_E_INVALID, "compression level outside 0..9");
    for (int32_t i = 0; i <= n_segments; i++) seg_out_off[i] = 0;
    if (seg_off[0] < 0) return fail(ctx, FASTP_GPU_E_INVALID, "negative segment offset");
    for (int32_t i = 0; i < n_segments; i++)
        if (seg_off[i + 1] < seg_off[i]) return fail(ctx, FASTP_GPU_E_INVALID, "segment offsets must ascend");
    if (n_segments > 0 && seg_off[n_segments] > seg_off[0] && !text) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    const bool chain = level >= 5;
    const u32 chain_depth = level >= 8 ? 16u : 4u, chain_lazy = 32u;
    std::vector<DefBlockEnt> table;
    std::vector<size_t> seg_first((size_t)n_segments + 1);   // a segment's first table entry
    u64 eof_bytes = 0;
    for (int32_t i = 0; i < n_segments; i++) {
        seg_first[i] = table.size();
        const bool eof = seg_eof && seg_eof[i];
        for (int64_t at = seg_off[i]; at < seg_off[i + 1]; at += DEF_BLOCK)
            table.push_back(DefBlockEnt{(u64)at, (u32)std::min<int64_t>(DEF_BLOCK, seg_off[i + 1] - at), 0u, eof_bytes});
        if (eof) {
            if (table.size() == seg_first[i]) table.push_back(DefBlockEnt{(u64)seg_off[i], 0u, 0u, eof_bytes});
            table.back().eof = 1;
            eof_bytes += 28;
        }
    }
    seg_first[n_segments] = table.size();
    const int64_t total_blocks = (int64_t)table.size();
    if (total_blocks == 0) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int round = (int)std::min<int64_t>(total_blocks, (int64_t)ctx->cus * 8);
    const int chain_grid = chain ? std::min(round, ctx->cus * std::max(1, ctx->lds_bytes / (int)sizeof(DefChainLds))) : 0;
    DeflateArgs scratch;
    DefBlockEnt* d_table = nullptr;
    int rc = deflate_scratch(ctx, round, chain, chain_grid, table.size(), scratch, &d_table);
    if (rc) return rc;
    // (synchronous: `table` is pageable and dies with this call, whatever path it returns by)
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipMemcpy(d_table, table.data(), table.size() * sizeof(DefBlockEnt), hipMemcpyHostToDevice));
    std::vector<u64> member_at(table.size() + 1);   // where each block's member starts, without the end-of-file members
    std::vector<u64> offs((size_t)round + 1);
    u64 written = 0;
    for (int64_t b0 = 0; b0 < total_blocks; b0 += round) {
        DeflateArgs a = scratch;
        a.nblocks = (int)std::min<int64_t>(round, total_blocks - b0);
        a.text = text;
        a.table = d_table + b0;
        a.out = out;
        a.out_base = written;
        a.out_cap = (u64)out_capacity;
        rc = deflate_launch_round(ctx, a, chain, chain_grid, chain_depth, chain_lazy);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(offs.data(), a.offs, ((size_t)a.nblocks + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int b = 0; b < a.nblocks; b++) member_at[(size_t)b0 + b] = written + offs[b];
        written += offs[a.nblocks];
    }
    member_at[table.size()] = written;
    for (int32_t i = 0; i < n_segments; i++) seg_out_off[i] = (int64_t)(member_at[seg_first[i]] + (seg_first[i] < table.size() ? table[seg_first[i]].shift : eof_bytes));
    seg_out_off[n_segments] = (int64_t)(written + eof_bytes);
    if (written + eof_bytes > (u64)out_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "output buffer too small (see seg_out_off[n_segments] for the needed size)");
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_device_alloc(fastp_gpu_ctx* ctx, int64_t bytes, void** dev_ptr) {
    if (!ctx || !dev_ptr || bytes < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    *dev_ptr = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(dev_ptr, (size_t)std::max<int64_t>(bytes, 16)) != hipSuccess) {
        *dev_ptr = nullptr;
        return fail(ctx, FASTP_GPU_E_NOMEM, "hipMalloc failed");
    }
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_device_free(fastp_gpu_ctx* ctx, void* dev_ptr) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    if (!dev_ptr) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(dev_ptr));
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_device_upload(fastp_gpu_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!dst_dev || !src_host))) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (bytes == 0) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_device_download(fastp_gpu_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!dst_host || !src_dev))) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    if (bytes == 0) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_synchronize(fastp_gpu_ctx* ctx) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

// host submits: the raw text and offsets of the batch's exotic units (fastp_gpu_batch::exotic_*) go to HBM with it
static int stage_exotic(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, fastp_gpu_batch* db, hipStream_t st) {
    if (b->n_exotic <= 0) return FASTP_GPU_OK;
    if (b->exotic_dense) return fail(ctx, FASTP_GPU_E_INVALID, "exotic_dense describes text that is already in HBM (fastp_gpu_submit_device)");
    const int mates = ctx->dp.paired ? 2 : 1;
    for (int m = 0; m < mates; m++) {
        if (!b->exotic_text[m] || !b->exotic_off[m] || b->exotic_text_bytes[m] <= 0)
            return fail(ctx, FASTP_GPU_E_INVALID, "n_exotic > 0 needs exotic_text, exotic_off and exotic_text_bytes");
        int rc = ensure(ctx, &ctx->d_x_text[m], &ctx->x_text_cap[m], (size_t)b->exotic_text_bytes[m] + 16);
        if (rc) return rc;
        rc = ensure(ctx, &ctx->d_x_off[m], &ctx->x_off_cap[m], (size_t)b->n_exotic * 4);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_x_text[m], b->exotic_text[m], (size_t)b->exotic_text_bytes[m], hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_x_off[m], b->exotic_off[m], (size_t)b->n_exotic * 4, hipMemcpyHostToDevice, st));
        db->exotic_text[m] = (const uint8_t*)ctx->d_x_text[m];
        db->exotic_off[m] = (const uint32_t*)ctx->d_x_off[m];
    }
    return FASTP_GPU_OK;
}

// ---- host submits (include/fastp_gpu.h "Pipelined host submits"; fastp_gpu_submit_host is one submit and its wait) ----
extern "C" int fastp_gpu_host_alloc(fastp_gpu_ctx* ctx, int64_t bytes, void** ptr) {
    if (!ctx || !ptr || bytes < 0) return fail(ctx, FASTP_GPU_E_INVALID, "bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostMalloc(ptr, (size_t)std::max<int64_t>(bytes, 16)));
    return FASTP_GPU_OK;
}
extern "C" int fastp_gpu_host_free(fastp_gpu_ctx* ctx, void* ptr) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    if (ptr) HIP_TRY(ctx, hipHostFree(ptr));
    return FASTP_GPU_OK;
}

// One batch in host memory through a slot: its rows into the slot's device staging, the step, the records back - all queued
// on the context's stream, the slot's event behind them.  Nothing is queued before every input has been checked; once
// something is, a failure drains the stream (the caller may reuse its buffers as soon as the call has returned).
static int submit_slot(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, fastp_gpu_results* res, fastp_gpu_ctx::AsyncSlot& sl) {
    const int mates = ctx->dp.paired ? 2 : 1;
    const void* hs[2][3] = {{b->seq1, b->qual1, b->len1}, {b->seq2, b->qual2, b->len2}};
    for (int m = 0; m < mates; m++)
        if (!hs[m][0] || !hs[m][1] || !hs[m][2]) return fail(ctx, FASTP_GPU_E_INVALID, "missing input buffer");
    if (!res->r1 || (mates == 2 && (!res->r2 || !res->pair))) return fail(ctx, FASTP_GPU_E_INVALID, "missing result buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!sl.done) HIP_TRY(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (!sl.counts) HIP_TRY(ctx, hipHostMalloc((void**)&sl.counts, 64));
    const size_t n = (size_t)b->n;
    const size_t in_bytes[3] = {n * fastp_gpu_seq_stride(ctx->dp.max_len), n * fastp_gpu_qual_stride(ctx->dp.max_len), n * 2};
    const size_t corr_cap = (res->corrections && res->corrections_capacity > 0) ? (size_t)res->corrections_capacity : 0;
    const size_t ev_cap = (res->adapter_events && res->adapter_events_capacity > 0) ? (size_t)res->adapter_events_capacity : 0;
    void* dsq[2][3];
    fastp_gpu_results dr;
    memset(&dr, 0, sizeof(dr));
    dr.corrections_capacity = (int32_t)corr_cap;
    dr.adapter_events_capacity = (int32_t)ev_cap;
    auto lay = [&](Carve c) {   // every piece on a 256-byte boundary
        for (int m = 0; m < mates; m++)
            for (int k = 0; k < 3; k++) dsq[m][k] = c.take(in_bytes[k], 256);
        dr.r1 = c.take<fastp_gpu_read_result>(n * sizeof(fastp_gpu_read_result), 256);
        if (mates == 2) {
            dr.r2 = c.take<fastp_gpu_read_result>(n * sizeof(fastp_gpu_read_result), 256);
            dr.pair = c.take<fastp_gpu_pair_result>(n * sizeof(fastp_gpu_pair_result), 256);
        }
        if (corr_cap) dr.corrections = c.take<fastp_gpu_correction>(corr_cap * sizeof(fastp_gpu_correction), 256);
        dr.n_corrections = c.take<int32_t>(sizeof(int32_t), 256);
        if (ev_cap) dr.adapter_events = c.take<fastp_gpu_adapter_event>(ev_cap * sizeof(fastp_gpu_adapter_event), 256);
        dr.n_adapter_events = c.take<int32_t>(sizeof(int32_t), 256);
        return c.off;
    };
    int rc = ensure(ctx, &sl.d_stage, &sl.cap, lay(Carve(nullptr)));
    if (rc) return rc;
    lay(Carve(sl.d_stage));
    hipStream_t st = ctx->stream;
    fastp_gpu_batch db = *b;
    db.seq1 = (const uint8_t*)dsq[0][0]; db.qual1 = (const uint8_t*)dsq[0][1]; db.len1 = (const uint16_t*)dsq[0][2];
    if (mates == 2) {
        db.seq2 = (const uint8_t*)dsq[1][0]; db.qual2 = (const uint8_t*)dsq[1][1]; db.len2 = (const uint16_t*)dsq[1][2];
    }
    auto queue = [&]() -> int {
        for (int m = 0; m < mates; m++)
            for (int k = 0; k < 3; k++) HIP_TRY(ctx, hipMemcpyAsync(dsq[m][k], hs[m][k], in_bytes[k], hipMemcpyHostToDevice, st));
        if (int e = stage_exotic(ctx, b, &db, st)) return e;
        if (int e = fastp_gpu_submit_device(ctx, &db, &dr, st)) return e;
        HIP_TRY(ctx, hipMemcpyAsync(res->r1, dr.r1, n * sizeof(fastp_gpu_read_result), hipMemcpyDeviceToHost, st));
        if (mates == 2) {
            HIP_TRY(ctx, hipMemcpyAsync(res->r2, dr.r2, n * sizeof(fastp_gpu_read_result), hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(res->pair, dr.pair, n * sizeof(fastp_gpu_pair_result), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipMemcpyAsync(&sl.counts[0], dr.n_corrections, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&sl.counts[1], dr.n_adapter_events, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(sl.done, st));
        return FASTP_GPU_OK;
    };
    rc = queue();
    if (rc) {   // copies from and to the caller's buffers may be queued: they must have drained before the caller may reuse them
        (void)hipStreamSynchronize(st);
        return rc;
    }
    // the sparse lists (--correction / --adapter_fasta) come out in finish_slot: their fill is only known once the batch has run,
    // and copying their whole capacity with every batch multiplied the D2H traffic of a window by ten
    sl.d_corr = dr.corrections;
    sl.d_ev = dr.adapter_events;
    sl.res = *res;
    sl.busy = true;
    return FASTP_GPU_OK;
}

static int finish_slot(fastp_gpu_ctx* ctx, fastp_gpu_ctx::AsyncSlot& sl) {
    sl.busy = false;
    const int32_t ncorr = sl.counts[0], nev = sl.counts[1];
    // the entries that were written, on the slot's own stream (the launch stream may already hold the next batches)
    const int32_t ccopy = sl.d_corr ? std::min(ncorr, sl.res.corrections_capacity) : 0, ecopy = sl.d_ev ? std::min(nev, sl.res.adapter_events_capacity) : 0;
    if (ccopy > 0 || ecopy > 0) {
        if (!sl.copy) HIP_TRY(ctx, hipStreamCreateWithFlags(&sl.copy, hipStreamNonBlocking));
        if (ccopy > 0) HIP_TRY(ctx, hipMemcpyAsync(sl.res.corrections, sl.d_corr, (size_t)ccopy * sizeof(fastp_gpu_correction), hipMemcpyDeviceToHost, sl.copy));
        if (ecopy > 0) HIP_TRY(ctx, hipMemcpyAsync(sl.res.adapter_events, sl.d_ev, (size_t)ecopy * sizeof(fastp_gpu_adapter_event), hipMemcpyDeviceToHost, sl.copy));
        HIP_TRY(ctx, hipStreamSynchronize(sl.copy));
    }
    if (sl.res.n_corrections) *sl.res.n_corrections = std::min(ncorr, sl.res.corrections ? sl.res.corrections_capacity : 0);
    if (sl.res.n_adapter_events) *sl.res.n_adapter_events = std::min(nev, sl.res.adapter_events ? sl.res.adapter_events_capacity : 0);
    if (sl.res.corrections && ncorr > sl.res.corrections_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "correction list capacity exceeded");
    if (sl.res.adapter_events && nev > sl.res.adapter_events_capacity) return fail(ctx, FASTP_GPU_E_OVERFLOW, "adapter event list capacity exceeded");
    return FASTP_GPU_OK;
}

static int wait_slot(fastp_gpu_ctx* ctx, fastp_gpu_ctx::AsyncSlot& sl) {
    if (!sl.busy) return FASTP_GPU_OK;
    HIP_TRY(ctx, hipEventSynchronize(sl.done));
    return finish_slot(ctx, sl);
}

extern "C" int fastp_gpu_submit_host(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, fastp_gpu_results* res) {
    if (!ctx || !b || !res) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    if (b->n < 0) return fail(ctx, FASTP_GPU_E_INVALID, "negative batch size");
    if (b->n == 0) { if (res->n_corrections) *res->n_corrections = 0; return FASTP_GPU_OK; }
    fastp_gpu_ctx::AsyncSlot& sl = ctx->aslot[FASTP_GPU_ASYNC_SLOTS];   // the context's own slot
    const int rc = submit_slot(ctx, b, res, sl);
    return rc ? rc : wait_slot(ctx, sl);
}

extern "C" int fastp_gpu_submit_host_async(fastp_gpu_ctx* ctx, const fastp_gpu_batch* b, fastp_gpu_results* res, int slot) {
    if (!ctx || !b || !res) return fail(ctx, FASTP_GPU_E_INVALID, "null argument");
    if (slot < 0 || slot >= FASTP_GPU_ASYNC_SLOTS) return fail(ctx, FASTP_GPU_E_INVALID, "slot out of range");
    if (b->n <= 0) return fail(ctx, FASTP_GPU_E_INVALID, "empty batch");
    if (ctx->aslot[slot].busy) return fail(ctx, FASTP_GPU_E_INVALID, "slot still in flight: fastp_gpu_wait it first");
    return submit_slot(ctx, b, res, ctx->aslot[slot]);
}

extern "C" int fastp_gpu_wait(fastp_gpu_ctx* ctx, int slot) {
    if (!ctx || slot < 0 || slot >= FASTP_GPU_ASYNC_SLOTS) return fail(ctx, FASTP_GPU_E_INVALID, "slot out of range");
    return wait_slot(ctx, ctx->aslot[slot]);
}

extern "C" int fastp_gpu_poll(fastp_gpu_ctx* ctx, int slot) {
    if (!ctx || slot < 0 || slot >= FASTP_GPU_ASYNC_SLOTS) return fail(ctx, FASTP_GPU_E_INVALID, "slot out of range");
    fastp_gpu_ctx::AsyncSlot& sl = ctx->aslot[slot];
    if (!sl.busy) return 1;
    const hipError_t e = hipEventQuery(sl.done);
    if (e == hipErrorNotReady) return 0;
    if (e != hipSuccess) { HIP_TRY(ctx, e); }
    const int rc = finish_slot(ctx, sl);
    return rc ? rc : 1;
}

extern "C" int fastp_gpu_counters_device(fastp_gpu_ctx* ctx, int64_t** dev_ptr, int64_t* n, void* hip_stream) {
    if (!ctx || !dev_ptr || !n) return FASTP_GPU_E_INVALID;
    (void)hip_stream;  // slabs are folded right after every launch, on the launch stream
    *dev_ptr = ctx->d_ctr;
    *n = ctx->cl.total;
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_counters(fastp_gpu_ctx* ctx, int64_t* out, int64_t n) {
    if (!ctx || !out || n != ctx->cl.total) return fail(ctx, FASTP_GPU_E_INVALID, "counter block size mismatch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());  // submits may have used a caller-provided stream
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_ctr, (size_t)n * 8, hipMemcpyDeviceToHost));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_counters_export(fastp_gpu_ctx* ctx, int64_t* dst_device, int64_t n) {
    if (!ctx || !dst_device || n != ctx->cl.total) return fail(ctx, FASTP_GPU_E_INVALID, "counter block size mismatch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(dst_device, ctx->d_ctr, (size_t)n * 8, hipMemcpyDeviceToDevice));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_counters_import(fastp_gpu_ctx* ctx, const int64_t* src_device, int64_t n) {
    if (!ctx || !src_device || n != ctx->cl.total) return fail(ctx, FASTP_GPU_E_INVALID, "counter block size mismatch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(ctx->d_ctr, src_device, (size_t)n * 8, hipMemcpyDeviceToDevice));
    const int64_t hdr[4] = {FASTP_GPU_ABI_VERSION, ctx->cl.cycles, ctx->dp.isize_max, 0};
    HIP_TRY(ctx, hipMemcpy(ctx->d_ctr, hdr, sizeof(hdr), hipMemcpyHostToDevice));
    return FASTP_GPU_OK;
}

// Bring the HIP runtime up on `device` (context creation, the library's code object) without creating an engine: a
// host program calls it from a helper thread as early as it knows a GPU run is coming, so that the ~0.2 s this takes
// overlap its own start-up (option parsing, the Evaluator pre-pass) instead of preceding the first batch.
extern "C" int fastp_gpu_warmup(int device) {
    int n = 0;
    fq::timeline("warmup: begin");
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return fail(nullptr, FASTP_GPU_E_NO_DEVICE, "no such HIP device");
    fq::timeline("warmup: hipGetDeviceCount (the runtime is up)");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, FASTP_GPU_E_HIP, "hipSetDevice failed");
    void* p = nullptr;
    if (hipMalloc(&p, 256) != hipSuccess) return fail(nullptr, FASTP_GPU_E_HIP, "hipMalloc failed");
    fq::timeline("warmup: first hipMalloc (the device's context)");
    (void)hipFuncSetAttribute((const void*)fq_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 0);   // looks the kernel up: loads the code object
    fq::timeline("warmup: code object loaded");
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    (void)hipFree(p);
    fq::timeline("warmup: end");
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_device(const fastp_gpu_ctx* ctx) { return ctx ? ctx->device : -1; }
extern "C" int fastp_gpu_plan(const fastp_gpu_ctx* ctx) {
    if (!ctx) return -1;
    return ctx->lane ? FASTP_GPU_PLAN_LANE : (ctx->split ? FASTP_GPU_PLAN_SPLIT : FASTP_GPU_PLAN_FUSED);
}

extern "C" int fastp_gpu_reset(fastp_gpu_ctx* ctx) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());  // submits may have used a caller-provided stream
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctr, 0, (size_t)ctx->cl.total * 8, ctx->stream));
    const int64_t hdr[4] = {FASTP_GPU_ABI_VERSION, ctx->cl.cycles, ctx->dp.isize_max, 0};
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ctr, hdr, sizeof(hdr), hipMemcpyHostToDevice, ctx->stream));
    if (ctx->d_bitmap)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_bitmap, 0, (size_t)(ctx->dp.dup_bits >> 3) * ctx->dp.dup_bufnum, ctx->stream));
    if (ctx->d_post_seen) HIP_TRY(ctx, hipMemsetAsync(ctx->d_post_seen, 0, sizeof(u64), ctx->stream));
    ctx->units_seen = 0;
    ctx->has_prefix = false;
    for (int w = 0; w < 2; w++) {   // fresh FilterResult: both adapter maps empty
        int rc = cs_clear_map(ctx, w);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return FASTP_GPU_OK;
}

extern "C" int fastp_gpu_kernel_time(fastp_gpu_ctx* ctx, double* total_ms, int64_t* launches) {
    if (!ctx) return FASTP_GPU_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drain_events(ctx);
    if (total_ms) *total_ms = ctx->kernel_ms;
    if (launches) *launches = ctx->kernel_launches;
    ctx->kernel_ms = 0.0;
    ctx->kernel_launches = 0;
    return FASTP_GPU_OK;
}
