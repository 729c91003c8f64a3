// The host submits through the C ABI, for a sanitizer run of the HOST code (tests/hostsim/host_submit_check.sh builds this
// file, the product sources and the emulator into one program with -fsanitize=address,undefined and runs it).  Cases 1, 3, 4
// and 5 of tests/test_host_submit.py: async equals sync with three batches in flight, the slot contract, a slot's staging
// growing, and a refused submit leaving the engine usable.  Exit status 0 and no sanitizer report = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastp_gpu.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, fastp_gpu_last_error(nullptr)); \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

// the emulator keeps its coroutine stacks in a pool for the life of the process (sim.cpp, sim::launch): not a leak of the host code
extern "C" const char* __lsan_default_suppressions() { return "leak:sim::launch\n"; }

static const int L = 150;
static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

// n pairs from fragments of 100..300 bases: read 2 is the reverse complement of the fragment's end, a few bases differ
struct Reads {
    int n;
    size_t ss, qs;
    std::vector<uint8_t> seq[2], qual[2];
    std::vector<uint16_t> len[2];
    Reads(int n_, int correction) : n(n_), ss(fastp_gpu_seq_stride(L)), qs(fastp_gpu_qual_stride(L)) {
        std::vector<std::string> s[2], q[2];
        for (int i = 0; i < n; i++) {
            const int frag = 100 + (int)(rnd() % 200), len_i = frag < L ? frag : L;
            std::string f(frag, 'A');
            for (char& c : f) c = "ACGT"[rnd() & 3];
            std::string r1 = f.substr(0, len_i), r2(len_i, 'A');
            for (int k = 0; k < len_i; k++) {
                const char c = f[frag - 1 - k];
                r2[k] = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
            }
            std::string q1(len_i, 'I'), q2(len_i, 'I');
            if (correction && (rnd() & 1)) { const int k = (int)(rnd() % len_i); r2[k] = r2[k] == 'A' ? 'C' : 'A'; q2[k] = '#'; }
            s[0].push_back(r1); s[1].push_back(r2); q[0].push_back(q1); q[1].push_back(q2);
        }
        for (int m = 0; m < 2; m++) {
            std::vector<const char*> sp(n), qp(n);
            std::vector<int32_t> ln(n);
            for (int i = 0; i < n; i++) { sp[i] = s[m][i].data(); qp[i] = q[m][i].data(); ln[i] = (int32_t)s[m][i].size(); }
            seq[m].assign(n * ss, 0); qual[m].assign(n * qs, 0); len[m].assign(n, 0);
            int32_t bad = -1;
            CHECK(fastp_gpu_pack_reads(L, n, sp.data(), qp.data(), ln.data(), seq[m].data(), qual[m].data(), len[m].data(), &bad) == 0);
        }
    }
};

// a batch and its result block, in page-locked memory (the engine's allocator) or on the heap
struct Staged {
    fastp_gpu_ctx* ctx;
    bool pinned;
    std::vector<void*> mem;
    fastp_gpu_batch b;
    fastp_gpu_results res;
    int32_t ncorr = -1;
    int n, cap;
    void* get(size_t bytes, const void* src = nullptr) {
        void* p = nullptr;
        if (pinned) CHECK(fastp_gpu_host_alloc(ctx, (int64_t)bytes, &p) == 0);
        else p = malloc(bytes ? bytes : 1);
        mem.push_back(p);
        if (src) memcpy(p, src, bytes); else memset(p, 0, bytes);
        return p;
    }
    Staged(fastp_gpu_ctx* c, const Reads& r, int lo, int n_, bool pin) : ctx(c), pinned(pin), n(n_), cap(n_ * 32 + 64) {
        memset(&b, 0, sizeof(b));
        memset(&res, 0, sizeof(res));
        b.n = n;
        b.flags = FASTP_GPU_BATCH_STAT_ISIZE;
        b.seq1 = (const uint8_t*)get(n * r.ss, r.seq[0].data() + lo * r.ss);
        b.qual1 = (const uint8_t*)get(n * r.qs, r.qual[0].data() + lo * r.qs);
        b.len1 = (const uint16_t*)get(n * 2, r.len[0].data() + lo);
        b.seq2 = (const uint8_t*)get(n * r.ss, r.seq[1].data() + lo * r.ss);
        b.qual2 = (const uint8_t*)get(n * r.qs, r.qual[1].data() + lo * r.qs);
        b.len2 = (const uint16_t*)get(n * 2, r.len[1].data() + lo);
        res.r1 = (fastp_gpu_read_result*)get(n * sizeof(fastp_gpu_read_result));
        res.r2 = (fastp_gpu_read_result*)get(n * sizeof(fastp_gpu_read_result));
        res.pair = (fastp_gpu_pair_result*)get(n * sizeof(fastp_gpu_pair_result));
        res.corrections = (fastp_gpu_correction*)get(cap * sizeof(fastp_gpu_correction));
        res.corrections_capacity = cap;
        res.n_corrections = &ncorr;
    }
    ~Staged() {
        for (void* p : mem) {
            if (pinned) CHECK(fastp_gpu_host_free(ctx, p) == 0);
            else free(p);
        }
    }
};

static uint64_t corr_key(const fastp_gpu_correction& c) { return ((uint64_t)c.read << 32) | ((uint64_t)c.pos << 16) | ((uint64_t)c.base << 8) | c.qual; }
static void same(const Staged& a, const Staged& b) {
    CHECK(a.n == b.n && a.ncorr == b.ncorr && a.ncorr >= 0);
    CHECK(!memcmp(a.res.r1, b.res.r1, a.n * sizeof(fastp_gpu_read_result)));
    CHECK(!memcmp(a.res.r2, b.res.r2, a.n * sizeof(fastp_gpu_read_result)));
    CHECK(!memcmp(a.res.pair, b.res.pair, a.n * sizeof(fastp_gpu_pair_result)));
    uint64_t sa = 0, sb = 0, xa = 0, xb = 0;   // the lists are unordered: compare them as multisets (sum and xor of the entries)
    for (int k = 0; k < a.ncorr; k++) {
        sa += corr_key(a.res.corrections[k]); xa ^= corr_key(a.res.corrections[k]);
        sb += corr_key(b.res.corrections[k]); xb ^= corr_key(b.res.corrections[k]);
    }
    CHECK(sa == sb && xa == xb);
}

static std::vector<int64_t> counters(fastp_gpu_ctx* ctx, const fastp_gpu_params& p) {
    fastp_gpu_counter_layout lay;
    fastp_gpu_counter_layout_for_params(&p, &lay);
    std::vector<int64_t> out((size_t)lay.total);
    CHECK(fastp_gpu_counters(ctx, out.data(), lay.total) == 0);
    return out;
}

int main() {
    for (int correction = 0; correction < 2; correction++) {
        fastp_gpu_params p;
        fastp_gpu_default_params(&p, 1, L);
        p.correction = correction;
        fastp_gpu_ctx *a = nullptr, *b = nullptr;
        CHECK(fastp_gpu_create(&p, 0, &a) == 0 && fastp_gpu_create(&p, 0, &b) == 0);
        const Reads r(300 + 129 + 1 + 1 + 300 + 129, correction);
        int lo = 0, total_corr = 0;
        {   // 1: three batches in flight against three synchronous submits
            const int sizes[3] = {300, 129, 1};
            Staged* sy[3];
            Staged* as[3];
            for (int k = 0; k < 3; lo += sizes[k++]) {
                sy[k] = new Staged(a, r, lo, sizes[k], false);
                as[k] = new Staged(b, r, lo, sizes[k], true);
                CHECK(fastp_gpu_submit_host(a, &sy[k]->b, &sy[k]->res) == 0);
                CHECK(fastp_gpu_submit_host_async(b, &as[k]->b, &as[k]->res, k) == 0);
            }
            for (int k = 0; k < 3; k++) CHECK(fastp_gpu_wait(b, k) == 0);
            for (int k = 0; k < 3; k++) { same(*sy[k], *as[k]); total_corr += sy[k]->ncorr; delete sy[k]; delete as[k]; }
        }
        CHECK(correction ? total_corr > 0 : total_corr == 0);
        {   // 4: a batch of 1, then one of 300 on the same slot
            const int sizes[2] = {1, 300};
            for (int k = 0; k < 2; lo += sizes[k++]) {
                Staged sy(a, r, lo, sizes[k], false), as(b, r, lo, sizes[k], true);
                CHECK(fastp_gpu_submit_host(a, &sy.b, &sy.res) == 0);
                CHECK(fastp_gpu_submit_host_async(b, &as.b, &as.res, 1) == 0 && fastp_gpu_wait(b, 1) == 0);
                same(sy, as);
            }
        }
        {   // 3 and 5: the slot contract, refused submits, and the engine afterwards
            Staged sy(a, r, lo, 129, false), as(b, r, lo, 129, true), late(b, r, lo, 129, true), empty(b, r, lo, 0, true);
            const int bad_slots[3] = {-1, FASTP_GPU_ASYNC_SLOTS, FASTP_GPU_ASYNC_SLOTS + 1};
            for (int s : bad_slots)
                CHECK(fastp_gpu_submit_host_async(b, &late.b, &late.res, s) == FASTP_GPU_E_INVALID &&
                      fastp_gpu_wait(b, s) == FASTP_GPU_E_INVALID && fastp_gpu_poll(b, s) == FASTP_GPU_E_INVALID);
            for (int s = 0; s < FASTP_GPU_ASYNC_SLOTS; s++) CHECK(fastp_gpu_poll(b, s) == 1 && fastp_gpu_wait(b, s) == 0);
            CHECK(fastp_gpu_submit_host_async(b, &empty.b, &empty.res, 0) == FASTP_GPU_E_INVALID);
            CHECK(fastp_gpu_submit_host(b, &empty.b, &empty.res) == 0 && empty.ncorr == 0);
            const uint8_t* seq2 = late.b.seq2;
            late.b.seq2 = nullptr;
            CHECK(fastp_gpu_submit_host_async(b, &late.b, &late.res, 2) == FASTP_GPU_E_INVALID);
            CHECK(fastp_gpu_submit_host(b, &late.b, &late.res) == FASTP_GPU_E_INVALID);
            late.b.seq2 = seq2;
            CHECK(fastp_gpu_submit_host(a, &sy.b, &sy.res) == 0);
            CHECK(fastp_gpu_submit_host_async(b, &as.b, &as.res, 2) == 0);
            CHECK(fastp_gpu_submit_host_async(b, &late.b, &late.res, 2) == FASTP_GPU_E_INVALID);   // busy
            int arrived = 0;
            while (!arrived) arrived = fastp_gpu_poll(b, 2);
            CHECK(arrived == 1 && fastp_gpu_poll(b, 2) == 1);
            same(sy, as);
        }
        CHECK(counters(a, p) == counters(b, p));
        fastp_gpu_destroy(a);
        fastp_gpu_destroy(b);
    }
    printf("host submits: clean\n");
    return 0;
}
