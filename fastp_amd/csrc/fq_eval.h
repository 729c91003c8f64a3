// fq_eval.h - the Evaluator pre-pass on the device: the loops of
// /root/reference/src/evaluator.cpp that run over a prefix of the input before any worker starts -
//   * the 4^10 ten-mer histogram of evalAdapterAndReadNum (evaluator.cpp:377-399),
//   * the substring census of computeOverRepSeq (evaluator.cpp:78-142): every substring of 5 lengths of the
//     first 1.51 Mbases, counted exactly (the reference keeps a std::map<string,long>),
//   * the loop of checkKnownAdapters (evaluator.cpp:242-289): every known adapter at every position of up to 100,000 reads, and
//   * the scans and tree walks of getAdapterWithSeed (evaluator.cpp:485-520) for one seed of the histogram.
// All read the packed rows a batch already holds in HBM (2-bit bases + the N flag in the quality byte).  What the Evaluator
// decides from the numbers stays on the host.
// A read with a letter outside ACGTN (soft-masked lower case, IUPAC codes, '.') is stored there with code 0 for that letter,
// so the text-aware forms (<true>, *_x_body; the fastp_gpu_eval_*_x entry points) take the bytes of the reads the caller
// lists from the FASTQ text instead - EvalText below has what the reference does with such a byte in each loop.
#pragma once
#include "fq_intrin.h"
#include "fq_types.h"

namespace fq {

struct EvalReads {
    const u8* seq;
    const u8* qual;
    const u16* len;
    int n;               // reads the limits of the reference loop admit (computed by the host from `len`)
    int seq_stride, qual_stride;
};

FQ_DEV u32 eval_base(const u8* s, const u8* q, int j) {   // 0..3 = A T C G, 4 = N
    return (q[j] & 0x80u) ? 4u : (u32)((s[j >> 2] >> (2 * (j & 3))) & 3u);
}

// ---- reads with letters outside ACGTN ------------------------------------------------------------------------
// The listed reads' symbols come from the text, every other read's from its packed row.  What a byte b outside ACGTN does:
//   seq2int (evaluator.cpp:577-626), histogram and hit search: a window holding anything but A T C G gives -1 - b acts as N
//   checkKnownAdapters (:266-287): a raw != against the adapter's letter - a mismatch inside the cmplen / 16 allowance
//   NucleotideTree::addSeq (nucleotidetree.cpp:42-55): only the byte 'N' cuts; b descends into child b & 7 (a / A share
//     bin 1, n goes to bin 6 and goes on), and a node prints the byte of the sequence that created it (reads, then
//     positions, ascending); getDominantPath (:57-88) sums and tests all eight children
//   computeOverRepSeq (:99-160): raw substrings in a std::map - b equals only the same byte
// rawoff is built once per call from the ascending list (eval_list_body): a word per read, no search per position.
enum : u32 { EVAL_UNLISTED = 0xFFFFFFFFu };
struct EvalText {
    const u8* text;
    const u32* rawoff;   // [n] byte offset of the read's sequence in text, EVAL_UNLISTED: the packed row is the read
};
struct EvalListArgs {
    const int* unit;     // [n_exotic] ascending read indexes
    int n_exotic, dense;
    const u32* off;      // dense: the parser's line_off table ([4 * read + 1]); else an offset per listed read
    u32* rawoff;         // [n], preset to EVAL_UNLISTED
};
FQ_DEV void eval_list_body(const EvalListArgs& a) {
    const int k = block_id() * block_threads() + thread_id();
    if (k >= a.n_exotic) return;
    const int u = a.unit[k];
    a.rawoff[u] = a.dense ? a.off[4 * (size_t)u + 1] : a.off[k];
}
FQ_DEV const u8* eval_raw(const EvalText& x, int rd) {   // the listed read's bytes, or null
    const u32 o = x.rawoff[rd];
    return o == EVAL_UNLISTED ? nullptr : x.text + o;
}
FQ_DEV u32 eval_byte(const u8* raw, const u8* s, const u8* q, int j) { return raw ? (u32)raw[j] : (u32)"ATCGN"[eval_base(s, q, j)]; }
// the accessor: the raw byte of read rd at position j
FQ_DEV u32 eval_byte(const EvalReads& r, const EvalText& x, int rd, int j) {
    return eval_byte(eval_raw(x, rd), r.seq + (size_t)rd * r.seq_stride, r.qual + (size_t)rd * r.qual_stride, j);
}
// a census symbol: the packed form compares codes (0..4), the text-aware form bytes - of listed and unlisted reads alike,
// so an all-ACGTN window hashes and compares the same whichever kind of read it came from
template <bool X> FQ_DEV u32 eval_sym(const u8* raw, const u8* s, const u8* q, int j) {
    if constexpr (X) return eval_byte(raw, s, q, j);
    else return eval_base(s, q, j);
}

// ---- ten-mer histogram --------------------------------------------------------------------------------------
// Evaluator::seq2int (evaluator.cpp:573-625) is a pure function of the window: the rolling update and the
// from-scratch computation give the same key, and a window holding a non-ACGT base gives -1 either way.
// key = first base in the most significant pair; rows hold base j in bits [2(j%4), 2(j%4)+1] of byte j/4.
struct EvalKmerArgs {
    EvalReads r;
    int shift_tail;      // max(1, trim_tail1)
    int span;            // positions per read one row of lanes covers (max_len rounded up)
    u32* counts;         // [1 << 20]
};

FQ_DEV u32 eval_reverse_pairs20(u32 v) {   // 10 two-bit groups, first group to the top
    u32 x = brev32(v);                     // bit i -> 31 - i : groups reversed, bits inside a group swapped
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    return x >> 12;
}

// Evaluator::seq2int for the window at `pos` of read rd: the key, or -1.  A listed read's window is read letter by letter
// (anything but A T C G: -1); an unlisted read's packed row holds it exactly.
template <bool X> FQ_DEV int eval_window_key(const EvalReads& r, const EvalText& x, int rd, int pos) {
    if constexpr (X) {
        const u8* raw = eval_raw(x, rd);
        if (raw) {
            u32 key = 0;
            for (int k = 0; k < 10; k++) {
                const u8 b = raw[pos + k];
                const u32 c = b == 'A' ? 0u : b == 'T' ? 1u : b == 'C' ? 2u : b == 'G' ? 3u : 4u;
                if (c > 3u) return -1;
                key = (key << 2) | c;
            }
            return (int)key;
        }
    }
    const u8* s = r.seq + (size_t)rd * r.seq_stride;
    const u8* q = r.qual + (size_t)rd * r.qual_stride;
    u32 nflag = 0;
    for (int k = 0; k < 10; k++) nflag |= q[pos + k];
    if (nflag & 0x80u) return -1;   // an N in the window
    // 20 bits starting at base `pos`: bytes pos/4 .. (pos + 9)/4 hold them (3 or 4 bytes)
    const int b = pos >> 2, nb = ((pos + 9) >> 2) - b;
    u32 w = 0;
    for (int k = 0; k <= nb; k++) w |= (u32)s[b + k] << (8 * k);
    return (int)eval_reverse_pairs20((w >> (2 * (pos & 3))) & 0xFFFFFu);
}

template <bool X> FQ_DEV void eval_kmer_body(const EvalKmerArgs& a, const EvalText& x) {
    const long long t = (long long)block_id() * block_threads() + thread_id();
    const int rd = (int)(t / a.span), pos = 20 + (int)(t % a.span);
    if (rd >= a.r.n) return;
    const int rlen = a.r.len[rd];
    if (pos > rlen - 10 - a.shift_tail) return;
    const int key = eval_window_key<X>(a.r, x, rd, pos);
    if (key > 0) g_atomic_add_u32(&a.counts[key], 1u);            // "set AAAAAAAAAA = 0" (evaluator.cpp:401-402)
}

// ---- substring census ---------------------------------------------------------------------------------------
// An exact multiset count without strings: an open-addressing table whose slot names ONE occurrence of its
// substring (the representative); a later occurrence that hashes there is compared base by base with the
// representative's text and either counts or moves on to the next slot.
//   slot word: (read + 1) << 40 | pos << 24 | step index << 21 | 21 hash bits        0 = empty
enum { EVAL_STEPS = 5 };
struct EvalCensusArgs {
    EvalReads r;
    int span;
    int step[EVAL_STEPS];      // 10, 20, 40, 100, min(150, seqlen - 2); <= 0: skipped
    u64* slot;                 // [cap]
    u32* count;                // [cap]
    u32 mask;                  // cap - 1
    // harvest
    int seqlen;
    u64* hot;                  // [hot_cap] slot words of the substrings over their threshold
    u32* hot_count;            // [hot_cap]
    u32* n_hot;                // [1]
    u32 hot_cap;
    // text
    u8* text;                  // [hot_cap * 152] a row of characters per hot substring
};

template <bool X> FQ_DEV void eval_census_body(const EvalCensusArgs& a, const EvalText& x) {
    const long long t = (long long)block_id() * block_threads() + thread_id();
    const int rd = (int)(t / a.span), pos = (int)(t % a.span);
    if (rd >= a.r.n) return;
    const int rlen = a.r.len[rd];
    const u8* s = a.r.seq + (size_t)rd * a.r.seq_stride;
    const u8* q = a.r.qual + (size_t)rd * a.r.qual_stride;
    const u8* raw = X ? eval_raw(x, rd) : nullptr;
    u64 h = 0x9E3779B97F4A7C15ull;
    int done = 0;
    // the steps grow (the last one may be smaller than the others: hash restarted then)
    for (int si = 0; si < EVAL_STEPS; si++) {
        const int step = a.step[si];
        if (step <= 0 || pos >= rlen - step) continue;   // for(i = 0; i < rlen - step; i++)
        if (step < done) { h = 0x9E3779B97F4A7C15ull; done = 0; }
        for (; done < step; done++) h = (h ^ (u64)(eval_sym<X>(raw, s, q, pos + done) + 1u)) * 0x100000001B3ull;
        u64 hs = (h ^ (u64)step) * 0xD6E8FEB86659FD93ull;
        hs ^= hs >> 32;
        const u64 mine = ((u64)(rd + 1) << 40) | ((u64)pos << 24) | ((u64)si << 21) | (hs & 0x1FFFFFull);
        u32 at = (u32)(hs >> 21) & a.mask;
        for (;;) {
            u64 cur = __hip_atomic_load(&a.slot[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0ull) {
                cur = g_atomic_cas_u64(&a.slot[at], 0ull, mine);
                if (cur == 0ull) {
                    g_atomic_add_u32(&a.count[at], 1u);
                    break;
                }
            }
            if (((cur ^ mine) & 0x1FFFFFull) == 0ull) {
                // same hash bits: same length and same text?
                const int rd2 = (int)(cur >> 40) - 1, pos2 = (int)((cur >> 24) & 0xFFFFu);
                const int step2 = a.step[(cur >> 21) & 7u];
                bool same = step2 == step;
                if (same && !(rd2 == rd && pos2 == pos)) {
                    const u8* s2 = a.r.seq + (size_t)rd2 * a.r.seq_stride;
                    const u8* q2 = a.r.qual + (size_t)rd2 * a.r.qual_stride;
                    const u8* raw2 = X ? eval_raw(x, rd2) : nullptr;
                    for (int k = 0; k < step; k++)
                        if (eval_sym<X>(raw, s, q, pos + k) != eval_sym<X>(raw2, s2, q2, pos2 + k)) {
                            same = false;
                            break;
                        }
                }
                if (same) {
                    g_atomic_add_u32(&a.count[at], 1u);
                    break;
                }
            }
            at = (at + 1u) & a.mask;
        }
    }
}

// thresholds of evaluator.cpp:115-137
FQ_DEV bool eval_is_hot(int len, u32 count, int seqlen) {
    if (len >= seqlen - 1) return count >= 3u;
    if (len >= 100) return count >= 5u;
    if (len >= 40) return count >= 20u;
    if (len >= 20) return count >= 100u;
    if (len >= 10) return count >= 500u;
    return false;
}

FQ_DEV void eval_harvest_body(const EvalCensusArgs& a) {
    const u32 at = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    if (at > a.mask) return;
    const u64 w = a.slot[at];
    if (w == 0ull) return;
    const u32 c = a.count[at];
    if (!eval_is_hot(a.step[(w >> 21) & 7u], c, a.seqlen)) return;
    const u32 k = g_atomic_add_u32(a.n_hot, 1u);
    if (k < a.hot_cap) {
        a.hot[k] = w;
        a.hot_count[k] = c;
    }
}

template <bool X> FQ_DEV void eval_text_body(const EvalCensusArgs& a, const EvalText& x) {
    // 16 lanes per hot substring
    const u32 t = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    const u32 k = t >> 4, gl = t & 15u;
    const u32 n = *a.n_hot < a.hot_cap ? *a.n_hot : a.hot_cap;
    if (k >= n) return;
    const u64 w = a.hot[k];
    const int rd = (int)(w >> 40) - 1, pos = (int)((w >> 24) & 0xFFFFu), step = a.step[(w >> 21) & 7u];
    const u8* s = a.r.seq + (size_t)rd * a.r.seq_stride;
    const u8* q = a.r.qual + (size_t)rd * a.r.qual_stride;
    u8* o = a.text + (size_t)k * 152;
    const u8* raw = X ? eval_raw(x, rd) : nullptr;
    for (int j = (int)gl; j < step; j += 16) o[j] = (u8)eval_byte(raw, s, q, pos + j);
}

// ---- known-adapter check (Evaluator::checkKnownAdapters, evaluator.cpp:220-306) -----------------------------
// Two steps whose composition is the reference's sequential loop.  The inner loop (:266-287) - the first position of
// a read at which an adapter fits with at most cmplen / 16 mismatches - does not depend on the loop's running state,
// so eval_match_body computes it for every (read, adapter); eval_replay_body then walks the matched pairs in read
// order and in std::map order inside a read, with the pruning rule (:263) and the exits (:252-255) of the loop.
// Adapters are given sorted (map order) as 2-bit words, 32 bases to a u64, base i in bits [2(i%32), 2(i%32)+1].
enum { EVAL_AD_WORDS = 8,        // 256 bases = FASTP_GPU_MAX_ADAPTER_LEN
       EVAL_MATCH_WAVES = 4,     // reads (wavefronts) per workgroup of the match kernel
       EVAL_MATCH_LDS = 48 + 48 + 32,   // dwords per wavefront: bases | N mask | matched bitset, then a dword per adapter
       EVAL_MAX_ADAPTERS = 1024,
       EVAL_CHECK_READS = 100000 };      // MAX_CHECK_READS (:226)
struct EvalMatchArgs {
    EvalReads r;             // r.n: the reads the check can reach (at most EVAL_CHECK_READS)
    const u64* words;        // [n_adapters][ad_words]
    const u16* alen;         // [n_adapters]
    int n_adapters, ad_words, bit_words;   // bit_words = ceil(n_adapters / 32)
    u32* bits;               // [n][bit_words]  bit a: adapter a matched the read
    u8* mm;                  // [n][n_adapters] its mismatches (written for matched pairs only)
    // replay
    int n_all;               // reads the caller has (the loop's `num`)
    int* counts;             // [n_adapters] possibleCounts | [n_adapters] mismatches
    long long* checked;      // [1] checkedReads
};

FQ_DEV u64 eval_pairs_mask(int c) {   // the low bit of each of the first c (0..32) base pairs
    return c >= 32 ? 0x5555555555555555ull : (((1ull << (2 * (c < 0 ? 0 : c))) - 1ull) & 0x5555555555555555ull);
}

// A wavefront per read, a lane per position, 64 positions to a tile, tiles in ascending order.  The read is staged once in
// LDS as 2-bit words and an N mask; a lane funnel-shifts its window out of them into registers, one u64 per 32 bases, and
// keeps it for all adapters, which arrive as wave-uniform words.  A lane whose position fits says so with an LDS minimum on
// pos << 8 | mismatches: the smallest position wins and brings its own count.  Fits are rare, so almost no lane gets there.
FQ_DEV void eval_match_body(const EvalMatchArgs& a, u32* lds) {
    const int lane = lane_id(), rd = block_id() * EVAL_MATCH_WAVES + wave_id();
    if (rd >= a.r.n) return;
    u32* sq = lds + wave_id() * (EVAL_MATCH_LDS + a.bit_words * 32);   // 32 dwords of bases (512) + 16 of zeros: a window may start at 503
    u32* nm = sq + 48;                            // the N flags spread to the low bit of each base's pair
    u32* done = nm + 48;                          // [32] adapters that fitted in the tiles so far
    u32* first = done + 32;                       // [bit_words * 32] pos << 8 | mismatches of the first fit, ~0: none
    const int rlen = a.r.len[rd] < 512 ? a.r.len[rd] : 512;   // (FASTP_GPU_MAX_READ_LEN: what the stage holds)
    const u8* s = a.r.seq + (size_t)rd * a.r.seq_stride;
    const u8* q = a.r.qual + (size_t)rd * a.r.qual_stride;
    if (lane < 48) {   // dword `lane`: bases 16 * lane .. + 15
        u32 w = 0, m = 0;
        if (16 * lane < rlen) {
            for (int k = 0; k < 4; k++)
                if (4 * lane + k < a.r.seq_stride) w |= (u32)s[4 * lane + k] << (8 * k);
            for (int k = 0; k < 16; k++)
                if (16 * lane + k < rlen) m |= (u32)(q[16 * lane + k] >> 7) << (2 * k);
        }
        sq[lane] = w;
        nm[lane] = m;
    }
    if (lane < 32) done[lane] = 0u;
    for (int k = lane; k < a.bit_words * 32; k += 64) first[k] = 0xFFFFFFFFu;
    wave_sync();
    const int npos = rlen - 8;   // for(pos = 0; pos < rlen - matchReq; pos++)
    u32* bits = a.bits + (size_t)rd * a.bit_words;
    if (npos <= 0) {
        if (lane < a.bit_words) bits[lane] = 0u;
        return;
    }
    if (lane >= npos && lane >= a.bit_words) return;    // a lane without a position in any tile and without a word to fold
    for (int tile = 0; tile * 64 < npos; tile++) {
        const int pos = tile * 64 + lane;
        const bool has_pos = pos < npos;
        // the read from `pos` on, as the adapters are laid out; bases past its end take no part in any comparison
        u64 R[EVAL_AD_WORDS], V[EVAL_AD_WORDS], N[EVAL_AD_WORDS];
        const u32 sh = 2u * (u32)(pos & 15);
#pragma unroll
        for (int w = 0; w < EVAL_AD_WORDS; w++) {
            R[w] = V[w] = N[w] = 0ull;
            if (w < a.ad_words && has_pos) {
                const int i0 = (pos >> 4) + 2 * w;   // <= 31 + 14, + 2 < 48
                R[w] = (u64)alignbit(sq[i0 + 1], sq[i0], sh) | ((u64)alignbit(sq[i0 + 2], sq[i0 + 1], sh) << 32);
                V[w] = eval_pairs_mask(rlen - pos - 32 * w);
                N[w] = ((u64)alignbit(nm[i0 + 1], nm[i0], sh) | ((u64)alignbit(nm[i0 + 2], nm[i0 + 1], sh) << 32)) & V[w];
            }
        }
        if (has_pos)
            for (int g = 0; g < a.bit_words; g++) {
                const u32 dn = tile ? done[g] : 0u;
                for (int j = 0; j < 32; j++) {
                    const int ad = g * 32 + j;
                    if (ad >= a.n_adapters) break;
                    if ((dn >> j) & 1u) continue;        // its first position lies in an earlier tile
                    const int alen = (int)a.alen[ad];
                    if (alen >= rlen) continue;          // :260
                    const int nw = (alen + 31) >> 5;
                    const u64* aw = a.words + (size_t)ad * a.ad_words;
                    int mism = 0;
#pragma unroll
                    for (int w = 0; w < EVAL_AD_WORDS; w++)
                        if (w < nw) {
                            const u64 x = R[w] ^ aw[w];
                            // a differing base or an N, inside the read and inside the adapter
                            mism += popc64((((x | (x >> 1)) & V[w]) | N[w]) & eval_pairs_mask(alen - 32 * w));
                        }
                    const int cmplen = rlen - pos < alen ? rlen - pos : alen;
                    if (mism <= (cmplen >> 4)) lds_min_u32(&first[ad], ((u32)pos << 8) | (u32)mism);   // mism <= 256 / 16
                }
            }
        wave_sync();
        if (lane < a.bit_words) {
            u32 dn = 0u;
            for (int j = 0; j < 32; j++) dn |= (u32)(first[lane * 32 + j] != 0xFFFFFFFFu) << j;
            done[lane] = dn;
        }
        wave_sync();
    }
    if (lane < a.bit_words) {
        bits[lane] = done[lane];
        u8* mm = a.mm + (size_t)rd * a.n_adapters;
        for (int ad = lane * 32; ad < lane * 32 + 32 && ad < a.n_adapters; ad++)
            if (first[ad] != 0xFFFFFFFFu) mm[ad] = (u8)first[ad];
    }
}

// The text-aware form.  An unlisted read's packed row is exact, so its wavefront runs the body above; a listed read's
// bytes are staged in LDS behind the packed stages of all wavefronts (128 dwords each: 512 bytes) and every lane runs
// the reference's inner loop (:269-279) on them as it is written: a raw != against the adapter's letter, left once the
// allowance is exceeded.  `first` is the wavefront's own of the packed layout, and the results have the same form.
FQ_DEV void eval_match_x_body(const EvalMatchArgs& a, const EvalText& x, u32* lds) {
    const int lane = lane_id(), rd = block_id() * EVAL_MATCH_WAVES + wave_id();
    if (rd >= a.r.n) return;
    const u8* raw = eval_raw(x, rd);
    if (!raw) {
        eval_match_body(a, lds);
        return;
    }
    u32* first = lds + wave_id() * (EVAL_MATCH_LDS + a.bit_words * 32) + EVAL_MATCH_LDS;
    u8* rb = (u8*)(lds + EVAL_MATCH_WAVES * (EVAL_MATCH_LDS + a.bit_words * 32) + wave_id() * 128);
    const int rlen = a.r.len[rd] < 512 ? a.r.len[rd] : 512;
    for (int i = lane; i < rlen; i += 64) rb[i] = raw[i];
    for (int k = lane; k < a.bit_words * 32; k += 64) first[k] = 0xFFFFFFFFu;
    wave_sync();
    const int npos = rlen - 8;
    u32* bits = a.bits + (size_t)rd * a.bit_words;
    if (npos <= 0) {
        if (lane < a.bit_words) bits[lane] = 0u;
        return;
    }
    for (int pos = lane; pos < npos; pos += 64)
        for (int ad = 0; ad < a.n_adapters; ad++) {
            const int alen = (int)a.alen[ad];
            if (alen >= rlen) continue;          // :260
            const u64* aw = a.words + (size_t)ad * a.ad_words;
            const int cmplen = rlen - pos < alen ? rlen - pos : alen, allowed = cmplen >> 4;
            int mism = 0;
            u64 w = 0;
            for (int i = 0; i < cmplen && mism <= allowed; i++) {
                if ((i & 31) == 0) w = aw[i >> 5];
                mism += (u8)"ATCG"[(w >> (2 * (i & 31))) & 3u] != rb[pos + i];
            }
            if (mism <= allowed) lds_min_u32(&first[ad], ((u32)pos << 8) | (u32)mism);   // the smallest position wins
        }
    wave_sync();
    if (lane < a.bit_words) {
        u32 dn = 0u;
        for (int j = 0; j < 32; j++) dn |= (u32)(first[lane * 32 + j] != 0xFFFFFFFFu) << j;
        bits[lane] = dn;
        u8* mm = a.mm + (size_t)rd * a.n_adapters;
        for (int ad = lane * 32; ad < lane * 32 + 32 && ad < a.n_adapters; ad++)
            if (first[ad] != 0xFFFFFFFFu) mm[ad] = (u8)first[ad];
    }
}

// One wavefront.  Only matched pairs change the loop's state, so reads are taken 64 at a time (a lane each) and lane 0
// walks the set bits of the ones that matched something.  LDS: counts | mismatches.
// The exits: `checkedReads > 100000` is read index 100000; `checkedBases > 100000000` cannot bind before it while a
// read has at most FASTP_GPU_MAX_READ_LEN = 512 bases (100000 * 512 < 10^8) - kept, on a 64-bit sum, for the day that
// limit moves; `curMaxCount > 1000` is seen at the read after the one that raised it.
FQ_DEV void eval_replay_body(const EvalMatchArgs& a, u32* lds) {
    const int lane = lane_id(), A = a.n_adapters;
    int* cnt = (int*)lds;
    int* mis = cnt + A;
    for (int k = lane; k < 2 * A; k += 64) cnt[k] = 0;
    wave_sync();
    long long bases = 0, checked = a.n_all;
    int cur_max = 0;        // lane 0's
    for (int base = 0; base < a.n_all; base += 64) {
        const int i = base + lane;
        const bool ok = i < a.n_all;
        u32 cum = ok ? (u32)a.r.len[i] : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 o = shfl(cum, lane >= d ? lane - d : lane);
            if (lane >= d) cum += o;
        }
        const u64 over = ballot(ok && (i >= EVAL_CHECK_READS || bases + (long long)cum > 100000000ll));
        const int cut = over ? ffs64(over) - 1 : 64;   // the read at which the loop leaves: counted, not looked at
        bool any = false;
        if (ok && lane < cut)
            for (int g = 0; g < a.bit_words; g++) any |= a.bits[(size_t)i * a.bit_words + g] != 0u;
        u64 ev = ballot(any);
        bool stop = false;
        if (lane == 0) {
            while (ev) {
                const int e = ffs64(ev) - 1;
                ev &= ev - 1ull;
                const size_t rd = (size_t)(base + e);
                for (int g = 0; g < a.bit_words; g++) {
                    u32 w = a.bits[rd * a.bit_words + g];
                    while (w) {
                        const int ad = g * 32 + ffs32(w) - 1;
                        w &= w - 1u;
                        if (cur_max > 20 && cnt[ad] < cur_max / 10) continue;   // :263
                        const int c = ++cnt[ad];
                        if (cur_max < c) cur_max = c;
                        mis[ad] += (int)a.mm[rd * A + ad];
                    }
                }
                if (cur_max > 1000) {   // :254, at the next read if there is one
                    checked = (long long)rd + 2 < a.n_all ? (long long)rd + 2 : a.n_all;
                    stop = true;
                    break;
                }
            }
            if (!stop && over) {
                checked = base + cut + 1;
                stop = true;
            }
        }
        bases += (long long)shfl(cum, 63);
        if (ballot(stop)) break;
    }
    wave_sync();
    for (int k = lane; k < 2 * A; k += 64) a.counts[k] = cnt[k];
    if (lane == 0) *a.checked = checked;
}

// ---- seed extension (Evaluator::getAdapterWithSeed evaluator.cpp:485-520, NucleotideTree nucleotidetree.cpp:42-88) ----
// The two scans find the same (read, pos) hits; a tree's dominant path only needs, per depth, how many of the hits that
// followed the path so far carry each base there.  eval_seed_gather_body lists the hits (or counts them: hits == nullptr),
// eval_seed_walk_body walks both directions, one workgroup each, over its lanes' share of the list.
//   hit word: read << 9 | pos (pos < 500); bit 31 / 30: left the forward / backward path
struct EvalSeedArgs {
    EvalReads r;
    int shift_tail, span;
    u32 seed;
    u32* hits;               // [cap] or nullptr
    u64* n_hits;             // [1]
    u64 cap;
    // walk
    u8* path;                // [2][512] forward | backward
    int* path_len;           // [2], then [2] = 1 unless a walk ended without a dominant base
};

template <bool X> FQ_DEV void eval_seed_gather_body(const EvalSeedArgs& a, const EvalText& x) {
    const long long t = (long long)block_id() * block_threads() + thread_id();
    const int rd = (int)(t / a.span), pos = 20 + (int)(t % a.span);   // span <= 480: pos < MAX_SEARCH_LENGTH
    if (rd >= a.r.n) return;
    const int rlen = a.r.len[rd];
    if (pos > rlen - 10 - a.shift_tail) return;
    if (eval_window_key<X>(a.r, x, rd, pos) != (int)a.seed) return;
    const u64 k = __hip_atomic_fetch_add(a.n_hits, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.hits && k < a.cap) a.hits[k] = ((u32)rd << 9) | (u32)pos;
}

// the base (0..3) depth d of a hit's sequence holds, 4: the sequence has ended (its end, or an N: addSeq :45)
FQ_DEV u32 eval_seed_base(const EvalSeedArgs& a, u32 hit, int dir, int d) {
    const int rd = (int)((hit >> 9) & 0x1FFFFFu), pos = (int)(hit & 511u);
    int j;
    if (dir == 0) {
        j = pos + 10 + d;
        if (j >= (int)a.r.len[rd] - a.shift_tail) return 4u;
    } else {
        j = pos - 1 - d;
        if (j < 0) return 4u;
    }
    return eval_base(a.r.seq + (size_t)rd * a.r.seq_stride, a.r.qual + (size_t)rd * a.r.qual_stride, j);
}

FQ_DEV void eval_seed_walk_body(const EvalSeedArgs& a, u32* lds) {
    const int dir = block_id(), tid = thread_id(), T = block_threads();
    const u32 dead = dir == 0 ? 0x80000000u : 0x40000000u;
    const u64 nh = *a.n_hits < a.cap ? *a.n_hits : a.cap;
    u8* path = a.path + 512 * dir;
    int depth = 0;
    u32 last = 0;
    bool leaf = true;
    for (; depth < 512; depth++) {
        if (tid < 4) lds[tid] = 0u;
        block_sync();
        u32 c[4] = {0u, 0u, 0u, 0u};
        for (u64 k = (u64)tid; k < nh; k += (u64)T) {
            const u32 h = __hip_atomic_load(&a.hits[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (h & dead) continue;
            u32 b = 4u;
            if (depth == 0 || eval_seed_base(a, h, dir, depth - 1) == last) b = eval_seed_base(a, h, dir, depth);
            if (b > 3u) {
                g_atomic_or_u32(&a.hits[k], dead);   // (the other direction's workgroup owns the other bit of the word)
                continue;
            }
            c[0] += b == 0u; c[1] += b == 1u; c[2] += b == 2u; c[3] += b == 3u;
        }
        for (int b = 0; b < 4; b++)
            if (c[b]) lds_add_u32(&lds[b], c[b]);
        block_sync();
        const u32 n0 = lds[0], n1 = lds[1], n2 = lds[2], n3 = lds[3];
        block_sync();
        const u32 total = n0 + n1 + n2 + n3;
        if (total < 50u) break;                      // NUM_THRESHOLD
        // children[base & 7]: A, C, T, G; at most one base can hold 95 %
        const u32 n[4] = {n0, n1, n2, n3};
        const int order[4] = {0, 2, 1, 3};
        int pick = -1;
        for (int o = 0; o < 4 && pick < 0; o++)
            if ((double)n[order[o]] / (double)total >= 0.95) pick = order[o];
        if (pick < 0) {
            leaf = false;
            break;
        }
        last = (u32)pick;
        if (tid == 0) path[depth] = (u8)"ATCG"[pick];
    }
    if (tid == 0) {
        a.path_len[dir] = depth;
        if (!leaf) g_atomic_exch_u32((u32*)&a.path_len[2], 0u);
    }
}

// The text-aware walk: the tree as nucleotidetree.cpp builds it from raw bytes.  Eight bins by byte & 7, only the byte 'N'
// ends a sequence (addSeq :45-47), and the character a node prints is the byte of the sequence that created it (:48-51) -
// the lowest (read, pos) among the hits that reach it, which is the smallest hit word.  LDS: 8 counts | 8 smallest words.
// the byte depth d of a hit's sequence holds, 256: the sequence has ended (its end, or an 'N')
FQ_DEV u32 eval_seed_byte(const EvalSeedArgs& a, const EvalText& x, u32 hit, int dir, int d) {
    const int rd = (int)((hit >> 9) & 0x1FFFFFu), pos = (int)(hit & 511u);
    int j;
    if (dir == 0) {
        j = pos + 10 + d;
        if (j >= (int)a.r.len[rd] - a.shift_tail) return 256u;
    } else {
        j = pos - 1 - d;
        if (j < 0) return 256u;
    }
    const u32 b = eval_byte(a.r, x, rd, j);
    return b == (u32)'N' ? 256u : b;
}

FQ_DEV void eval_seed_walk_x_body(const EvalSeedArgs& a, const EvalText& x, u32* lds) {
    const int dir = block_id(), tid = thread_id(), T = block_threads();
    const u32 dead = dir == 0 ? 0x80000000u : 0x40000000u;
    const u64 nh = *a.n_hits < a.cap ? *a.n_hits : a.cap;
    u8* path = a.path + 512 * dir;
    int depth = 0;
    u32 last = 0;
    bool leaf = true;
    for (; depth < 512; depth++) {
        if (tid < 16) lds[tid] = tid < 8 ? 0u : 0xFFFFFFFFu;
        block_sync();
        u32 c[8], lo[8];
#pragma unroll
        for (int b = 0; b < 8; b++) { c[b] = 0u; lo[b] = 0xFFFFFFFFu; }
        for (u64 k = (u64)tid; k < nh; k += (u64)T) {
            const u32 h = __hip_atomic_load(&a.hits[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (h & dead) continue;
            // (a live hit's byte at depth - 1 is no 'N' and lies inside its sequence: it would have died there)
            u32 b = 256u;
            if (depth == 0 || (eval_seed_byte(a, x, h, dir, depth - 1) & 7u) == last) b = eval_seed_byte(a, x, h, dir, depth);
            if (b > 255u) {
                g_atomic_or_u32(&a.hits[k], dead);   // (the other direction's workgroup owns the other bit of the word)
                continue;
            }
            const u32 word = h & 0x3FFFFFFFu;
#pragma unroll
            for (u32 e = 0; e < 8u; e++) {
                const bool in = (b & 7u) == e;
                c[e] += in;
                lo[e] = in && word < lo[e] ? word : lo[e];
            }
        }
#pragma unroll
        for (int b = 0; b < 8; b++)
            if (c[b]) {
                lds_add_u32(&lds[b], c[b]);
                lds_min_u32(&lds[8 + b], lo[b]);
            }
        block_sync();
        u32 n[8], total = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) { n[b] = lds[b]; total += n[b]; }
        int pick = -1;   // children[0..7] in order; at most one can hold 95 %
#pragma unroll
        for (int b = 0; b < 8; b++)
            if (pick < 0 && n[b] && total >= 50u && (double)n[b] / (double)total >= 0.95) pick = b;
        const u32 creator = pick >= 0 ? lds[8 + pick] : 0u;
        block_sync();
        if (total < 50u) break;                      // NUM_THRESHOLD
        if (pick < 0) {
            leaf = false;
            break;
        }
        last = (u32)pick;
        if (tid == 0) path[depth] = (u8)eval_seed_byte(a, x, creator, dir, depth);
    }
    if (tid == 0) {
        a.path_len[dir] = depth;
        if (!leaf) g_atomic_exch_u32((u32*)&a.path_len[2], 0u);
    }
}

}  // namespace fq
