// fq_census.h - the adapter census: FilterResult::mAdapter1 / mAdapter2 (src/filterresult.cpp:115-180, the two string-keyed
// maps behind the report's adapter_cutting.read1_adapter_counts / read2_adapter_counts) counted on the device.
//
// A map only grows, so a key is admitted or refused at its first occurrence for good, and an admitted key's count is the
// number of its occurrences (for map 2: of those the pair form's early return, quirk #8, does not skip).  One launch
// therefore is, per map:
//   gather   the units that hand a string to addAdapterTrimmed become items: where the bytes are, the order key
//            (unit, slot within the unit) that says when the reference would have seen them, a 64-bit hash of the bytes
//            and the low-complexity bit;
//   look-up  against the persistent table (hash, then the bytes): a hit adds to the key's count, a miss is a candidate;
//   dedupe   the candidates claim slots of a per-launch table by their hash; the smallest order key of a slot is the
//            first occurrence; every item is then compared with its slot's first item byte by byte, and the items that
//            differ (two strings, one hash) go round again under another salt until none are left;
//   admit    with s the map's size: candidate j, in order of first occurrence, is admitted iff
//            !(s > 20000 || (s > 5000 && low_complexity(j))), and s advances on admission.  Everything is admitted while
//            s <= 5000, afterwards only the strings that are not low complexity, while s <= 20000: two thresholds on the
//            order key (the K-th smallest first occurrence: a radix select the host drives), then every slot decides
//            for itself and appends its key to the persistent table.
// Map 1 does not depend on map 2; a pair form's read 2 string is dropped when map 1 refused its read 1 string, so map 1 is
// settled first.  Every phase is a kernel of its own: the kernel boundary is what makes one phase's writes visible to the
// next.  No workgroup waits for another, every probe loop is bounded by the table it probes.
#pragma once
#include "fq_intrin.h"
#include "fq_types.h"

namespace fq {

enum {
    CS_MAX_ADAPTER_REC = 20000,      // filterresult.cpp:7
    CS_LOW_COMPLEXITY_SKIP = 5000,   // filterresult.cpp:8
    CS_MAX_ENTRIES = CS_MAX_ADAPTER_REC + 1,   // an insertion is refused once size > 20000
    CS_INDEX_SLOTS = 1 << 16,        // the persistent table's open-addressing index (entry + 1, 0 = empty): load <= 0.31
    CS_GROUP = 8,                    // lanes that share one string: lane j reads bytes j, j + 8, ...
    CS_BLOCK = 256,
};
// item states
enum { CS_NEW = 0, CS_HIT = 1, CS_CAND = 2, CS_RESOLVED = 3, CS_REFUSED = 4, CS_SKIP = 5 };
// CsItem::meta: bits 0..15 the string's length, 16..17 where the bytes are, 18 the map, 19 low complexity, 20 pair form
enum { CS_SRC_SHIFT = 16, CS_SRC_BLOB = 2, CS_MAP_BIT = 1u << 18, CS_LC_BIT = 1u << 19, CS_PAIR_BIT = 1u << 20 };
enum { CS_VERDICT_ADMITTED = 1, CS_VERDICT_REFUSED = 2 };
enum { CS_RF_ADAPTER = 0x04, CS_RF_ADAPTER_OV = 0x08 };   // FASTP_GPU_RF_ADAPTER / FASTP_GPU_RF_ADAPTER_OV (include/fastp_gpu.h)
#define CS_NONE 0xFFFFFFFFu
#define CS_CLOSED 0x8000000000000000ull   // a dedupe slot of an earlier round: no live hash word has this bit
// launch counters (CsArgs::ctl)
enum { CS_CTL_ITEMS = 0, CS_CTL_CAND = 1, CS_CTL_UNRESOLVED = 2, CS_CTL_SLOTS = 3, CS_CTL_TOO_LONG = 4, CS_CTL_WORDS = 8 };

struct CsItem {
    u64 hash0;   // of the bytes, salt 0: what the persistent table keeps
    u64 hash;    // under the current round's salt
    u64 key;     // order key: unit * slots per unit + slot
    u32 off;     // byte offset in its source
    u32 meta;
    u32 link;    // pair form, read 2's string: the item of read 1's string, CS_NONE when that was empty
    u32 state;
    u32 slot;    // dedupe slot (CS_CAND after an insert, CS_RESOLVED)
    u32 pad;
};   // 48 bytes

struct CsMap {   // the persistent table of one map
    u32* index;  // [CS_INDEX_SLOTS]
    u64* ehash;  // [CS_MAX_ENTRIES]
    u64* ecount;
    u32* eoff;
    u32* elen;
    u8* arena;
    u32* ctl;    // [0] entries, [1] arena bytes in use
    u32 arena_cap;
    u32 pad;
};

struct CsMate {
    const u8* text;
    const u32* line_off;
    const u32* line_len;
    const u32* res;   // fastp_gpu_read_result as three dwords
};

struct CsArgs {
    CsMate m[2];
    const u32* events;      // fastp_gpu_adapter_event as three dwords
    const u8* blob;         // adapter sequences: -a | --adapter_sequence_r2 | the --adapter_fasta entries
    const u32* blob_off;    // [2 + n_fasta]
    const u32* blob_len;
    CsItem* items;
    u32* ctl;
    // the per-launch dedupe table
    u64* s_word;
    u64* s_first;
    u32* s_item;
    u32* s_count;
    u32* s_verdict;
    u32* hist;              // [256]
    CsMap map;
    u64 hash_mask, salt;
    u64 x1, x2;             // admit: key < x1, or not low complexity and key < x2
    u64 sel_lo, sel_prefix; // select: keys >= sel_lo [that are not low complexity] whose bits above the digit equal sel_prefix
    int n, paired, n_events, n_fasta, n_items, n_slots, which, max_str;
    int want_state, sel_shift, sel_nonlc, sel_top;
};

// ---- the hash: a sum over positions, so that the lanes of a group add up their own bytes ----------------------------
__host__ __device__ inline u64 cs_mix(u64 x) {   // splitmix64's finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ inline u64 cs_term(u32 pos, u32 byte, u64 salt) { return cs_mix((((u64)pos << 8) | byte) + salt * 0x9E3779B97F4A7C15ull + 1); }
__host__ __device__ inline u64 cs_finish(u64 sum, u32 len, u64 salt, u64 mask) { return cs_mix(sum + ((u64)len << 40) + salt) & mask; }

FQ_DEV u32 cs_min(u32 x, u32 y) { return x < y ? x : y; }
FQ_DEV u32 cs_sum_group(u32 v) { return sum8(v); }
FQ_DEV u64 cs_sum_group_u64(u64 v) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#pragma unroll
    for (int sh = 1; sh < CS_GROUP; sh <<= 1) {
        const u32 olo = shfl_xor(lo, sh), ohi = shfl_xor(hi, sh);
        const u64 s = (((u64)hi << 32) | lo) + (((u64)ohi << 32) | olo);
        lo = (u32)s; hi = (u32)(s >> 32);
    }
    return ((u64)hi << 32) | lo;
}

// the items of the map this launch works on (which < 0: both) that are in `state`
FQ_DEV bool cs_in_pass(const CsArgs& a, u32 i, u32 state) {
    if (i >= (u32)a.n_items) return false;
    const CsItem& it = a.items[i];
    return it.state == state && (a.which < 0 || ((it.meta & CS_MAP_BIT) != 0) == (a.which != 0));
}

FQ_DEV const u8* cs_bytes(const CsArgs& a, const CsItem& it) {
    const u32 src = (it.meta >> CS_SRC_SHIFT) & 3u;
    const u8* base = src == CS_SRC_BLOB ? a.blob : a.m[src & 1u].text;
    return base + it.off;
}

// one wavefront-wide compaction step: the lanes with `pred` get consecutive slots of the item list
FQ_DEV u32 cs_claim_items(const CsArgs& a, bool pred) {
    const u64 mask = ballot(pred);
    u32 base = 0;
    if (lane_id() == 0 && mask) base = g_atomic_add_u32(&a.ctl[CS_CTL_ITEMS], (u32)popc64(mask));
    base = shfl(base, 0);
    return base + (u32)popc64(mask & (((u64)1 << lane_id()) - 1));
}

// the string a result record (or an --adapter_fasta event) names: (source, offset, length), length 0 = no string
struct CsString { u32 src, off, len; };
FQ_DEV CsString cs_string(const CsArgs& a, int mt, int g, int pos, u32 alen, u32 front, int blob_entry, bool& too_long) {
    CsString s = {0, 0, 0};
    if (pos < 0) {   // the first alen bytes of the adapter sequence
        s.src = CS_SRC_BLOB;
        s.off = a.blob_off[blob_entry];
        s.len = cs_min(alen, a.blob_len[blob_entry]);
    } else {         // bytes [front + pos, + alen) of the sequence line, clamped to the line
        const u32 ll = a.m[mt].line_len[4 * (size_t)g + 1], start = front + (u32)pos;
        s.src = (u32)mt;
        if (start < ll) {
            s.off = a.m[mt].line_off[4 * (size_t)g + 1] + start;
            s.len = cs_min(alen, ll - start);
        }
    }
    if (s.len > (u32)a.max_str) { too_long = true; s.len = 0; }
    return s;
}

FQ_DEV void cs_put_item(const CsArgs& a, u32 idx, const CsString& s, u64 key, int map, bool pair, u32 link) {
    CsItem it;
    it.hash0 = it.hash = 0;
    it.key = key;
    it.off = s.off;
    it.meta = s.len | (s.src << CS_SRC_SHIFT) | (map ? CS_MAP_BIT : 0u) | (pair ? CS_PAIR_BIT : 0u);
    it.link = link;
    it.state = CS_NEW;
    it.slot = CS_NONE;
    it.pad = 0;
    a.items[idx] = it;
}

// ---- gather ---------------------------------------------------------------------------------------------------------
// one lane per unit: the pair form (read 1 trimmed by the overlap analysis) or each mate's single form
FQ_DEV void cs_gather_units_body(const CsArgs& a) {
    const int g = block_id() * block_threads() + thread_id();
    const bool live = g < a.n;
    const u32 slots = a.paired ? 2u + 2u * (u32)a.n_fasta : 1u + (u32)a.n_fasta;
    bool too_long = false, pair = false;
    CsString s[2] = {{0, 0, 0}, {0, 0, 0}};
    if (live) {
        const u32 w1 = a.m[0].res[3 * (size_t)g + 1];
        pair = a.paired && ((w1 >> 8) & CS_RF_ADAPTER_OV);
        for (int mt = 0; mt < (a.paired ? 2 : 1); mt++) {
            const u32* r = a.m[mt].res + 3 * (size_t)g;
            const u32 front = r[0] & 0xFFFFu, flags = (r[1] >> 8) & 0xFFu, alen = r[2] & 0xFFFFu;
            const int pos = (int)(int16_t)(r[1] >> 16);
            if (alen && (pair || (flags & CS_RF_ADAPTER))) s[mt] = cs_string(a, mt, g, pos, alen, front, mt, too_long);
        }
    }
    const u32 i1 = cs_claim_items(a, s[0].len != 0);
    if (s[0].len) cs_put_item(a, i1, s[0], (u64)g * slots, 0, pair, CS_NONE);
    if (a.paired) {   // (uniform: every lane takes part in the second claim)
        const u32 i2 = cs_claim_items(a, s[1].len != 0);
        if (s[1].len) cs_put_item(a, i2, s[1], (u64)g * slots + 1, 1, pair, (pair && s[0].len) ? i1 : CS_NONE);
    }
    if (too_long) a.ctl[CS_CTL_TOO_LONG] = 1;
}

// one lane per --adapter_fasta event (the list is unordered: the order key carries the adapter's index)
FQ_DEV void cs_gather_events_body(const CsArgs& a) {
    const int e = block_id() * block_threads() + thread_id();
    bool too_long = false;
    CsString s = {0, 0, 0};
    u64 key = 0;
    int mt = 0;
    if (e < a.n_events) {
        const u32 rd = a.events[3 * (size_t)e], w1 = a.events[3 * (size_t)e + 1], ai = a.events[3 * (size_t)e + 2] & 0xFFFFu;
        mt = a.paired ? (int)(rd & 1u) : 0;
        const u32 g = a.paired ? rd >> 1 : rd;
        if (g < (u32)a.n && ai < (u32)a.n_fasta) {
            const u32 front = a.m[mt].res[3 * (size_t)g] & 0xFFFFu;
            s = cs_string(a, mt, (int)g, (int)(int16_t)(w1 & 0xFFFFu), w1 >> 16, front, 2 + (int)ai, too_long);
            const u32 slots = a.paired ? 2u + 2u * (u32)a.n_fasta : 1u + (u32)a.n_fasta;
            key = (u64)g * slots + (a.paired ? 2u + (u32)mt * (u32)a.n_fasta : 1u) + ai;
        }
    }
    const u32 idx = cs_claim_items(a, s.len != 0);
    if (s.len) cs_put_item(a, idx, s, key, mt, false, CS_NONE);
    if (too_long) a.ctl[CS_CTL_TOO_LONG] = 1;
}

// eight lanes per item: the hash of its bytes under a.salt and (salt 0) the low-complexity bit,
// lowComplexity(a) = (number of i with a[i] != a[i + 1]) < len / 2 (filterresult.cpp:115-122)
FQ_DEV void cs_hash_body(const CsArgs& a) {
    const u32 t = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    const u32 i = t / CS_GROUP, sub = t % CS_GROUP;
    const bool live = cs_in_pass(a, i, (u32)a.want_state);
    u64 sum = 0;
    u32 diff = 0, len = 0;
    if (live) {
        const CsItem it = a.items[i];
        const u8* p = cs_bytes(a, it);
        len = it.meta & 0xFFFFu;
        for (u32 k = sub; k < len; k += CS_GROUP) {
            const u32 b = p[k];
            sum += cs_term(k, b, a.salt);
            if (k + 1 < len) diff += b != p[k + 1];
        }
    }
    sum = cs_sum_group_u64(sum);
    diff = cs_sum_group(diff);
    if (live && sub == 0) {
        const u64 h = cs_finish(sum, len, a.salt, a.hash_mask);
        a.items[i].hash = h;
        if (a.salt == 0) {
            a.items[i].hash0 = h;
            if (diff < len / 2) a.items[i].meta |= CS_LC_BIT;
        }
    }
}

// ---- look-up against the persistent table (read only here, but for the counts) ----------------------------------------
FQ_DEV void cs_lookup_body(const CsArgs& a) {
    const u32 t = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    const u32 i = t / CS_GROUP, sub = t % CS_GROUP;
    bool active = cs_in_pass(a, i, CS_NEW);
    const bool mine = active;
    CsItem it = {};
    const u8* p = nullptr;
    u32 len = 0, found = CS_NONE;
    if (active) {
        it = a.items[i];
        p = cs_bytes(a, it);
        len = it.meta & 0xFFFFu;
    }
    const u32 entries = a.map.ctl[0];
    if (entries == 0) active = false;
    // Each lane walks its probe sequence on its own (the lanes of a group read the same words) up to the next entry with the
    // item's hash and length, or the empty slot that ends the sequence; only the byte compare is the group's joint work.
    u32 step = 0;
    while (ballot(active)) {
        u32 mism = 0, e = 0;
        bool same = false;
        if (active) {
            for (; step < CS_INDEX_SLOTS; step++) {
                e = a.map.index[((u32)it.hash0 + step) & (CS_INDEX_SLOTS - 1)];
                if (e == 0 || (a.map.ehash[e - 1] == it.hash0 && a.map.elen[e - 1] == len)) break;
            }
            same = step < CS_INDEX_SLOTS && e != 0;
            if (same) {
                const u8* q = a.map.arena + a.map.eoff[e - 1];
                for (u32 k = sub; k < len; k += CS_GROUP) mism += p[k] != q[k];
            }
        }
        mism = cs_sum_group(mism);
        if (active) {
            if (same && mism == 0) found = e - 1;
            if (!same || mism == 0) active = false;   // the end of the sequence, or the key
            step++;
        }
    }
    if (mine && sub == 0) {
        if (found != CS_NONE) {
            g_atomic_add_u64(&a.map.ecount[found], 1);
            a.items[i].state = CS_HIT;
        } else if (entries > CS_MAX_ADAPTER_REC) {
            a.items[i].state = CS_REFUSED;   // the map takes no new key any more
        } else {
            a.items[i].state = CS_CAND;
            g_atomic_add_u32(&a.ctl[CS_CTL_CAND], 1u);
        }
    }
}

// ---- candidate dedupe -------------------------------------------------------------------------------------------------
FQ_DEV bool cs_is_cand(const CsArgs& a, u32 i) { return cs_in_pass(a, i, CS_CAND); }
// claim the slot of this round's hash word, leave the smallest order key there
FQ_DEV void cs_insert_body(const CsArgs& a) {
    const u32 i = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    if (!cs_is_cand(a, i)) return;
    const u64 h = a.items[i].hash;
    const u64 word = (h & ~CS_CLOSED) ? (h & ~CS_CLOSED) : CS_CLOSED - 1;   // never 0 (an empty slot), never a closed slot's word
    const u32 mask = (u32)a.n_slots - 1;
    for (u32 step = 0; step < (u32)a.n_slots; step++) {
        const u32 s = ((u32)h + step) & mask;
        const u64 old = g_atomic_cas_u64(&a.s_word[s], 0, word);
        if (old == 0 || old == word) {
            if (old == 0) g_atomic_add_u32(&a.ctl[CS_CTL_SLOTS], 1u);
            g_atomic_min_u64(&a.s_first[s], a.items[i].key);
            a.items[i].slot = s;
            return;
        }
    }
}
// the item with the slot's smallest order key is its first occurrence; the slot is closed for later rounds
FQ_DEV void cs_first_body(const CsArgs& a) {
    const u32 i = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    if (!cs_is_cand(a, i)) return;
    const u32 s = a.items[i].slot;
    if (s == CS_NONE || a.s_first[s] != a.items[i].key) return;
    a.s_item[s] = i;
    a.s_word[s] |= CS_CLOSED;
}
// eight lanes per item: the same bytes as the slot's first item, or another string with the same hash (next round)
FQ_DEV void cs_verify_body(const CsArgs& a) {
    const u32 t = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    const u32 i = t / CS_GROUP, sub = t % CS_GROUP;
    const bool live = cs_is_cand(a, i) && a.items[i].slot != CS_NONE;
    u32 mism = 0, s = 0;
    if (live) {
        const CsItem it = a.items[i];
        s = it.slot;
        const CsItem f = a.items[a.s_item[s]];
        const u32 len = it.meta & 0xFFFFu;
        if ((f.meta & 0xFFFFu) != len) mism = 1;
        else {
            const u8 *p = cs_bytes(a, it), *q = cs_bytes(a, f);
            for (u32 k = sub; k < len; k += CS_GROUP) mism += p[k] != q[k];
        }
    }
    mism = cs_sum_group(mism);
    if (live && sub == 0) {
        if (mism == 0) {
            a.items[i].state = CS_RESOLVED;
            g_atomic_add_u32(&a.s_count[s], 1u);
        } else {
            a.items[i].slot = CS_NONE;
            g_atomic_add_u32(&a.ctl[CS_CTL_UNRESOLVED], 1u);
        }
    }
}

// ---- admit --------------------------------------------------------------------------------------------------------------
// one digit of the radix select over the slots' first occurrences: a histogram of bits [sel_shift, sel_shift + 8) of the keys
// >= sel_lo [of strings that are not low complexity] whose higher bits equal sel_prefix
FQ_DEV void cs_hist_body(const CsArgs& a, u32* lds) {
    lds[thread_id()] = 0;
    block_sync();
    for (u32 s = (u32)block_id() * (u32)block_threads() + (u32)thread_id(); s < (u32)a.n_slots; s += (u32)grid_blocks() * (u32)block_threads()) {
        if (a.s_word[s] == 0) continue;
        const u64 key = a.s_first[s];
        if (key < a.sel_lo) continue;
        if (a.sel_nonlc && (a.items[a.s_item[s]].meta & CS_LC_BIT)) continue;
        if (!a.sel_top && (key >> (a.sel_shift + 8)) != a.sel_prefix) continue;
        lds_add_u32(&lds[(u32)(key >> a.sel_shift) & 255u], 1u);
    }
    block_sync();
    if (lds[thread_id()]) g_atomic_add_u32(&a.hist[thread_id()], lds[thread_id()]);
}

// eight lanes per slot: the verdict, and an admitted key's bytes, count and hash appended to the persistent table
FQ_DEV void cs_admit_body(const CsArgs& a) {
    const u32 t = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    const u32 s = t / CS_GROUP, sub = t % CS_GROUP;
    bool admit = false;
    CsItem f = {};
    if (s < (u32)a.n_slots && a.s_word[s] != 0) {
        f = a.items[a.s_item[s]];
        const u64 key = a.s_first[s];
        admit = key < a.x1 || (!(f.meta & CS_LC_BIT) && key < a.x2);
        if (sub == 0) a.s_verdict[s] = admit ? CS_VERDICT_ADMITTED : CS_VERDICT_REFUSED;
    }
    const u32 len = f.meta & 0xFFFFu;
    u32 e = 0, aoff = 0;
    if (admit && sub == 0) {
        e = g_atomic_add_u32(&a.map.ctl[0], 1u);
        aoff = g_atomic_add_u32(&a.map.ctl[1], len);
    }
    e = shfl(e, lane_id() & ~(CS_GROUP - 1));
    aoff = shfl(aoff, lane_id() & ~(CS_GROUP - 1));
    if (!admit || e >= CS_MAX_ENTRIES || aoff + len > a.map.arena_cap) return;   // (cannot happen: the thresholds admit at most what fits)
    const u8* p = cs_bytes(a, f);
    for (u32 k = sub; k < len; k += CS_GROUP) a.map.arena[aoff + k] = p[k];
    if (sub != 0) return;
    a.map.ehash[e] = f.hash0;
    a.map.ecount[e] = a.s_count[s];
    a.map.eoff[e] = aoff;
    a.map.elen[e] = len;
    for (u32 step = 0; step < CS_INDEX_SLOTS; step++) {
        const u32 at = ((u32)f.hash0 + step) & (CS_INDEX_SLOTS - 1);
        if (g_atomic_cas_u32(&a.map.index[at], 0u, e + 1) == 0u) break;
    }
}

// quirk #8: a pair form's read 2 string is not looked at when a cap refused read 1's (filterresult.cpp:154-180)
FQ_DEV void cs_pair_verdict_body(const CsArgs& a) {
    const u32 i = (u32)block_id() * (u32)block_threads() + (u32)thread_id();
    if (i >= (u32)a.n_items) return;
    const CsItem it = a.items[i];
    if (!(it.meta & CS_MAP_BIT) || !(it.meta & CS_PAIR_BIT) || it.link == CS_NONE) return;
    const CsItem p = a.items[it.link];
    const bool taken = p.state == CS_HIT || (p.state == CS_RESOLVED && a.s_verdict[p.slot] == CS_VERDICT_ADMITTED);
    if (!taken) a.items[i].state = CS_SKIP;
}

}  // namespace fq
