// fq_names.h - what the reference reads out of a record's name line (src/read.cpp): Read::fixMGI (:160-171),
// Read::firstIndex (:87-100), Read::lastIndex (:75-85) and the first space UmiProcessor::addUmiToName looks for
// (src/umiprocessor.cpp:70-76).  The worker loops fix the MGI id first and hand the fixed name to everything else
// (src/peprocessor.cpp:413-420, src/seprocessor.cpp:227-233), so every function here takes the name AS PARSED (`name`,
// `len` bytes, the '@' counts) plus the result of the MGI test, and answers in the coordinates of the FIXED name:
//     fixed = name[0, len - 2) + ' ' + name[len - 2, len)   if mgi,   name   otherwise
// Nothing is read outside name[0, len).  The functions know nothing about the formatter: they take a pointer and a length.
//   - the serial forms: one thread (or the host: fq_glue.cpp, fq_stream.cpp) walks the bytes
//   - the group forms (device only): the 16 lanes of a copy group look at 16 bytes per step, one compare per lane and a
//     ballot cut down to the group's 16 bits; every lane of the group must call them, with the same arguments
#pragma once
#include <stdint.h>
#ifdef FQ_NAMES_HOST
#include <string>
#endif

#ifdef __HIP__
#define FQ_NAMES_FN __host__ __device__ inline
#else
#define FQ_NAMES_FN inline
#endif

namespace fq {

// a piece of the fixed name: [off, off + len).  A piece that reaches the end of an MGI-fixed name (off + len == len of the
// parsed name + 1) holds the space of the fix: it is name[off, name_len - 2) + ' ' + name[name_len - 2, name_len), len >= 3
struct NameIndex {
    uint32_t off, len;
};

// Read::fixMGI: the name ends in "/1" or "/2"
FQ_NAMES_FN bool name_is_mgi(const uint8_t* name, uint32_t len) {
    return len >= 2u && name[len - 2u] == '/' && (name[len - 1u] == '1' || name[len - 1u] == '2');
}

// Both index scans walk i = fixed_len - 3 ... 0.  With the MGI fix, position fixed_len - 3 is the inserted space, which
// matches nothing: in the coordinates of the parsed name both walks start at len - 3 either way, and positions below
// len - 2 are the same in both names.

// Read::firstIndex: behind the last ':' in front of the final two characters, up to the leftmost '+' behind that ':'
FQ_NAMES_FN NameIndex name_first_index(const uint8_t* name, uint32_t len, bool mgi) {
    NameIndex r = {0u, 0u};
    const uint32_t flen = len + (mgi ? 1u : 0u);
    if (flen < 5u) return r;
    uint32_t stop = flen;
    for (int i = (int)len - 3; i >= 0; i--) {
        if (name[i] == '+') stop = (uint32_t)i;
        if (name[i] == ':') {
            r.off = (uint32_t)i + 1u;
            r.len = stop - r.off;
            return r;
        }
    }
    return r;
}

// Read::lastIndex: behind the last ':' or '+' in front of the final two characters, to the end of the name
FQ_NAMES_FN NameIndex name_last_index(const uint8_t* name, uint32_t len, bool mgi) {
    NameIndex r = {0u, 0u};
    const uint32_t flen = len + (mgi ? 1u : 0u);
    if (flen < 5u) return r;
    for (int i = (int)len - 3; i >= 0; i--)
        if (name[i] == ':' || name[i] == '+') {
            r.off = (uint32_t)i + 1u;
            r.len = flen - r.off;
            return r;
        }
    return r;
}

// position of the fixed name's first space, its length if it has none (addUmiToName then appends).  An MGI name's
// inserted space sits at len - 2 and its last two characters are no spaces, so len - 2 is the answer when the bytes
// in front hold none
FQ_NAMES_FN uint32_t name_first_space(const uint8_t* name, uint32_t len, bool mgi) {
    const uint32_t lim = mgi ? len - 2u : len;
    for (uint32_t i = 0; i < lim; i++)
        if (name[i] == ' ') return i;
    return lim;
}

#ifdef FQ_DEV
// the group's 16 bits of a ballot; bit k = lane k of the group
FQ_DEV uint32_t names_ballot16(bool pred) { return (uint32_t)(ballot(pred) >> (lane_id() & 48)) & 0xFFFFu; }

// step s of the backward walks: lane gl looks at position top - gl, so a lower bit is a position the reference sees earlier
FQ_DEV NameIndex name_first_index_group(const uint8_t* name, uint32_t len, bool mgi, int gl) {
    NameIndex r = {0u, 0u};
    const uint32_t flen = len + (mgi ? 1u : 0u);
    if (flen < 5u) return r;
    uint32_t stop = flen;
    for (int top = (int)len - 3; top >= 0; top -= 16) {
        const int p = top - gl;
        const uint8_t c = p >= 0 ? name[p] : (uint8_t)0;
        const uint32_t colon = names_ballot16(c == ':'), plus = names_ballot16(c == '+');
        if (colon) {
            const int kc = ffs32(colon) - 1;
            const uint32_t seen = plus & ((1u << kc) - 1u);   // the '+' the walk passed before it met the ':'
            if (seen) stop = (uint32_t)(top - (31 - clz32(seen)));
            r.off = (uint32_t)(top - kc) + 1u;
            r.len = stop - r.off;
            return r;
        }
        if (plus) stop = (uint32_t)(top - (31 - clz32(plus)));
    }
    return r;
}

FQ_DEV NameIndex name_last_index_group(const uint8_t* name, uint32_t len, bool mgi, int gl) {
    NameIndex r = {0u, 0u};
    const uint32_t flen = len + (mgi ? 1u : 0u);
    if (flen < 5u) return r;
    for (int top = (int)len - 3; top >= 0; top -= 16) {
        const int p = top - gl;
        const uint8_t c = p >= 0 ? name[p] : (uint8_t)0;
        const uint32_t hit = names_ballot16(c == ':' || c == '+');
        if (hit) {
            r.off = (uint32_t)(top - (ffs32(hit) - 1)) + 1u;
            r.len = flen - r.off;
            return r;
        }
    }
    return r;
}

FQ_DEV uint32_t name_first_space_group(const uint8_t* name, uint32_t len, bool mgi, int gl) {
    const uint32_t lim = mgi ? len - 2u : len;
    for (uint32_t base = 0; base < lim; base += 16u) {
        const uint32_t p = base + (uint32_t)gl;
        const uint32_t hit = names_ballot16(p < lim && name[p] == ' ');
        if (hit) return base + (uint32_t)(ffs32(hit) - 1);
    }
    return lim;
}
#endif  // FQ_DEV

#ifdef FQ_NAMES_HOST
// The host writers' form of the whole name edit (fq_glue.cpp, fq_stream.cpp; needs <string>): Read::fixMGI on each mate,
// then UmiProcessor::process (src/umiprocessor.cpp:11-61) on the fixed names, as the reference does it - on strings, with
// no coordinate of the parsed name involved.  umi_loc_word: FASTP_GPU_UMI_* | FASTP_GPU_NAME_FIX_MGI (0x100);
// name2 == nullptr: single-end.  out2 may be null.
inline std::string names_host_fixed(const char* name, size_t len, bool fix_mgi) {
    std::string s(name, len);
    if (fix_mgi && name_is_mgi((const uint8_t*)name, (uint32_t)len)) s.insert(len - 2, 1, ' ');
    return s;
}
inline std::string names_host_index(const std::string& fixed, bool first) {
    const NameIndex ix = first ? name_first_index((const uint8_t*)fixed.data(), (uint32_t)fixed.size(), false)
                               : name_last_index((const uint8_t*)fixed.data(), (uint32_t)fixed.size(), false);
    return fixed.substr(ix.off, ix.len);
}
inline void names_host_edit(int umi_loc_word, int umi_len, const std::string& delim, const std::string& prefix,
                            const char* name1, size_t nl1, const char* seq1, size_t sl1,
                            const char* name2, size_t nl2, const char* seq2, size_t sl2,
                            std::string* out1, std::string* out2) {
    const bool paired = name2 != nullptr, fix_mgi = (umi_loc_word & 0x100) != 0;
    const int loc = umi_loc_word & 0xFF;
    std::string f1 = names_host_fixed(name1, nl1, fix_mgi), f2 = paired ? names_host_fixed(name2, nl2, fix_mgi) : std::string();
    const size_t ul = (size_t)(umi_len > 0 ? umi_len : 0);
    std::string umi;
    bool tag = loc != 0;
    const bool always = loc == 3 || loc == 6;   // per_read / per_index: tagged even when the UMI is empty
    if (loc == 1) umi.assign(seq1, sl1 < ul ? sl1 : ul);
    else if (loc == 2) { if (paired) umi.assign(seq2, sl2 < ul ? sl2 : ul); else tag = false; }
    else if (loc == 3) { umi.assign(seq1, sl1 < ul ? sl1 : ul); if (paired) { umi += '_'; umi.append(seq2, sl2 < ul ? sl2 : ul); } }
    else if (loc == 4) umi = names_host_index(f1, true);
    else if (loc == 5) { if (paired) umi = names_host_index(f2, false); else tag = false; }
    else if (loc == 6) { umi = names_host_index(f1, true); if (paired) umi += "_" + names_host_index(f2, false); }
    if (!always && umi.empty()) tag = false;
    if (tag) {  // addUmiToName :62-81: in front of the first space, appended if there is none
        const std::string t = delim + (prefix.empty() ? std::string() : prefix + "_") + umi;
        size_t sp = f1.find(' ');
        f1.insert(sp == std::string::npos ? f1.size() : sp, t);
        if (paired) {
            sp = f2.find(' ');
            f2.insert(sp == std::string::npos ? f2.size() : sp, t);
        }
    }
    if (out1) out1->swap(f1);
    if (out2 && paired) out2->swap(f2);
}
#endif  // FQ_NAMES_HOST

}  // namespace fq
