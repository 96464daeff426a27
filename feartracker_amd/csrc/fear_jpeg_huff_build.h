// fear_jpeg_huff_build.h — the Huffman table of T.81 K.2 as libjpeg's jpeg_gen_optimal_table builds it, from 256 symbol counts
// (include/fear_train.h fear_jpeg_huff_optimal, DESIGN.md section 14 "Per-file Huffman tables"; jpeg_encode.jpeg_optimal_table_host
// restates it in Python).  Plain C++ without a HIP call, so that the same text is the device code of fear_jpeg_encode.h's table kernel
// (which replaces only the search for the two smallest frequencies by a wave-wide reduction) and a host program's under the sanitizers
// (tools/jpeg_huff_build_host.cpp).
//
// Safe for any 256 uint32 counts: frequencies are summed in 64 bits (257 x 2^32 < 2^41), every chain walk ends after at most 257 links,
// a code size is compared with kHuffMaxDepth before anything is indexed by it, and the length limiting cannot leave its array.
#ifndef FEAR_JPEG_HUFF_BUILD_H
#define FEAR_JPEG_HUFF_BUILD_H

#include <cstdint>

#if defined(__HIPCC__)
#define FEAR_HUFF_HD __host__ __device__
#else
#define FEAR_HUFF_HD
#endif

constexpr int kHuffSymbols = 257;          // 256 and the reserved one, whose code would be all ones
constexpr int kHuffMaxDepth = 32;          // libjpeg's MAX_CLEN: a deeper tree is refused (JERR_HUFF_CLEN_OVERFLOW)

struct HuffWork {
    uint64_t freq[kHuffSymbols];           // 0: merged away, or never seen
    int32_t size[kHuffSymbols];            // the symbol's depth in the tree so far
    int32_t others[kHuffSymbols];          // the next symbol of the same subtree, -1 at the chain's end
    int32_t bits[kHuffMaxDepth + 2];       // codes per length
    int32_t at[kHuffMaxDepth + 2];         // where the symbols of a length begin in the values
};

FEAR_HUFF_HD inline void huff_init_one(HuffWork& w, int i, uint32_t count) {
    w.freq[i] = i == kHuffSymbols - 1 ? 1u : count;
    w.size[i] = 0;
    w.others[i] = -1;
}

// the symbol of the smallest non-zero frequency other than `skip`, the larger symbol in a tie; -1 if there is none
FEAR_HUFF_HD inline int huff_smallest(const HuffWork& w, int skip) {
    int best = -1;
    for (int i = 0; i < kHuffSymbols; ++i)
        if (w.freq[i] && i != skip && (best < 0 || w.freq[i] <= w.freq[best])) best = i;
    return best;
}

// c2's subtree joins c1's: every symbol of both is one level deeper, c2's chain hangs behind c1's
FEAR_HUFF_HD inline void huff_merge(HuffWork& w, int c1, int c2) {
    w.freq[c1] += w.freq[c2];
    w.freq[c2] = 0;
    int guard = kHuffSymbols;
    ++w.size[c1];
    while (w.others[c1] >= 0 && --guard > 0) {
        c1 = w.others[c1];
        ++w.size[c1];
    }
    w.others[c1] = c2;
    ++w.size[c2];
    while (w.others[c2] >= 0 && --guard > 0) {
        c2 = w.others[c2];
        ++w.size[c2];
    }
}

// After the last merge: counts[16] codes per length 1..16, values[*n_values] the symbols by (depth in the tree, value), codes[256]
// length << 16 | code per symbol (T.81 annex C; 0 for a symbol without a code) and *depth, the tree's depth before limiting.  False,
// with counts, codes and *n_values zeroed, if that depth is above kHuffMaxDepth.
FEAR_HUFF_HD inline bool huff_finish(HuffWork& w, uint8_t* counts, uint8_t* values, int32_t* n_values, uint32_t* codes, int32_t* depth) {
    int deepest = 0;
    for (int i = 0; i < kHuffSymbols; ++i) deepest = w.size[i] > deepest ? w.size[i] : deepest;
    *depth = deepest;
    for (int i = 0; i < 16; ++i) counts[i] = 0;
    for (int i = 0; i < 256; ++i) codes[i] = 0;
    *n_values = 0;
    if (deepest > kHuffMaxDepth) return false;
    for (int i = 0; i < kHuffMaxDepth + 2; ++i) w.bits[i] = w.at[i] = 0;
    for (int i = 0; i < kHuffSymbols; ++i)
        if (w.size[i]) ++w.bits[w.size[i]];                  // (1..kHuffMaxDepth: checked above)
    // the values: symbols of one depth are contiguous, in rising value; the reserved symbol takes no place
    int n = 0;
    for (int len = 1; len <= kHuffMaxDepth; ++len) {
        w.at[len] = n;
        n += w.bits[len] - (w.size[kHuffSymbols - 1] == len ? 1 : 0);
    }
    for (int i = 0; i < 256; ++i)
        if (w.size[i]) values[w.at[w.size[i]]++] = (uint8_t)i;
    // Adjust_BITS: a pair of the longest codes becomes one a bit shorter, a shorter code two codes a bit longer
    for (int i = kHuffMaxDepth; i > 16; --i) {
        while (w.bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && w.bits[j] == 0) --j;
            if (j == 0) return false;                        // (not a prefix code: no tree gives this)
            w.bits[i] -= 2;
            ++w.bits[i - 1];
            w.bits[j + 1] += 2;
            --w.bits[j];
        }
    }
    int last = 16;
    while (last > 0 && w.bits[last] == 0) --last;
    if (last > 0) --w.bits[last];                            // the reserved symbol leaves the longest length in use
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int c = w.bits[len] < 0 ? 0 : w.bits[len];
        counts[len - 1] = (uint8_t)c;
        for (int i = 0; i < c && k < n; ++i, ++k) codes[values[k]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
    *n_values = n;
    return true;
}

// the whole rule on one thread: the host's form, and the reference for the device's
inline bool huff_build_serial(const uint32_t* freq, uint8_t* counts, uint8_t* values, int32_t* n_values, uint32_t* codes, int32_t* depth) {
    HuffWork w;
    for (int i = 0; i < kHuffSymbols; ++i) huff_init_one(w, i, i < 256 ? freq[i] : 0u);
    for (;;) {
        const int c1 = huff_smallest(w, -1), c2 = huff_smallest(w, c1);
        if (c2 < 0) break;
        huff_merge(w, c1, c2);
    }
    return huff_finish(w, counts, values, n_values, codes, depth);
}

#endif
