// fear_jpeg_progressive.h — progressive JPEG files (SOF2) on the host (include/fear_train.h, DESIGN.md section 14, "Progressive files"):
// every scan decoded to quantised coefficients (ITU-T T.81 annex G.1 and G.2), and those coefficients written again as a baseline file
// with a restart marker after every MCU row, which the resident store then treats as any other baseline file.  Plain C++17 on top of
// fear_jpeg_entropy.h's Huffman, Bits and marker rules: neither HIP nor the GPU is touched, and the file compiles stand-alone
// (tools/jpeg_progressive_host.cpp builds it with the address and undefined-behaviour sanitizers).
//
// Written for hostile input as fear_jpeg_entropy.h is: every read is checked against the buffer's length, every write against the
// caller's capacity or the coefficient buffer the frame header sized, at most kMaxScans scans are decoded, and no scan walks further than
// the frame's block counts.  jpeg_progressive.py restates it in Python check for check, in the same order;
// tests/test_jpeg_progressive_host.py holds the two to the same verdict on every prefix and every flipped byte of a file.
//
// Included by fear_train.hip behind fear_jpeg_entropy.h.
#ifndef FEAR_JPEG_PROGRESSIVE_H
#define FEAR_JPEG_PROGRESSIVE_H

#include "fear_jpeg_entropy.h"

namespace fear_jpeg {

constexpr int kMaxScans = 100;

struct Progressive {
    FearJpegInfo info;
    Huffman dc[4], ac[4];
    bool q_defined[4] = {false, false, false, false};
    uint16_t q[4][64];             // natural order
    uint8_t q_file[4][64];         // as the DQT segment holds it: zigzag order
    uint8_t ids[3], hv[3], tq[3];
    int nf = 0, adobe = -1, restart = 0, scans = 0;
    size_t jfif_at = 0, jfif_len = 0, adobe_at = 0, adobe_len = 0;   // the whole segments, marker included, in front of the first SOS
    int8_t coef_bits[3][64];       // the Al a coefficient has reached, -1: not coded yet (libjpeg's coef_bits)
    uint32_t comp_first[3];
    int own_w[3], own_h[3];        // a component's own block grid: what a scan of that component alone walks
    std::vector<int16_t> coef;     // [total_blocks][64], zigzag order, component-major on the padded grid
};

// `k` plain bits; false when the data ends first.  1 <= k <= 14
inline bool get_bits(Bits& b, int k, int* out) {
    if (b.have < k) b.fill();
    const int v = (int)b.peek(k);
    if (!b.take(k)) return false;
    *out = v;
    return true;
}

inline int16_t wrap16(int v) { return (int16_t)(uint16_t)v; }

// One scan's entropy-coded data from `p` on; `p` leaves at the marker that follows it.
inline int progressive_scan(const uint8_t* d, size_t n, size_t& p, Progressive& pg, int ns, const int* comp, const int* td, const int* ta,
                            int Ss, int Se, int Ah, int Al) {
    const FearJpegInfo& in = pg.info;
    Bits bits{d, n, p};
    int pred[3] = {0, 0, 0};
    int eobrun = 0;
    const int ri = pg.restart, c0 = comp[0];
    const int across = ns > 1 ? in.mcus_x : pg.own_w[c0];
    const uint32_t units = ns > 1 ? (uint32_t)in.mcus_x * (uint32_t)in.mcus_y : (uint32_t)pg.own_w[c0] * (uint32_t)pg.own_h[c0];
    const int p1 = 1 << Al, m1 = -(1 << Al);
    int ux = 0, uy = 0, to_restart = ri, next_rst = 0;
    for (uint32_t u = 0; u < units; ++u) {
        if (ri && u && to_restart == 0) {
            if (!bits.restart(next_rst)) return FEAR_TRAIN_ERR_FORMAT;
            next_rst = (next_rst + 1) & 7;
            to_restart = ri;
            pred[0] = pred[1] = pred[2] = 0;
            eobrun = 0;
        }
        --to_restart;
        if (Ss == 0) {                                                    // a DC scan: the MCU's blocks, or the one block
            for (int s = 0; s < ns; ++s) {
                const int c = comp[s];
                const int bh = ns > 1 ? in.h[c] : 1, bv = ns > 1 ? in.v[c] : 1;
                for (int j = 0; j < bv; ++j)
                    for (int i = 0; i < bh; ++i) {
                        int16_t* blk = pg.coef.data() + ((size_t)pg.comp_first[c] + (size_t)(uy * bv + j) * (size_t)in.blocks_w[c] + (size_t)(ux * bh + i)) * 64;
                        if (Ah == 0) {
                            const int t = bits.symbol(pg.dc[td[s]]);
                            if (t < 0 || t > 15) return FEAR_TRAIN_ERR_FORMAT;
                            int diff;
                            if (!bits.receive(t, &diff)) return FEAR_TRAIN_ERR_FORMAT;
                            pred[c] = wrap16(pred[c] + diff);
                            blk[0] = wrap16((int)((uint32_t)pred[c] << Al));
                        } else {
                            int bit;
                            if (!get_bits(bits, 1, &bit)) return FEAR_TRAIN_ERR_FORMAT;
                            if (bit) blk[0] = wrap16(blk[0] | p1);
                        }
                    }
            }
        } else {
            int16_t* blk = pg.coef.data() + ((size_t)pg.comp_first[c0] + (size_t)uy * (size_t)in.blocks_w[c0] + (size_t)ux) * 64;
            const Huffman& ac = pg.ac[ta[0]];
            if (Ah == 0) {                                                // G.1.2.2: the first scan of a band
                if (eobrun > 0) {
                    --eobrun;
                } else {
                    int k = Ss;
                    while (k <= Se) {
                        const int rs = bits.symbol(ac);
                        if (rs < 0) return FEAR_TRAIN_ERR_FORMAT;
                        const int r = rs >> 4, s = rs & 15;
                        if (s) {
                            k += r;
                            if (k > Se) return FEAR_TRAIN_ERR_FORMAT;
                            int v;
                            if (!bits.receive(s, &v)) return FEAR_TRAIN_ERR_FORMAT;
                            blk[k] = wrap16((int)((uint32_t)v << Al));
                            ++k;
                        } else if (r == 15) {                             // ZRL: a coefficient follows
                            if (k + 16 > Se) return FEAR_TRAIN_ERR_FORMAT;
                            k += 16;
                        } else {                                          // EOBn: this block and eobrun more end here
                            int more = 0;
                            if (r && !get_bits(bits, r, &more)) return FEAR_TRAIN_ERR_FORMAT;
                            eobrun = (1 << r) + more - 1;
                            break;
                        }
                    }
                }
            } else {                                                      // G.1.2.3: refinement
                int k = Ss;
                if (eobrun == 0) {
                    while (k <= Se) {
                        const int rs = bits.symbol(ac);
                        if (rs < 0) return FEAR_TRAIN_ERR_FORMAT;
                        int r = rs >> 4;
                        const int s = rs & 15;
                        int value = 0;
                        if (s) {
                            if (s != 1) return FEAR_TRAIN_ERR_FORMAT;
                            int bit;
                            if (!get_bits(bits, 1, &bit)) return FEAR_TRAIN_ERR_FORMAT;
                            value = bit ? p1 : m1;
                        } else if (r != 15) {
                            int more = 0;
                            if (r && !get_bits(bits, r, &more)) return FEAR_TRAIN_ERR_FORMAT;
                            eobrun = (1 << r) + more;
                            break;
                        }
                        // pass the coefficients with a history, each with its correction bit, and r (ZRL: 16 with the one that ends it) without
                        while (k <= Se) {
                            if (blk[k] != 0) {
                                int bit;
                                if (!get_bits(bits, 1, &bit)) return FEAR_TRAIN_ERR_FORMAT;
                                if (bit && (blk[k] & p1) == 0) blk[k] = wrap16(blk[k] + (blk[k] >= 0 ? p1 : m1));
                            } else if (--r < 0) {
                                break;
                            }
                            ++k;
                        }
                        if (s) {
                            if (k > Se) return FEAR_TRAIN_ERR_FORMAT;
                            blk[k] = (int16_t)value;
                        }
                        ++k;
                    }
                }
                if (eobrun > 0) {
                    for (; k <= Se; ++k)
                        if (blk[k] != 0) {
                            int bit;
                            if (!get_bits(bits, 1, &bit)) return FEAR_TRAIN_ERR_FORMAT;
                            if (bit && (blk[k] & p1) == 0) blk[k] = wrap16(blk[k] + (blk[k] >= 0 ? p1 : m1));
                        }
                    --eobrun;
                }
            }
        }
        if (++ux == across) { ux = 0; ++uy; }
    }
    bits.have -= bits.have & 7;                                           // the rest of the byte is padding and a marker follows at once
    if (bits.have != 0) return FEAR_TRAIN_ERR_FORMAT;
    p = bits.pos;
    return FEAR_TRAIN_OK;
}

// The whole file: the segments, and unless `headers_only` (which returns behind the first SOS header) every scan up to EOI.
inline int progressive_run(const uint8_t* d, size_t n, Progressive& pg, bool headers_only) {
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) return FEAR_TRAIN_ERR_FORMAT;
    FearJpegInfo& info = pg.info;
    std::memset(&info, 0, sizeof(info));
    std::memset(pg.coef_bits, -1, sizeof(pg.coef_bits));
    bool sof = false;
    int nf = 0;
    size_t p = 2;
    for (;;) {
        if (p >= n || d[p] != 0xFF) return FEAR_TRAIN_ERR_FORMAT;        // a file without EOI ends here
        while (p < n && d[p] == 0xFF) ++p;                                // fill bytes
        if (p >= n) return FEAR_TRAIN_ERR_FORMAT;
        const int m = d[p++];
        if (m == 0x01) continue;                                          // TEM stands alone
        if (m == 0xD9) {
            if (pg.scans == 0) return FEAR_TRAIN_ERR_FORMAT;
            break;
        }
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD8)) return FEAR_TRAIN_ERR_FORMAT;
        if (n - p < 2) return FEAR_TRAIN_ERR_FORMAT;
        const size_t L = (size_t)d[p] << 8 | d[p + 1];
        if (L < 2 || L > n - p) return FEAR_TRAIN_ERR_FORMAT;
        const uint8_t* seg = d + p + 2;
        const size_t len = L - 2, seg_at = p - 2;
        p += L;
        if (m == 0xC2) {                                                  // fear_jpeg_entropy.h's SOF0 rules
            if (sof || len < 6) return FEAR_TRAIN_ERR_FORMAT;
            if (seg[0] != 8) return FEAR_TRAIN_ERR_UNSUPPORTED;
            info.height = seg[1] << 8 | seg[2];
            info.width = seg[3] << 8 | seg[4];
            nf = seg[5];
            if (info.width == 0) return FEAR_TRAIN_ERR_FORMAT;
            if (info.height == 0) return FEAR_TRAIN_ERR_UNSUPPORTED;
            if (info.width > FEAR_JPEG_MAX_SIDE || info.height > FEAR_JPEG_MAX_SIDE) return FEAR_TRAIN_ERR_UNSUPPORTED;
            if (nf == 0) return FEAR_TRAIN_ERR_FORMAT;
            if (nf != 1 && nf != 3) return FEAR_TRAIN_ERR_UNSUPPORTED;
            if (len != 6 + 3 * (size_t)nf) return FEAR_TRAIN_ERR_FORMAT;
            for (int i = 0; i < nf; ++i) {
                const uint8_t* c = seg + 6 + 3 * i;
                const int h = c[1] >> 4, v = c[1] & 15;
                if (h < 1 || h > 4 || v < 1 || v > 4 || c[2] > 3) return FEAR_TRAIN_ERR_FORMAT;
                for (int j = 0; j < i; ++j)
                    if (pg.ids[j] == c[0]) return FEAR_TRAIN_ERR_FORMAT;
                pg.ids[i] = c[0];
                pg.hv[i] = c[1];
                info.h[i] = h;
                info.v[i] = v;
                pg.tq[i] = c[2];
            }
            if (nf == 1) {
                info.h[0] = info.v[0] = 1;
            } else {
                const int h = info.h[0], v = info.v[0];
                const bool luma_ok = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma_ok || info.h[1] != 1 || info.v[1] != 1 || info.h[2] != 1 || info.v[2] != 1) return FEAR_TRAIN_ERR_UNSUPPORTED;
            }
            info.components = nf;
            pg.nf = nf;
            info.mcus_x = (info.width + 8 * info.h[0] - 1) / (8 * info.h[0]);
            info.mcus_y = (info.height + 8 * info.v[0] - 1) / (8 * info.v[0]);
            uint32_t total = 0;
            for (int i = 0; i < nf; ++i) {
                info.blocks_w[i] = info.mcus_x * info.h[i];
                info.blocks_h[i] = info.mcus_y * info.v[i];
                pg.comp_first[i] = total;
                total += (uint32_t)info.blocks_w[i] * (uint32_t)info.blocks_h[i];
                pg.own_w[i] = ((info.width * info.h[i] + info.h[0] - 1) / info.h[0] + 7) / 8;
                pg.own_h[i] = ((info.height * info.v[i] + info.v[0] - 1) / info.v[0] + 7) / 8;
            }
            info.total_blocks = total;                                    // at most 3 * 1024 * 1024
            sof = true;
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4) {
            return FEAR_TRAIN_ERR_UNSUPPORTED;                            // baseline and the other frame kinds: not this decoder's
        } else if (m == 0xC4) {
            size_t s = 0;
            while (s < len) {
                const int tc = seg[s] >> 4, th = seg[s] & 15;
                if (tc > 1 || th > 3 || len - s < 17) return FEAR_TRAIN_ERR_FORMAT;
                int total = 0;
                for (int i = 1; i <= 16; ++i) total += seg[s + i];
                if (total > 256 || len - s - 17 < (size_t)total) return FEAR_TRAIN_ERR_FORMAT;
                if (!huffman_build(tc ? pg.ac[th] : pg.dc[th], seg + s + 1, seg + s + 17, total)) return FEAR_TRAIN_ERR_FORMAT;
                s += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {
            if (pg.scans) return FEAR_TRAIN_ERR_UNSUPPORTED;              // libjpeg latches the tables per component; nobody writes them late
            size_t s = 0;
            while (s < len) {
                const int pq = seg[s] >> 4, tq = seg[s] & 15;
                if (pq == 1) return FEAR_TRAIN_ERR_UNSUPPORTED;
                if (pq > 1 || tq > 3 || len - s < 65) return FEAR_TRAIN_ERR_FORMAT;
                for (int i = 0; i < 64; ++i) {
                    pg.q[tq][kZigzag[i]] = seg[s + 1 + i];
                    pg.q_file[tq][i] = seg[s + 1 + i];
                }
                pg.q_defined[tq] = true;
                s += 65;
            }
        } else if (m == 0xDD) {
            if (len != 2) return FEAR_TRAIN_ERR_FORMAT;
            pg.restart = seg[0] << 8 | seg[1];
        } else if (m == 0xDC) {
            return FEAR_TRAIN_ERR_UNSUPPORTED;                            // DNL
        } else if (m == 0xE0) {
            if (pg.scans == 0 && len >= 5 && std::memcmp(seg, "JFIF", 5) == 0) { pg.jfif_at = seg_at; pg.jfif_len = L + 2; }
        } else if (m == 0xEE) {
            if (pg.scans == 0 && len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) {
                pg.adobe = seg[11];
                pg.adobe_at = seg_at;
                pg.adobe_len = L + 2;
            }
        } else if (m == 0xDA) {
            if (!sof) return FEAR_TRAIN_ERR_FORMAT;
            if (len < 1 || seg[0] == 0 || seg[0] > 4) return FEAR_TRAIN_ERR_FORMAT;
            const int ns = seg[0];
            if (ns > nf || len != 4 + 2 * (size_t)ns) return FEAR_TRAIN_ERR_FORMAT;
            if (pg.scans == kMaxScans) return FEAR_TRAIN_ERR_UNSUPPORTED;
            int comp[3], td[3], ta[3];
            for (int i = 0; i < ns; ++i) {
                const int cs = seg[1 + 2 * i], t = seg[2 + 2 * i];
                int c = i ? comp[i - 1] + 1 : 0;                          // a subset of the frame's, in frame order
                while (c < nf && pg.ids[c] != cs) ++c;
                if (c >= nf) return FEAR_TRAIN_ERR_FORMAT;
                if ((t >> 4) > 3 || (t & 15) > 3) return FEAR_TRAIN_ERR_FORMAT;
                comp[i] = c;
                td[i] = t >> 4;
                ta[i] = t & 15;
            }
            const uint8_t* tail = seg + 1 + 2 * ns;
            const int Ss = tail[0], Se = tail[1], Ah = tail[2] >> 4, Al = tail[2] & 15;
            if (Ss == 0 ? Se != 0 : (ns != 1 || Se < Ss || Se > 63)) return FEAR_TRAIN_ERR_FORMAT;
            if (Al > 13 || (Ah != 0 && Ah != Al + 1)) return FEAR_TRAIN_ERR_FORMAT;
            if (pg.scans == 0) {
                if (nf == 3 && pg.adobe == 0) return FEAR_TRAIN_ERR_UNSUPPORTED;  // RGB samples
                for (int i = 0; i < nf; ++i) {
                    if (!pg.q_defined[pg.tq[i]]) return FEAR_TRAIN_ERR_FORMAT;
                    std::memcpy(info.qt[i], pg.q[pg.tq[i]], sizeof(info.qt[i]));
                }
            }
            for (int i = 0; i < ns; ++i) {
                if (Ss == 0 && Ah == 0 && !pg.dc[td[i]].defined) return FEAR_TRAIN_ERR_FORMAT;
                if (Ss > 0 && !pg.ac[ta[i]].defined) return FEAR_TRAIN_ERR_FORMAT;
            }
            for (int i = 0; i < ns; ++i) {                                // the progression, as libjpeg's coef_bits tracks it
                int8_t* cb = pg.coef_bits[comp[i]];
                if (Ss > 0 && cb[0] < 0) return FEAR_TRAIN_ERR_UNSUPPORTED;
                for (int k = Ss; k <= Se; ++k) {
                    if (Ah == 0 ? cb[k] >= 0 : cb[k] != Ah) return FEAR_TRAIN_ERR_UNSUPPORTED;
                    cb[k] = (int8_t)Al;
                }
            }
            if (headers_only) return FEAR_TRAIN_OK;
            if (pg.scans == 0) {
                try {
                    pg.coef.assign((size_t)info.total_blocks * 64, 0);
                } catch (const std::bad_alloc&) {
                    return FEAR_TRAIN_ERR_WORKSPACE;
                }
            }
            ++pg.scans;
            const int rc = progressive_scan(d, n, p, pg, ns, comp, td, ta, Ss, Se, Ah, Al);
            if (rc != FEAR_TRAIN_OK) return rc;
        }
        // the other APPn, COM and the reserved markers carry nothing the decoder needs
    }
    for (int c = 0; c < nf; ++c)
        for (int k = 0; k < 64; ++k)
            if (pg.coef_bits[c][k] != 0) return FEAR_TRAIN_ERR_UNSUPPORTED;      // incomplete: libjpeg would smooth the blocks
    return FEAR_TRAIN_OK;
}

inline int bit_length(int v) {
    int t = 0;
    while (v) { ++t; v >>= 1; }
    return t;
}

// The coefficients as the symbols of one interleaved baseline scan with a restart after every MCU row.  sink.put(ac, table, symbol, bits,
// value) per code, sink.restart(k) in front of every MCU row but the first.  FEAR_TRAIN_ERR_UNSUPPORTED for a value the baseline
// alphabet lacks: an AC term outside +-1023, a DC difference outside +-2047.
template <class Sink>
int baseline_walk(const Progressive& pg, Sink& sink) {
    const FearJpegInfo& in = pg.info;
    for (int my = 0; my < in.mcus_y; ++my) {
        int pred[3] = {0, 0, 0};
        if (my) sink.restart((my - 1) & 7);
        for (int mx = 0; mx < in.mcus_x; ++mx)
            for (int c = 0; c < pg.nf; ++c)
                for (int j = 0; j < in.v[c]; ++j)
                    for (int i = 0; i < in.h[c]; ++i) {
                        const int16_t* blk = pg.coef.data() + ((size_t)pg.comp_first[c] + (size_t)(my * in.v[c] + j) * (size_t)in.blocks_w[c] + (size_t)(mx * in.h[c] + i)) * 64;
                        const int t = c ? 1 : 0, diff = blk[0] - pred[c];
                        pred[c] = blk[0];
                        if (diff < -2047 || diff > 2047) return FEAR_TRAIN_ERR_UNSUPPORTED;
                        const int cat = bit_length(diff < 0 ? -diff : diff);
                        sink.put(0, t, cat, cat, diff < 0 ? diff - 1 : diff);
                        int r = 0;
                        for (int k = 1; k < 64; ++k) {
                            const int v = blk[k];
                            if (v == 0) { ++r; continue; }
                            if (v < -1023 || v > 1023) return FEAR_TRAIN_ERR_UNSUPPORTED;
                            for (; r > 15; r -= 16) sink.put(1, t, 0xF0, 0, 0);
                            const int s = bit_length(v < 0 ? -v : v);
                            sink.put(1, t, r << 4 | s, s, v < 0 ? v - 1 : v);
                            r = 0;
                        }
                        if (r > 0) sink.put(1, t, 0, 0, 0);
                    }
    }
    return FEAR_TRAIN_OK;
}

struct SymbolCount {
    uint32_t freq[2][2][257];
    void put(int ac, int t, int symbol, int, int) { ++freq[ac][t][symbol]; }
    void restart(int) {}
};

// T.81 K.2, as libjpeg's jpeg_gen_optimal_table states it: code lengths from the counts (symbol 256 is reserved so that no code is all
// ones), limited to 16 bits, the symbols sorted by length and value.  `freq` is consumed.
inline void optimal_table(uint32_t* freq, uint8_t* counts16, uint8_t* values, int* total) {
    int bits[258], codesize[257], others[257];
    std::memset(bits, 0, sizeof(bits));
    std::memset(codesize, 0, sizeof(codesize));
    for (int i = 0; i < 257; ++i) others[i] = -1;
    freq[256] = 1;
    for (;;) {
        int c1 = -1, c2 = -1;
        uint32_t v = 0xFFFFFFFFu;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v) { v = freq[i]; c1 = i; }
        v = 0xFFFFFFFFu;
        for (int i = 0; i <= 256; ++i)
            if (freq[i] && freq[i] <= v && i != c1) { v = freq[i]; c2 = i; }
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (++codesize[c1]; others[c1] >= 0;) { c1 = others[c1]; ++codesize[c1]; }
        others[c1] = c2;
        for (++codesize[c2]; others[c2] >= 0;) { c2 = others[c2]; ++codesize[c2]; }
    }
    for (int i = 0; i <= 256; ++i)
        if (codesize[i]) ++bits[codesize[i]];
    for (int i = 257; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2;
            ++bits[i - 1];
            bits[j + 1] += 2;
            --bits[j];
        }
    int last = 16;
    while (bits[last] == 0) --last;
    --bits[last];                                                         // the reserved symbol's code
    for (int i = 1; i <= 16; ++i) counts16[i - 1] = (uint8_t)bits[i];
    int k = 0;
    for (int len = 1; len <= 256; ++len)
        for (int j = 0; j < 256; ++j)
            if (codesize[j] == len) values[k++] = (uint8_t)j;
    *total = k;
}

struct BaselineWriter {
    uint8_t* out;
    size_t cap, at = 0;
    bool full = false;
    uint64_t acc = 0;
    int have = 0;
    uint16_t code[2][2][256];
    uint8_t size[2][2][256];

    void byte(int b) {
        if (at < cap) out[at++] = (uint8_t)b;
        else full = true;
    }
    void bytes(const uint8_t* src, size_t count) {
        for (size_t i = 0; i < count; ++i) byte(src[i]);
    }
    void word(int v) { byte(v >> 8); byte(v & 255); }
    void push(uint32_t v, int k) {                                        // 0 <= k <= 16
        acc = acc << k | (v & ((1u << k) - 1));
        have += k;
        while (have >= 8) {
            const int b = (int)(acc >> (have - 8)) & 255;
            byte(b);
            if (b == 0xFF) byte(0);
            have -= 8;
        }
    }
    void flush() {
        if (have) push(0xFF, 8 - have);                                   // ones up to the byte boundary
    }
    void put(int ac, int t, int symbol, int k, int value) {
        push(code[ac][t][symbol], size[ac][t][symbol]);
        push((uint32_t)value, k);
    }
    void restart(int k) {
        flush();
        byte(0xFF);
        byte(0xD0 + k);
    }
    void table(int ac, int t, const uint8_t* counts16, const uint8_t* values, int total) {
        byte(0xFF); byte(0xC4);
        word(2 + 1 + 16 + total);
        byte(ac << 4 | t);
        bytes(counts16, 16);
        bytes(values, (size_t)total);
        int c = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < counts16[len - 1]; ++i, ++k) {
                code[ac][t][values[k]] = (uint16_t)c++;
                size[ac][t][values[k]] = (uint8_t)len;
            }
            c <<= 1;
        }
    }
};

// The walk's verdict alone: what fear_jpeg_progressive_decode shares with fear_jpeg_progressive_to_baseline.
struct NoSink {
    void put(int, int, int, int, int) {}
    void restart(int) {}
};

}  // namespace fear_jpeg

extern "C" {

int fear_jpeg_progressive_parse(const uint8_t* data, size_t n, FearJpegInfo* info) {
    if (!data || !info) return FEAR_TRAIN_ERR_NULL;
    fear_jpeg::Progressive* pg = new (std::nothrow) fear_jpeg::Progressive();
    if (!pg) return FEAR_TRAIN_ERR_WORKSPACE;
    const int rc = fear_jpeg::progressive_run(data, n, *pg, true);
    if (rc == FEAR_TRAIN_OK) *info = pg->info;
    delete pg;
    return rc;
}

int fear_jpeg_progressive_decode(const uint8_t* data, size_t n, const FearJpegInfo* info, int16_t* coef, size_t coef_cap, uint32_t* block_start,
                                 size_t* coef_used) {
    using namespace fear_jpeg;
    if (!data || !info || !coef || !block_start || !coef_used) return FEAR_TRAIN_ERR_NULL;
    Progressive* pg = new (std::nothrow) Progressive();
    if (!pg) return FEAR_TRAIN_ERR_WORKSPACE;
    struct Guard { Progressive* p; ~Guard() { delete p; } } guard{pg};
    int rc = progressive_run(data, n, *pg, true);
    if (rc != FEAR_TRAIN_OK) return rc;
    if (std::memcmp(&pg->info, info, sizeof(*info)) != 0) return FEAR_TRAIN_ERR_SHAPE;   // `info` is not this file's
    *pg = Progressive();
    rc = progressive_run(data, n, *pg, false);
    if (rc != FEAR_TRAIN_OK) return rc;
    NoSink none;
    rc = baseline_walk(*pg, none);
    if (rc != FEAR_TRAIN_OK) return rc;
    const uint32_t total = pg->info.total_blocks;
    size_t at = 0;
    for (uint32_t b = 0; b < total; ++b) {
        const int16_t* blk = pg->coef.data() + (size_t)b * 64;
        int last = 63;
        while (last > 0 && blk[last] == 0) --last;
        if ((size_t)last + 1 > coef_cap - at) return FEAR_TRAIN_ERR_WORKSPACE;
        block_start[b] = (uint32_t)at;
        std::memcpy(coef + at, blk, ((size_t)last + 1) * sizeof(int16_t));
        at += (size_t)last + 1;
    }
    block_start[total] = (uint32_t)at;
    *coef_used = at;
    return FEAR_TRAIN_OK;
}

size_t fear_jpeg_baseline_bound(const FearJpegInfo* info) {
    // two copied APPn segments, the tables and headers; per block 27 + 63 * 26 + 16 bits, every byte stuffed; padding and a marker per row
    return info ? (size_t)2 * 65537 + 2048 + (size_t)info->total_blocks * 512 + (size_t)info->mcus_y * 4 : 0;
}

int fear_jpeg_progressive_to_baseline(const uint8_t* data, size_t n, uint8_t* out, size_t out_cap, size_t* out_used) {
    using namespace fear_jpeg;
    if (!data || !out || !out_used) return FEAR_TRAIN_ERR_NULL;
    Progressive* pg = new (std::nothrow) Progressive();
    SymbolCount* count = new (std::nothrow) SymbolCount();
    BaselineWriter* w = new (std::nothrow) BaselineWriter();
    struct Guard { Progressive* p; SymbolCount* c; BaselineWriter* w; ~Guard() { delete p; delete c; delete w; } } guard{pg, count, w};
    if (!pg || !count || !w) return FEAR_TRAIN_ERR_WORKSPACE;
    int rc = progressive_run(data, n, *pg, false);
    if (rc != FEAR_TRAIN_OK) return rc;
    std::memset(count->freq, 0, sizeof(count->freq));
    rc = baseline_walk(*pg, *count);
    if (rc != FEAR_TRAIN_OK) return rc;
    const FearJpegInfo& in = pg->info;
    const int nf = pg->nf;
    w->out = out;
    w->cap = out_cap;
    w->byte(0xFF); w->byte(0xD8);
    if (pg->jfif_len) w->bytes(data + pg->jfif_at, pg->jfif_len);
    if (pg->adobe_len) w->bytes(data + pg->adobe_at, pg->adobe_len);
    for (int c = 0; c < nf; ++c) {                                        // every quantiser table a component selects, once
        bool seen = false;
        for (int j = 0; j < c; ++j) seen = seen || pg->tq[j] == pg->tq[c];
        if (seen) continue;
        w->byte(0xFF); w->byte(0xDB);
        w->word(67);
        w->byte(pg->tq[c]);
        w->bytes(pg->q_file[pg->tq[c]], 64);
    }
    w->byte(0xFF); w->byte(0xC0);
    w->word(8 + 3 * nf);
    w->byte(8);
    w->word(in.height);
    w->word(in.width);
    w->byte(nf);
    for (int c = 0; c < nf; ++c) { w->byte(pg->ids[c]); w->byte(pg->hv[c]); w->byte(pg->tq[c]); }
    for (int t = 0; t < (nf == 3 ? 2 : 1); ++t)
        for (int ac = 0; ac < 2; ++ac) {
            uint8_t counts16[16], values[256];
            int total = 0;
            optimal_table(count->freq[ac][t], counts16, values, &total);
            w->table(ac, t, counts16, values, total);
        }
    w->byte(0xFF); w->byte(0xDD);
    w->word(4);
    w->word(in.mcus_x);
    w->byte(0xFF); w->byte(0xDA);
    w->word(6 + 2 * nf);
    w->byte(nf);
    for (int c = 0; c < nf; ++c) { w->byte(pg->ids[c]); w->byte(c ? 0x11 : 0x00); }
    w->byte(0); w->byte(63); w->byte(0);
    baseline_walk(*pg, *w);
    w->flush();
    w->byte(0xFF); w->byte(0xD9);
    if (w->full) return FEAR_TRAIN_ERR_WORKSPACE;
    *out_used = w->at;
    return FEAR_TRAIN_OK;
}

}  // extern "C"

#endif  // FEAR_JPEG_PROGRESSIVE_H
