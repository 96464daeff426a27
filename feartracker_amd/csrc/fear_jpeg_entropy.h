// fear_jpeg_entropy.h — the host half of the JPEG frame decoder (include/fear_train.h): the segment parser and the
// Huffman stage of baseline sequential JPEG (ITU-T T.81 annex B and F.2).  Plain C++17: neither HIP nor the GPU is touched, so the file
// also compiles stand-alone (tools/jpeg_entropy_host.cpp builds it with the address and undefined-behaviour sanitizers).
//
// Written for hostile input: every read is checked against the buffer's length, every write against the caller's capacity, every Huffman
// table is validated as it is built (at most 256 symbols, no over-subscribed code length), and no loop runs further than the frame header's
// block counts or the 64 coefficients of a block allow.  jpeg_frames._parse / jpeg_coefficients_host restate it in Python check for check;
// tests/test_jpeg_decode_host.py holds the two to the same verdict on every prefix and every flipped byte of a file.
//
// Included by fear_train.hip behind fear_train_jpeg.h.
#ifndef FEAR_JPEG_ENTROPY_H
#define FEAR_JPEG_ENTROPY_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/fear_train.h"
#include "fear_jpeg_tables.h"                                  // kZigzag

namespace fear_jpeg {

constexpr int kLookBits = 9;

struct Huffman {
    bool defined = false;
    uint8_t counts[17];            // codes of each length 1..16
    uint8_t values[256];
    int32_t first[17], index[17];  // the first code of a length and its place in `values`
    uint16_t look[1 << kLookBits]; // (length << 8 | symbol) for codes of at most kLookBits bits, 0 otherwise
};

struct Header {
    FearJpegInfo info;
    Huffman dc[4], ac[4];
    bool q_defined[4] = {false, false, false, false};
    uint16_t q[4][64];             // natural order
    uint8_t ids[3], tq[3], td[3], ta[3];
    int adobe = -1;                // the transform byte of an Adobe APP14 segment
    size_t scan = 0;               // the first byte of the entropy-coded segment
};

// One table of a DHT segment; `values` holds `total` symbols.  False for an over-subscribed code length.
inline bool huffman_build(Huffman& t, const uint8_t* counts16, const uint8_t* values, int total) {
    t.counts[0] = 0;
    std::memcpy(t.counts + 1, counts16, 16);
    std::memcpy(t.values, values, (size_t)total);
    std::memset(t.look, 0, sizeof(t.look));
    int32_t code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.first[len] = code;
        t.index[len] = k;
        const int32_t cnt = t.counts[len];
        if (code + cnt > (1 << len)) return false;
        if (len <= kLookBits)
            for (int32_t c = 0; c < cnt; ++c) {
                const uint16_t entry = (uint16_t)(len << 8 | t.values[k + c]);
                const int32_t base = (code + c) << (kLookBits - len);
                for (int32_t f = 0; f < (1 << (kLookBits - len)); ++f) t.look[base + f] = entry;
            }
        code = (code + cnt) << 1;
        k += cnt;
    }
    t.defined = true;
    return true;
}

// The segments up to and including SOS.
inline int parse(const uint8_t* d, size_t n, Header& hd) {
    if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) return FEAR_TRAIN_ERR_FORMAT;
    FearJpegInfo& info = hd.info;
    std::memset(&info, 0, sizeof(info));
    bool sof = false;
    int nf = 0;
    size_t p = 2;
    for (;;) {
        if (p >= n || d[p] != 0xFF) return FEAR_TRAIN_ERR_FORMAT;
        while (p < n && d[p] == 0xFF) ++p;                                // fill bytes
        if (p >= n) return FEAR_TRAIN_ERR_FORMAT;
        const int m = d[p++];
        if (m == 0x01) continue;                                          // TEM stands alone
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD9)) return FEAR_TRAIN_ERR_FORMAT;
        if (n - p < 2) return FEAR_TRAIN_ERR_FORMAT;
        const size_t L = (size_t)d[p] << 8 | d[p + 1];
        if (L < 2 || L > n - p) return FEAR_TRAIN_ERR_FORMAT;
        const uint8_t* seg = d + p + 2;
        const size_t len = L - 2;
        p += L;
        if (m == 0xC0) {
            if (sof || len < 6) return FEAR_TRAIN_ERR_FORMAT;
            if (seg[0] != 8) return FEAR_TRAIN_ERR_UNSUPPORTED;
            info.height = seg[1] << 8 | seg[2];
            info.width = seg[3] << 8 | seg[4];
            nf = seg[5];
            if (info.width == 0) return FEAR_TRAIN_ERR_FORMAT;
            if (info.height == 0) return FEAR_TRAIN_ERR_UNSUPPORTED;      // the height comes in a DNL segment
            if (info.width > FEAR_JPEG_MAX_SIDE || info.height > FEAR_JPEG_MAX_SIDE) return FEAR_TRAIN_ERR_UNSUPPORTED;
            if (nf == 0) return FEAR_TRAIN_ERR_FORMAT;
            if (nf != 1 && nf != 3) return FEAR_TRAIN_ERR_UNSUPPORTED;
            if (len != 6 + 3 * (size_t)nf) return FEAR_TRAIN_ERR_FORMAT;
            for (int i = 0; i < nf; ++i) {
                const uint8_t* c = seg + 6 + 3 * i;
                const int h = c[1] >> 4, v = c[1] & 15;
                if (h < 1 || h > 4 || v < 1 || v > 4 || c[2] > 3) return FEAR_TRAIN_ERR_FORMAT;
                for (int j = 0; j < i; ++j)
                    if (hd.ids[j] == c[0]) return FEAR_TRAIN_ERR_FORMAT;
                hd.ids[i] = c[0];
                info.h[i] = h;
                info.v[i] = v;
                hd.tq[i] = c[2];
            }
            if (nf == 1) {
                info.h[0] = info.v[0] = 1;                                // not interleaved: the sampling factors mean nothing
            } else {
                const int h = info.h[0], v = info.v[0];
                const bool luma_ok = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma_ok || info.h[1] != 1 || info.v[1] != 1 || info.h[2] != 1 || info.v[2] != 1) return FEAR_TRAIN_ERR_UNSUPPORTED;
            }
            info.components = nf;
            sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            return FEAR_TRAIN_ERR_UNSUPPORTED;                            // the other frame kinds, JPG, arithmetic conditioning
        } else if (m == 0xC4) {
            size_t s = 0;
            while (s < len) {
                const int tc = seg[s] >> 4, th = seg[s] & 15;
                if (tc > 1 || th > 3 || len - s < 17) return FEAR_TRAIN_ERR_FORMAT;
                int total = 0;
                for (int i = 1; i <= 16; ++i) total += seg[s + i];
                if (total > 256 || len - s - 17 < (size_t)total) return FEAR_TRAIN_ERR_FORMAT;
                if (!huffman_build(tc ? hd.ac[th] : hd.dc[th], seg + s + 1, seg + s + 17, total)) return FEAR_TRAIN_ERR_FORMAT;
                s += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {
            size_t s = 0;
            while (s < len) {
                const int pq = seg[s] >> 4, tq = seg[s] & 15;
                if (pq == 1) return FEAR_TRAIN_ERR_UNSUPPORTED;           // 16-bit table
                if (pq > 1 || tq > 3 || len - s < 65) return FEAR_TRAIN_ERR_FORMAT;
                for (int i = 0; i < 64; ++i) hd.q[tq][kZigzag[i]] = seg[s + 1 + i];
                hd.q_defined[tq] = true;
                s += 65;
            }
        } else if (m == 0xDD) {
            if (len != 2) return FEAR_TRAIN_ERR_FORMAT;
            info.restart_interval = seg[0] << 8 | seg[1];
        } else if (m == 0xDC) {
            return FEAR_TRAIN_ERR_UNSUPPORTED;                            // DNL
        } else if (m == 0xEE) {
            if (len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) hd.adobe = seg[11];
        } else if (m == 0xDA) {
            if (!sof) return FEAR_TRAIN_ERR_FORMAT;
            if (len < 1 || seg[0] == 0 || seg[0] > 4) return FEAR_TRAIN_ERR_FORMAT;
            if (seg[0] != nf) return FEAR_TRAIN_ERR_UNSUPPORTED;          // part of the components: a second scan follows
            if (len != 4 + 2 * (size_t)nf) return FEAR_TRAIN_ERR_FORMAT;
            for (int i = 0; i < nf; ++i) {
                const int cs = seg[1 + 2 * i], t = seg[2 + 2 * i];
                if (cs != hd.ids[i]) {
                    for (int j = 0; j < nf; ++j)
                        if (hd.ids[j] == cs) return FEAR_TRAIN_ERR_UNSUPPORTED;   // out of frame order
                    return FEAR_TRAIN_ERR_FORMAT;
                }
                if ((t >> 4) > 3 || (t & 15) > 3) return FEAR_TRAIN_ERR_FORMAT;
                hd.td[i] = (uint8_t)(t >> 4);
                hd.ta[i] = (uint8_t)(t & 15);
            }
            const uint8_t* tail = seg + 1 + 2 * nf;
            if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return FEAR_TRAIN_ERR_FORMAT;
            if (nf == 3 && hd.adobe == 0) return FEAR_TRAIN_ERR_UNSUPPORTED;      // RGB samples
            for (int i = 0; i < nf; ++i)
                if (!hd.q_defined[hd.tq[i]] || !hd.dc[hd.td[i]].defined || !hd.ac[hd.ta[i]].defined) return FEAR_TRAIN_ERR_FORMAT;
            hd.scan = p;
            break;
        }
        // APPn, COM and the reserved markers carry nothing the decoder needs
    }
    info.mcus_x = (info.width + 8 * info.h[0] - 1) / (8 * info.h[0]);
    info.mcus_y = (info.height + 8 * info.v[0] - 1) / (8 * info.v[0]);
    uint32_t total = 0;
    for (int i = 0; i < nf; ++i) {
        info.blocks_w[i] = info.mcus_x * info.h[i];
        info.blocks_h[i] = info.mcus_y * info.v[i];
        total += (uint32_t)info.blocks_w[i] * (uint32_t)info.blocks_h[i];
        std::memcpy(info.qt[i], hd.q[hd.tq[i]], sizeof(info.qt[i]));
    }
    info.total_blocks = total;                                            // at most 3 * 1024 * 1024
    return FEAR_TRAIN_OK;
}

// The entropy-coded segment as a bit stream: FF 00 is a data byte FF, any other FF xx ends the data.  `acc` holds `have` bits that are
// really there; a peek past them reads zeros, and taking more than `have` is the truncation error — so the verdict is that of a reader
// that fetches a byte only when it needs one, whatever the look-ahead.
struct Bits {
    const uint8_t* d;
    size_t n, pos;
    uint64_t acc = 0;
    int have = 0;

    void fill() {
        while (have <= 56 && pos < n) {
            const uint8_t b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= n || d[pos + 1] != 0) return;              // a marker, or the file ends inside one
                pos += 2;
            } else {
                pos += 1;
            }
            acc = acc << 8 | b;
            have += 8;
        }
    }
    uint32_t peek(int k) const {                                          // 1 <= k <= 16
        const uint64_t mask = (1u << k) - 1;
        return (uint32_t)((have >= k ? acc >> (have - k) : acc << (k - have)) & mask);
    }
    bool take(int k) {
        if (k > have) return false;
        have -= k;
        return true;
    }
    // 0..255, or -1: a code in no table, or the data ends inside the code
    int symbol(const Huffman& t) {
        if (have < 16) fill();
        const uint16_t e = t.look[peek(kLookBits)];
        if (e) return take(e >> 8) ? (e & 255) : -1;
        for (int len = kLookBits + 1; len <= 16; ++len) {
            const int32_t k = (int32_t)peek(len) - t.first[len];
            if (k >= 0 && k < t.counts[len]) return take(len) ? t.values[t.index[len] + k] : -1;
        }
        return -1;
    }
    // `k` bits extended to a signed value (T.81 F.2.2.1); false when the data ends first.  0 <= k <= 15
    bool receive(int k, int* out) {
        if (k == 0) { *out = 0; return true; }
        if (have < k) fill();
        const int v = (int)peek(k);
        if (!take(k)) return false;
        *out = v >= (1 << (k - 1)) ? v : v - (1 << k) + 1;
        return true;
    }
    // The rest of the byte is padding and the marker RST`expected` follows at once.
    bool restart(int expected) {
        have -= have & 7;
        if (have != 0) return false;                                      // whole data bytes in front of the marker
        acc = 0;
        if (n - pos < 2 || d[pos] != 0xFF || d[pos + 1] != 0xD0 + expected) return false;
        pos += 2;
        return true;
    }
};

}  // namespace fear_jpeg

extern "C" {

int fear_jpeg_parse(const uint8_t* data, size_t n, FearJpegInfo* info) {
    if (!data || !info) return FEAR_TRAIN_ERR_NULL;
    fear_jpeg::Header* hd = new (std::nothrow) fear_jpeg::Header();
    if (!hd) return FEAR_TRAIN_ERR_WORKSPACE;
    const int rc = fear_jpeg::parse(data, n, *hd);
    if (rc == FEAR_TRAIN_OK) *info = hd->info;
    delete hd;
    return rc;
}

size_t fear_jpeg_packed_bound(const FearJpegInfo* info) {
    return info ? (size_t)info->total_blocks * 64 : 0;
}

int fear_jpeg_entropy_decode(const uint8_t* data, size_t n, const FearJpegInfo* info, int16_t* coef, size_t coef_cap, uint32_t* block_start,
                             size_t* coef_used) {
    using namespace fear_jpeg;
    if (!data || !info || !coef || !block_start || !coef_used) return FEAR_TRAIN_ERR_NULL;
    Header* hd = new (std::nothrow) Header();
    if (!hd) return FEAR_TRAIN_ERR_WORKSPACE;
    struct Guard { Header* h; ~Guard() { delete h; } } guard{hd};
    const int rc = parse(data, n, *hd);
    if (rc != FEAR_TRAIN_OK) return rc;
    const FearJpegInfo& in = hd->info;
    if (std::memcmp(&in, info, sizeof(in)) != 0) return FEAR_TRAIN_ERR_SHAPE;     // `info` is not this file's
    const int nf = in.components;
    const uint32_t total = in.total_blocks;
    // the scan interleaves the components; the packed output does not: decode in scan order, then gather component by component
    std::vector<int16_t> scan;
    std::vector<uint32_t> where, count;
    try {
        scan.reserve((size_t)total * 8);
        where.resize(total);
        count.resize(total);
    } catch (const std::bad_alloc&) {
        return FEAR_TRAIN_ERR_WORKSPACE;
    }
    uint32_t comp_first[3] = {0, 0, 0};
    for (int c = 1; c < nf; ++c) comp_first[c] = comp_first[c - 1] + (uint32_t)in.blocks_w[c - 1] * (uint32_t)in.blocks_h[c - 1];
    Bits bits{data, n, hd->scan};
    int pred[3] = {0, 0, 0};
    const int n_mcu = in.mcus_x * in.mcus_y;
    int mx = 0, my = 0, to_restart = in.restart_interval, next_rst = 0;
    int16_t block[64];
    for (int mcu = 0; mcu < n_mcu; ++mcu) {
        if (in.restart_interval && mcu) {
            if (to_restart == 0) {
                if (!bits.restart(next_rst)) return FEAR_TRAIN_ERR_FORMAT;
                next_rst = (next_rst + 1) & 7;
                to_restart = in.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
        }
        --to_restart;
        for (int c = 0; c < nf; ++c) {
            const Huffman& dc = hd->dc[hd->td[c]];
            const Huffman& ac = hd->ac[hd->ta[c]];
            for (int j = 0; j < in.v[c]; ++j)
                for (int i = 0; i < in.h[c]; ++i) {
                    const int t = bits.symbol(dc);
                    if (t < 0 || t > 15) return FEAR_TRAIN_ERR_FORMAT;
                    int diff;
                    if (!bits.receive(t, &diff)) return FEAR_TRAIN_ERR_FORMAT;
                    pred[c] = (int16_t)(uint16_t)(pred[c] + diff);                // JCOEF is 16 bits wide
                    block[0] = (int16_t)pred[c];
                    int k = 1, last = 0;
                    while (k < 64) {
                        const int rs = bits.symbol(ac);
                        if (rs < 0) return FEAR_TRAIN_ERR_FORMAT;
                        const int r = rs >> 4, s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;                                   // EOB
                            if (k + 16 > 63) return FEAR_TRAIN_ERR_FORMAT;        // ZRL: a coefficient follows
                            for (int z = 0; z < 16; ++z) block[k + z] = 0;
                            k += 16;
                            continue;
                        }
                        if (k + r > 63) return FEAR_TRAIN_ERR_FORMAT;
                        for (int z = 0; z < r; ++z) block[k + z] = 0;
                        k += r;
                        int v;
                        if (!bits.receive(s, &v)) return FEAR_TRAIN_ERR_FORMAT;
                        block[k] = (int16_t)v;
                        if (v != 0) last = k;
                        ++k;
                    }
                    const uint32_t b = comp_first[c] + (uint32_t)(my * in.v[c] + j) * (uint32_t)in.blocks_w[c] + (uint32_t)(mx * in.h[c] + i);
                    where[b] = (uint32_t)scan.size();
                    count[b] = (uint32_t)last + 1;
                    try {
                        scan.insert(scan.end(), block, block + last + 1);
                    } catch (const std::bad_alloc&) {
                        return FEAR_TRAIN_ERR_WORKSPACE;
                    }
                }
        }
        if (++mx == in.mcus_x) { mx = 0; ++my; }
    }
    if (scan.size() > coef_cap) return FEAR_TRAIN_ERR_WORKSPACE;
    uint32_t at = 0;
    for (uint32_t b = 0; b < total; ++b) {
        block_start[b] = at;
        std::memcpy(coef + at, scan.data() + where[b], count[b] * sizeof(int16_t));
        at += count[b];
    }
    block_start[total] = at;
    *coef_used = at;
    return FEAR_TRAIN_OK;
}

// The scan for the device's Huffman stage (fear_jpeg_huffman.h): the entropy-coded bytes without their stuffing, split at the restart
// markers, and the tables the scan's components select.  One pass at memchr's speed; nothing is decoded.
int fear_jpeg_scan_prepare(const uint8_t* data, size_t n, const FearJpegInfo* info, uint8_t* bytes_out, size_t bytes_cap,
                           uint32_t* seg_start, size_t seg_cap, FearJpegScan* scan) {
    using namespace fear_jpeg;
    if (!data || !info || !bytes_out || !seg_start || !scan) return FEAR_TRAIN_ERR_NULL;
    Header* hd = new (std::nothrow) Header();
    if (!hd) return FEAR_TRAIN_ERR_WORKSPACE;
    struct Guard { Header* h; ~Guard() { delete h; } } guard{hd};
    const int rc = parse(data, n, *hd);
    if (rc != FEAR_TRAIN_OK) return rc;
    const FearJpegInfo& in = hd->info;
    if (std::memcmp(&in, info, sizeof(in)) != 0) return FEAR_TRAIN_ERR_SHAPE;     // `info` is not this file's
    if (n - hd->scan > 0xFFFFFFFFu) return FEAR_TRAIN_ERR_UNSUPPORTED;            // the offsets are 32 bits wide
    const uint32_t n_mcu = (uint32_t)in.mcus_x * (uint32_t)in.mcus_y;
    const uint32_t want = in.restart_interval ? (n_mcu + (uint32_t)in.restart_interval - 1) / (uint32_t)in.restart_interval : 1;
    if (seg_cap < (size_t)want + 1) return FEAR_TRAIN_ERR_WORKSPACE;
    size_t p = hd->scan, out = 0;
    uint32_t seg = 0, longest = 0;
    seg_start[0] = 0;
    for (;;) {
        const void* ff = p < n ? std::memchr(data + p, 0xFF, n - p) : nullptr;
        const size_t q = ff ? (size_t)(static_cast<const uint8_t*>(ff) - data) : n;
        if (q - p > bytes_cap - out) return FEAR_TRAIN_ERR_WORKSPACE;
        if (q > p) std::memcpy(bytes_out + out, data + p, q - p);
        out += q - p;
        if (q + 1 >= n) break;                                            // the file ends, perhaps inside a marker
        const int m = data[q + 1];
        if (m == 0) {                                                     // a stuffed FF
            if (out >= bytes_cap) return FEAR_TRAIN_ERR_WORKSPACE;
            bytes_out[out++] = 0xFF;
            p = q + 2;
            continue;
        }
        if (seg + 1 == want) break;                                       // any marker ends the last segment
        if (m != 0xD0 + (int)(seg & 7)) return FEAR_TRAIN_ERR_FORMAT;
        if ((uint32_t)out - seg_start[seg] > longest) longest = (uint32_t)out - seg_start[seg];
        seg_start[++seg] = (uint32_t)out;
        p = q + 2;
    }
    if (seg + 1 != want) return FEAR_TRAIN_ERR_FORMAT;                    // a restart marker is missing
    if ((uint32_t)out - seg_start[seg] > longest) longest = (uint32_t)out - seg_start[seg];
    seg_start[want] = (uint32_t)out;
    std::memset(scan, 0, sizeof(*scan));
    scan->n_bytes = (uint32_t)out;
    scan->n_seg = want;
    scan->max_seg_bytes = longest;
    scan->total_blocks = in.total_blocks;
    scan->components = in.components;
    scan->h = in.h[0];
    scan->v = in.v[0];
    scan->mcus_x = in.mcus_x;
    scan->mcus_y = in.mcus_y;
    scan->restart_interval = in.restart_interval;
    for (int c = 0; c < in.components; ++c)
        for (int k = 0; k < 2; ++k) {
            const Huffman& t = k ? hd->ac[hd->ta[c]] : hd->dc[hd->td[c]];
            FearJpegHuff& o = k ? scan->ac[c] : scan->dc[c];
            std::memcpy(o.look, t.look, sizeof(o.look));
            std::memcpy(o.values, t.values, sizeof(o.values));
            std::memcpy(o.counts, t.counts, sizeof(o.counts));
            for (int len = 1; len <= 16; ++len) { o.first[len] = t.first[len]; o.index[len] = t.index[len]; }
        }
    return FEAR_TRAIN_OK;
}

// The subsequences of a prepared scan, for its index (fear_jpeg_store.h): segment s has ceil(bytes / subsequence_bytes) of them, and
// sub_start holds the prefix sums.  Reads seg_start[0 .. n_seg], writes sub_start[0 .. n_seg] where it is given.
int fear_jpeg_sub_start(const uint32_t* seg_start, uint32_t n_seg, uint32_t n_bytes, int subsequence_bytes, uint32_t* sub_start,
                        size_t sub_cap, uint32_t* n_sub) {
    if (!seg_start || !n_sub) return FEAR_TRAIN_ERR_NULL;
    if (subsequence_bytes < 4 || subsequence_bytes > 1024 || (subsequence_bytes & 3) != 0) return FEAR_TRAIN_ERR_SHAPE;
    if (sub_start && sub_cap < (size_t)n_seg + 1) return FEAR_TRAIN_ERR_WORKSPACE;
    if (n_seg == 0 || seg_start[0] != 0 || seg_start[n_seg] != n_bytes) return FEAR_TRAIN_ERR_SHAPE;   // not this scan's offsets
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        if (seg_start[s + 1] < seg_start[s]) return FEAR_TRAIN_ERR_SHAPE;
        if (sub_start) sub_start[s] = (uint32_t)total;
        total += ((uint64_t)(seg_start[s + 1] - seg_start[s]) + (uint32_t)subsequence_bytes - 1) / (uint32_t)subsequence_bytes;
    }
    if (sub_start) sub_start[n_seg] = (uint32_t)total;                   // at most 2^32 - 1 bytes in all, at least 4 per subsequence
    *n_sub = (uint32_t)total;
    return FEAR_TRAIN_OK;
}

}  // extern "C"

#endif  // FEAR_JPEG_ENTROPY_H
