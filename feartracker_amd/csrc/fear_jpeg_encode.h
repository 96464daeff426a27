// fear_jpeg_encode.h — baseline JPEG files (4:2:0, 4:2:2, 4:4:4 or one gray component) written on gfx950 from uint8 frames: the counterpart of fear_jpeg_decode.h and
// fear_jpeg_huffman.h (include/fear_train.h states the ABI and the passes, DESIGN.md section 14 "Writing JPEG files" the contract;
// jpeg_encode.jpeg_encode_host restates it in numpy and equals Pillow's libjpeg-turbo byte for byte).  The forward transform shares
// jpeg_fdct and the LDS pitch with fear_train_jpeg.h, and reads the zigzag order and the base quantiser from fear_jpeg_tables.h; what is new is frames of any size, the Huffman coder in parallel and
// the byte stream.
//
// Why each launch boundary is there: every one is a dependency across workgroups.
//   transform | sizes      a block's DC difference reads the block before it, which another workgroup may have transformed
//   transform | stats      (calls with an optimised record only) the same; stats | tables: a table is built from the counts of all of
//                          the image's workgroups; tables | sizes: a block's bit count needs the image's own code lengths
//   sizes | segments       a block's bit offset is the sum of all bit counts before it in its restart segment
//   segments | offsets     a segment's byte offset is the sum of all segment lengths before it in its image
//   offsets | write        a block's place in the stream is its segment's offset plus its own
//   write | count          a chunk of the stream is complete when every block that touches it has been written
//   count | lengths        the file's length, and whether it fits, is the sum over all chunks
//   lengths | assemble     a byte's place in the file is the sum over all chunks before its own; nothing is stored before the file is
//                          known to fit
// Included by fear_train.hip behind fear_jpeg_store.h.

#include <algorithm>
#include <initializer_list>

#include "fear_jpeg_huff_build.h"

namespace {

constexpr int kEncMcus = kJpMcus;                              // MCUs per workgroup of the transform: fear_train_jpeg.h's LDS layout
constexpr int kEncGroup = FEAR_JPEG_ENC_GROUP_BLOCKS;          // blocks per workgroup of sizes and write
constexpr int kEncChunk = FEAR_JPEG_ENC_CHUNK_BYTES;           // stream bytes per workgroup of count and assemble
static_assert(kEncGroup == 256 && kEncChunk == 4096, "one lane per block; one lane per 16 bytes of a chunk");
constexpr uint32_t kEncLumaBits = 9 + 11 + 63 * 26, kEncChromaBits = 11 + 11 + 63 * 26;   // the longest block; 4:2:0's MCU: 1244 bytes
constexpr uint32_t kEncOptBits = 16 + 11 + 63 * 26;           // with per-file tables any code may be 16 bits long: 1665 for every block

// An optimised record's scratch.  Its symbol counts stand in FRONT of its stream, so that the call's one memset zeroes them:
// uint32 [4][256] at stream_offset - kEncCountBytes, tables in kEncStd's order.  Behind its plain scratch (EncGeom::bytes): uint32
// codes [4][256] in kEncCodes' form | per table its DHT segment, kEncDhtPitch bytes apart | uint32 dht_bytes [4] (0 for a table the
// layout lacks) | uint32 deep [4] (1: the table's tree is deeper than 32).  The file's header is the record's header with the DHT
// segments put in at enc_dht_at: its length is a device value.
constexpr uint32_t kEncCountBytes = 4 * 256 * 4, kEncDhtPitch = 288, kEncDhtMax = 5 + 16 + 256;
constexpr size_t kEncOptDhtAt = 4 * 256 * 4, kEncOptInfoAt = kEncOptDhtAt + 4 * kEncDhtPitch, kEncOptBytes = kEncOptInfoAt + 32;
static_assert(kEncDhtMax <= kEncDhtPitch && kEncOptBytes % 16 == 0 && kEncCountBytes % 16 == 0, "the scratch keeps 16-byte alignment");
__host__ __device__ inline bool enc_optimized(uint32_t flags) { return (flags & FEAR_JPEG_ENC_OPTIMIZE) != 0; }

// A record's sampling: FEAR_JPEG_ENC_420 .. _GRAY in the low byte.  Per layout the MCU's side shifts, its blocks B, of which the first
// L are luma, and the MCUs per workgroup of the transform: B x MCUS is the 24 blocks of the LDS tile in every layout.
__host__ __device__ inline int enc_mode(uint32_t sampling) { return (int)(sampling & 0xFFu); }
__host__ __device__ inline bool enc_gray_rgb(uint32_t sampling) { return (sampling & FEAR_JPEG_ENC_GRAY_RGB) != 0; }
__host__ __device__ inline int enc_blocks(int mode) { return mode == 0 ? 6 : mode == 1 ? 4 : mode == 2 ? 3 : 1; }
__host__ __device__ inline int enc_luma(int mode) { return mode == 0 ? 4 : mode == 1 ? 2 : 1; }
__host__ __device__ inline int enc_mcus(int mode) { return mode == 0 ? kEncMcus : mode == 1 ? 6 : mode == 2 ? 8 : 24; }
static_assert(kEncMcus * 6 == kJpBlocks && kJpBlocks == 24, "the tile is 24 blocks: 4, 6, 8 or 24 MCUs");
inline bool enc_sampling_ok(uint32_t sampling) {
    return sampling <= FEAR_JPEG_ENC_GRAY || sampling == (FEAR_JPEG_ENC_GRAY | FEAR_JPEG_ENC_GRAY_RGB);
}
// where the DHT segments stand in a header: behind SOI, APP0, the DQT segments and SOF0
__host__ __device__ inline uint32_t enc_dht_at(int mode) { return mode == FEAR_JPEG_ENC_GRAY ? 20 + 69 + 13 : 20 + 2 * 69 + 19; }

// T.81 tables K.3 to K.6 in the order of the file's DHT segments and of the code table below: DC 0, AC 0, DC 1, AC 1
struct EncStdTable {
    uint8_t counts[16];
    int total;
    uint8_t values[162];
};
constexpr EncStdTable kEncStd[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa}},
};

// symbol -> length << 16 | code (T.81 annex C), per table in kEncStd's order; 0 for a symbol the table lacks
struct EncCodes {
    uint32_t v[4 * 256];
};
constexpr EncCodes enc_make_codes() {
    EncCodes c{};
    for (int t = 0; t < 4; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kEncStd[t].counts[len - 1]; ++i, ++k) c.v[t * 256 + kEncStd[t].values[k]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
    }
    return c;
}
__device__ const EncCodes kEncCodes = enc_make_codes();

// One image's geometry and the layout of its scratch behind work_offset: int16 coefficients [n_blocks][64] | uint32 bits [n_blocks] (a
// block's bit count, then its bit offset in its segment) | uint32 seg [n_seg + 1] (a segment's bytes, then its byte offset) | uint32 chunk
// [n_chunks + 1] (a chunk's FF bytes, then the FF bytes before it) | uint32 state [4] (the stream's length, 1 if it exceeds stream_cap)
struct EncGeom {
    int mw, mh, B;
    uint32_t n_mcu, n_blocks, interval, n_seg, n_chunks;
    size_t bits_at, seg_at, chunk_at, state_at, bytes;
};

__host__ __device__ inline EncGeom enc_geom(int W, int H, int restart_interval, uint32_t stream_cap, uint32_t sampling) {
    EncGeom g;
    const int mode = enc_mode(sampling), sx = mode < 2 ? 4 : 3, sy = mode == 0 ? 4 : 3;
    g.mw = (W + (1 << sx) - 1) >> sx;
    g.mh = (H + (1 << sy) - 1) >> sy;
    g.B = enc_blocks(mode);
    g.n_mcu = (uint32_t)g.mw * (uint32_t)g.mh;
    g.n_blocks = g.n_mcu * (uint32_t)g.B;
    g.interval = restart_interval > 0 && (uint32_t)restart_interval < g.n_mcu ? (uint32_t)restart_interval : g.n_mcu;
    g.n_seg = (g.n_mcu + g.interval - 1) / g.interval;
    g.n_chunks = (stream_cap + kEncChunk - 1) / kEncChunk;
    g.bits_at = (size_t)g.n_blocks * 128;
    g.seg_at = g.bits_at + (size_t)g.n_blocks * 4;
    g.chunk_at = g.seg_at + ((size_t)g.n_seg + 1) * 4;
    g.state_at = g.chunk_at + ((size_t)g.n_chunks + 1) * 4;
    g.bytes = (g.state_at + 16 + 15) & ~(size_t)15;
    return g;
}

struct EncArgs {
    const FearJpegEncImage* rec;   // the workspace's first bytes: the caller's device copy of the records
    uint8_t* ws;
    int32_t* length;
    int32_t* status;
    int n;
};

// the image whose workgroups of `pass` include `unit`: the last record whose start[pass] is not above it (every image has workgroups)
__device__ __forceinline__ int enc_find(const FearJpegEncImage* rec, int n, int pass, uint32_t unit) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec[mid].start[pass] <= unit) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Exclusive scan of one value per lane over the 256 lanes of a workgroup; `total` is the sum.  Wave-64 shuffles, then the four waves'
// sums through LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ uint32_t enc_wg_exscan(uint32_t v, uint32_t* lds4, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                          // the previous call's readers are done with lds4
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = lds4[i];
        if (i < wave) base += s;
        sum += s;
    }
    *total = sum;
    return base + inc - v;
}

// The transform's two layout-dependent stages, one body per sampling: enc_fill puts the workgroup's MCUs into the 24-block LDS tile
// (level-shifted samples, blocks in MCU order), enc_store writes the tile's quantised blocks in zigzag order.  A workgroup belongs to
// one image, so the choice between the bodies is uniform.
struct EncTile {
    int W, H, mw, mh, n_mcu, group;
};

__device__ __forceinline__ int enc_y(int r, int g, int b) { return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128; }
__device__ __forceinline__ int enc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int enc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// 4:2:0: four MCUs of 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr
__device__ __forceinline__ void enc_fill_420(int* blk, const uint8_t* __restrict__ src, const EncTile& t, int tid) {
    // one 2 x 2 quad of one MCU per lane.  Luma clamps its coordinates to the frame (replication right and down).  Chroma clamps the
    // full-size column, and the full-size rows of the last downsampled row that exists: rows below it repeat THAT row.
    const int W = t.W, H = t.H;
    const int g = tid >> 6, qy = (tid >> 3) & 7, qx = tid & 7;
    const int mcu = t.group * kEncMcus + g;
    int* yb = blk + (g * 6 + (qy >> 2) * 2 + (qx >> 2)) * kJpPitch + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
    int cb = 0, cr = 0;
    if (mcu < t.n_mcu) {
        const int my = mcu / t.mw, mx = mcu - my * t.mw;
        const int cy = min(my * 8 + qy, ((H + 1) >> 1) - 1);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int yl = min(my * 16 + 2 * qy + dy, H - 1), yc = min(2 * cy + dy, H - 1);
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = min(mx * 16 + 2 * qx + dx, W - 1);
                const uint8_t* p = src + ((size_t)yl * W + x) * 3;
                int rr = p[0], gg = p[1], bb = p[2];
                yb[dy * 8 + dx] = ((19595 * rr + 38470 * gg + 7471 * bb + 32768) >> 16) - 128;
                if (yc != yl) {
                    p = src + ((size_t)yc * W + x) * 3;
                    rr = p[0]; gg = p[1]; bb = p[2];
                }
                cb += (-11059 * rr - 21709 * gg + 32768 * bb + (128 << 16) + 32767) >> 16;
                cr += (32768 * rr - 27439 * gg - 5329 * bb + (128 << 16) + 32767) >> 16;
            }
        }
        const int bias = 1 + (qx & 1);                    // 1, 2, 1, 2 along a row of the downsampled plane
        cb = ((cb + bias) >> 2) - 128;
        cr = ((cr + bias) >> 2) - 128;
    } else {
        yb[0] = yb[1] = yb[8] = yb[9] = 0;
    }
    blk[(g * 6 + 4) * kJpPitch + qy * 8 + qx] = cb;
    blk[(g * 6 + 5) * kJpPitch + qy * 8 + qx] = cr;
}

// 4:2:2 (h2v1): six MCUs of 16 x 8, blocks Y0 Y1 Cb Cr.  One horizontal pair of one MCU per step: 384 pairs.  Every component clamps
// its full-size coordinates to the frame; the bias is 0, 1, 0, 1 along a row of the downsampled plane.
__device__ __forceinline__ void enc_fill_422(int* blk, const uint8_t* __restrict__ src, const EncTile& t, int tid) {
    for (int p = tid; p < 6 * 64; p += 256) {
        const int g = p >> 6, py = (p >> 3) & 7, qx = p & 7;
        const int mcu = t.group * 6 + g;
        int* yb = blk + (g * 4 + (qx >> 2)) * kJpPitch + py * 8 + ((2 * qx) & 7);
        int cb = 0, cr = 0;
        if (mcu < t.n_mcu) {
            const int my = mcu / t.mw, mx = mcu - my * t.mw;
            const uint8_t* row = src + (size_t)min(my * 8 + py, t.H - 1) * t.W * 3;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const uint8_t* q = row + (size_t)min(mx * 16 + 2 * qx + dx, t.W - 1) * 3;
                const int rr = q[0], gg = q[1], bb = q[2];
                yb[dx] = enc_y(rr, gg, bb);
                cb += enc_cb(rr, gg, bb);
                cr += enc_cr(rr, gg, bb);
            }
            cb = ((cb + (qx & 1)) >> 1) - 128;
            cr = ((cr + (qx & 1)) >> 1) - 128;
        } else {
            yb[0] = yb[1] = 0;
        }
        blk[(g * 4 + 2) * kJpPitch + py * 8 + qx] = cb;
        blk[(g * 4 + 3) * kJpPitch + py * 8 + qx] = cr;
    }
}

// 4:4:4: eight MCUs of 8 x 8, blocks Y Cb Cr.  Two pixels of one MCU per lane, replicated right and down.
__device__ __forceinline__ void enc_fill_444(int* blk, const uint8_t* __restrict__ src, const EncTile& t, int tid) {
    const int g = tid >> 5, py = (tid >> 2) & 7, px = (tid & 3) * 2;
    const int mcu = t.group * 8 + g;
    int* yb = blk + (g * 3) * kJpPitch + py * 8 + px;
    if (mcu < t.n_mcu) {
        const int my = mcu / t.mw, mx = mcu - my * t.mw;
        const uint8_t* row = src + (size_t)min(my * 8 + py, t.H - 1) * t.W * 3;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const uint8_t* q = row + (size_t)min(mx * 8 + px + dx, t.W - 1) * 3;
            const int rr = q[0], gg = q[1], bb = q[2];
            yb[dx] = enc_y(rr, gg, bb);
            yb[kJpPitch + dx] = enc_cb(rr, gg, bb) - 128;
            yb[2 * kJpPitch + dx] = enc_cr(rr, gg, bb) - 128;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) yb[c * kJpPitch] = yb[c * kJpPitch + 1] = 0;
    }
}

// gray: 24 MCUs of one block.  The source has one channel, or three of which the luma is taken (RGB true).
template <bool RGB>
__device__ __forceinline__ void enc_fill_gray(int* blk, const uint8_t* __restrict__ src, const EncTile& t, int tid) {
    for (int e = tid; e < kJpBlocks * 64; e += 256) {
        const int g = e >> 6, py = (e >> 3) & 7, px = e & 7;
        const int mcu = t.group * kJpBlocks + g;
        int v = 0;
        if (mcu < t.n_mcu) {
            const int my = mcu / t.mw, mx = mcu - my * t.mw;
            const size_t at = (size_t)min(my * 8 + py, t.H - 1) * t.W + min(mx * 8 + px, t.W - 1);
            if (RGB) v = enc_y(src[at * 3], src[at * 3 + 1], src[at * 3 + 2]);
            else v = (int)src[at] - 128;
        }
        blk[g * kJpPitch + py * 8 + px] = v;
    }
}

// zigzag int16 in MCU order: two coefficients per store, the workgroup's 24 blocks contiguous.  A luma block outside the component
// takes the DC term of the block before it in MCU order and no AC terms: MODE 0 has them right and below, MODE 1 to the right.
template <int MODE>
__device__ __forceinline__ void enc_store(const int* blk, uint32_t* dst, const EncTile& t, int tid) {
    constexpr int B = MODE == 0 ? 6 : MODE == 1 ? 4 : MODE == 2 ? 3 : 1, PER = kJpBlocks / B;
    const int by = (t.H + 7) >> 3, bx = (t.W + 7) >> 3;
    for (int e = tid; e < kJpBlocks * 32; e += 256) {
        const int bl = e >> 5, z = (e & 31) * 2;
        const int g = bl / B, kk = bl - g * B;
        const int mcu = t.group * PER + g;
        if (mcu >= t.n_mcu) continue;
        int from = kk;
        if (MODE == 0) {
            const int my = mcu / t.mw, mx = mcu - my * t.mw;
            const bool R = mx == t.mw - 1 && (bx & 1), D = my == t.mh - 1 && (by & 1);
            const int s1 = R ? 0 : 1, s2 = D ? s1 : 2, s3 = (R || D) ? s2 : 3;
            from = kk == 1 ? s1 : kk == 2 ? s2 : kk == 3 ? s3 : kk;
        } else if (MODE == 1) {
            if (kk == 1 && (bx & 1) && mcu % t.mw == t.mw - 1) from = 0;
        }
        const int* sb = blk + (g * B + from) * kJpPitch;
        int v0, v1;
        if (from != kk) {
            v0 = z == 0 ? sb[0] : 0;
            v1 = 0;
        } else {
            v0 = sb[fear_jpeg::kZigzagDev.v[z]];
            v1 = sb[fear_jpeg::kZigzagDev.v[z + 1]];
        }
        dst[e] = ((uint32_t)v0 & 0xFFFFu) | ((uint32_t)v1 << 16);
    }
}

__global__ __launch_bounds__(256) void jpeg_enc_transform_kernel(EncArgs a) {
    __shared__ __attribute__((aligned(16))) int blk[kJpBlocks * kJpPitch];
    __shared__ int qt[128];
    const int tid = threadIdx.x;
    const int img = enc_find(a.rec, a.n, 0, blockIdx.x);
    const FearJpegEncImage* r = a.rec + img;
    const int quality = r->quality;
    const uint32_t sampling = r->sampling;
    const int mode = enc_mode(sampling);
    const uint8_t* src = r->src;
    EncTile t;
    t.W = r->width;
    t.H = r->height;
    t.mw = (t.W + (mode < 2 ? 15 : 7)) >> (mode < 2 ? 4 : 3);
    t.mh = (t.H + (mode == 0 ? 15 : 7)) >> (mode == 0 ? 4 : 3);
    t.n_mcu = t.mw * t.mh;
    t.group = (int)(blockIdx.x - r->start[0]);
    if (tid < 128) {                                          // jpeg_set_quality(quality, force_baseline)
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        qt[tid] = min(max(((int)fear_jpeg::kBaseQuantDev.v[tid] * scale + 50) / 100, 1), 255);
    }
    if (mode == 0) enc_fill_420(blk, src, t, tid);
    else if (mode == 1) enc_fill_422(blk, src, t, tid);
    else if (mode == 2) enc_fill_444(blk, src, t, tid);
    else if (enc_gray_rgb(sampling)) enc_fill_gray<true>(blk, src, t, tid);
    else enc_fill_gray<false>(blk, src, t, tid);
    __syncthreads();
    const bool lane_on = tid < kJpBlocks * 8;                 // eight lanes per block
    const int b = tid >> 3, k = tid & 7;
    int* row = blk + (lane_on ? b * kJpPitch + k * 8 : 0);
    int* col = blk + (lane_on ? b * kJpPitch + k : 0);
    int d[8];
    if (lane_on) {                                            // FDCT, rows
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jpeg_fdct<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = d[i];
    }
    __syncthreads();
    if (lane_on) {                                            // FDCT columns, quantiser
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = col[i * 8];
        jpeg_fdct<false>(d);
        const bool chroma = mode == 0 ? (b % 6) >= 4 : mode == 1 ? (b & 3) >= 2 : mode == 2 ? (b % 3) != 0 : false;
        const int* q = qt + (chroma ? 64 : 0) + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned div = (unsigned)q[i * 8] << 3;
            const int mag = (int)(((unsigned)abs(d[i]) + (div >> 1)) / div);
            col[i * 8] = d[i] < 0 ? -mag : mag;
        }
    }
    __syncthreads();
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.ws + r->work_offset) + (size_t)t.group * (kJpBlocks * 32);
    if (mode == 0) enc_store<0>(blk, dst, t, tid);
    else if (mode == 1) enc_store<1>(blk, dst, t, tid);
    else if (mode == 2) enc_store<2>(blk, dst, t, tid);
    else enc_store<3>(blk, dst, t, tid);
}

// the block in front of block k of MCU `mcu` in its component, in MCU order; -1 at the start of a restart segment
__device__ __forceinline__ long enc_prev_block(uint32_t mcu, int k, uint32_t interval, int B, int L) {
    if (k >= 1 && k < L) return (long)mcu * B + k - 1;
    if (mcu % interval == 0) return -1;
    return (long)(mcu - 1) * B + (k == 0 ? L - 1 : k);
}

struct EncCount {
    uint32_t bits = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { bits += (uint32_t)len; }
    __device__ __forceinline__ void symbol(const uint32_t* table, int s) { bits += table[s] >> 16; }
};

// stats: a symbol counts in the workgroup's histogram; the extra bits do not matter
struct EncStat {
    __device__ __forceinline__ void put(uint32_t, int) {}
    __device__ __forceinline__ void symbol(uint32_t* table, int s) { atomicAdd(table + s, 1u); }
};

// MSB first into 32-bit words of the little-endian byte stream.  A word this block covers whole is stored; the first word (other blocks'
// bits may lie in front) and the last (others' may follow) are merged with an OR into the zeroed stream.
struct EncWrite {
    uint32_t* words;
    size_t w;
    uint64_t acc = 0;
    int fill;
    bool first = true;
    __device__ __forceinline__ void word(uint32_t v, bool merge) {
        v = __builtin_bswap32(v);
        if (merge) atomicOr(words + w, v);
        else words[w] = v;
        ++w;
    }
    __device__ __forceinline__ void put(uint32_t v, int len) {          // len <= 16, v < 2^len
        acc = acc << len | v;
        fill += len;
        if (fill >= 32) {
            fill -= 32;
            word((uint32_t)(acc >> fill), first);
            first = false;
            acc &= (1ull << fill) - 1;
        }
    }
    __device__ __forceinline__ void symbol(const uint32_t* table, int s) {
        const uint32_t c = table[s];
        put(c & 0xFFFFu, (int)(c >> 16));
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) word((uint32_t)(acc << (32 - fill)), true);
    }
};

// T.81 F.1.2 over one block's 64 zigzag coefficients: `codes` is the code table (kEncCodes' form) in LDS, or for EncStat the
// histogram of the same shape; `t` 0 for luma and 1 for chroma.  The sink takes each Huffman symbol with its table, and the extra bits.
template <class Sink>
__device__ __forceinline__ void enc_block(const uint4* cp, int pred, uint32_t* codes, int t, Sink& sink) {
    uint32_t* dc = codes + t * 512;
    uint32_t* ac = dc + 256;
    int run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint4 q = cp[j];
        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v = (int)(int16_t)(w4[i >> 1] >> (16 * (i & 1)));
            if (j == 0 && i == 0) {
                v -= pred;
                const int s = 32 - __clz(abs(v));
                sink.symbol(dc, s);
                sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
            } else if (v == 0) {
                ++run;
            } else {
                for (; run > 15; run -= 16) sink.symbol(ac, 0xF0);
                const int s = 32 - __clz(abs(v));
                sink.symbol(ac, (run << 4 | s) & 255);
                sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
                run = 0;
            }
        }
    }
    if (run) sink.symbol(ac, 0);
}

// sizes (WRITE false) and write (WRITE true): one lane per block
template <bool WRITE>
__global__ __launch_bounds__(256) void jpeg_enc_code_kernel(EncArgs a) {
    __shared__ uint32_t codes[4 * 256];
    const int tid = threadIdx.x;
    const int img = enc_find(a.rec, a.n, 1, blockIdx.x);
    const FearJpegEncImage* r = a.rec + img;
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    uint8_t* work = a.ws + r->work_offset;
    // the image's own tables if it is optimised, otherwise the standard ones
    const uint32_t* table = enc_optimized(r->flags) ? reinterpret_cast<const uint32_t*>(work + g.bytes) : kEncCodes.v;
#pragma unroll
    for (int i = 0; i < 4; ++i) codes[tid + 256 * i] = table[tid + 256 * i];
    __syncthreads();
    const uint32_t* state = reinterpret_cast<const uint32_t*>(work + g.state_at);
    if (WRITE && state[1]) return;                            // the stream alone exceeds the slot: nothing of this image is written
    const uint32_t b = (blockIdx.x - r->start[1]) * kEncGroup + tid;
    if (b >= g.n_blocks) return;
    const int B = g.B, L = enc_luma(enc_mode(r->sampling));
    const uint32_t mcu = B == 6 ? b / 6 : B == 4 ? b >> 2 : B == 3 ? b / 3 : b;   // (divisions by constants)
    const int k = (int)(b - mcu * (uint32_t)B);
    const int16_t* coef = reinterpret_cast<const int16_t*>(work);
    const long prev = enc_prev_block(mcu, k, g.interval, B, L);
    const int pred = prev < 0 ? 0 : coef[prev * 64];
    const uint4* cp = reinterpret_cast<const uint4*>(coef + (size_t)b * 64);
    uint32_t* bits = reinterpret_cast<uint32_t*>(work + g.bits_at);
    if (!WRITE) {
        EncCount sink;
        enc_block(cp, pred, codes, k >= L, sink);
        bits[b] = sink.bits;
    } else {
        const uint32_t seg = mcu / g.interval;
        const uint32_t* seg_at = reinterpret_cast<const uint32_t*>(work + g.seg_at);
        const uint64_t pos = (uint64_t)seg_at[seg] * 8 + bits[b];
        EncWrite sink;
        sink.words = reinterpret_cast<uint32_t*>(a.ws + r->stream_offset);
        sink.w = (size_t)(pos >> 5);
        sink.fill = (int)(pos & 31);
        enc_block(cp, pred, codes, k >= L, sink);
        const uint32_t seg_last = min((seg + 1) * g.interval, g.n_mcu) * (uint32_t)B - 1;
        if (b == seg_last) {                                  // ones up to the byte
            const int pad = (32 - sink.fill) & 7;
            sink.put((1u << pad) - 1, pad);
        }
        sink.finish();
    }
}

// stats: sizes' grid, one lane per block of an optimised image.  The workgroup's symbols are counted in LDS, and what it saw is added to
// the image's counts: integer sums, the same whatever the order.  A workgroup's blocks belong to one image; a plain image's return.
__global__ __launch_bounds__(256) void jpeg_enc_stats_kernel(EncArgs a) {
    __shared__ uint32_t hist[4 * 256];
    const int tid = threadIdx.x;
    const int img = enc_find(a.rec, a.n, 1, blockIdx.x);
    const FearJpegEncImage* r = a.rec + img;
    if (!enc_optimized(r->flags)) return;                     // the same for the whole workgroup
#pragma unroll
    for (int i = 0; i < 4; ++i) hist[tid + 256 * i] = 0u;
    __syncthreads();
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    const uint8_t* work = a.ws + r->work_offset;
    const uint32_t b = (blockIdx.x - r->start[1]) * kEncGroup + tid;
    if (b < g.n_blocks) {
        const int B = g.B, L = enc_luma(enc_mode(r->sampling));
        const uint32_t mcu = B == 6 ? b / 6 : B == 4 ? b >> 2 : B == 3 ? b / 3 : b;
        const int k = (int)(b - mcu * (uint32_t)B);
        const int16_t* coef = reinterpret_cast<const int16_t*>(work);
        const long prev = enc_prev_block(mcu, k, g.interval, B, L);
        const int pred = prev < 0 ? 0 : coef[prev * 64];
        EncStat sink;
        enc_block(reinterpret_cast<const uint4*>(coef + (size_t)b * 64), pred, hist, k >= L, sink);
    }
    __syncthreads();
    uint32_t* counts = reinterpret_cast<uint32_t*>(a.ws + r->stream_offset - kEncCountBytes);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = hist[tid + 256 * i];
        if (v) atomicAdd(counts + tid + 256 * i, v);
    }
}

// The smallest non-zero frequency other than `skip`'s over the 257 symbols, the larger symbol in a tie: every lane of the wave gets the
// symbol, or -1.  A key is frequency << 9 | (256 - symbol), so that the smallest key is the answer; frequencies stay below 2^41.
__device__ __forceinline__ int enc_huff_smallest(const HuffWork& w, int skip, int lane) {
    uint64_t best = ~0ull;
    for (int i = lane; i < kHuffSymbols; i += 64) {
        const uint64_t f = w.freq[i];
        const uint64_t key = f << 9 | (uint64_t)(kHuffSymbols - 1 - i);
        if (f && i != skip && key < best) best = key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t other = __shfl_xor(best, d, 64);
        best = other < best ? other : best;
    }
    return best == ~0ull ? -1 : kHuffSymbols - 1 - (int)(best & 511u);
}

// One wave builds one table from 256 counts (fear_jpeg_huff_build.h's rule): the frequencies, depths and chains live in LDS, each merge
// takes two wave-wide searches, lane 0 walks the chains and, at the end, limits the lengths, sorts and writes.  Returns on lane 0 whether
// the tree was shallow enough; the other lanes' result is not meaningful.
__device__ __forceinline__ bool enc_huff_table(HuffWork& w, const uint32_t* freq, uint8_t* counts, uint8_t* values, int32_t* n_values,
                                               uint32_t* codes, int32_t* depth) {
    const int lane = threadIdx.x;
    for (int i = lane; i < kHuffSymbols; i += 64) huff_init_one(w, i, i < 256 ? freq[i] : 0u);
    __syncthreads();
    for (int round = 0; round < kHuffSymbols; ++round) {      // at most 256 merges
        const int c1 = enc_huff_smallest(w, -1, lane), c2 = enc_huff_smallest(w, c1, lane);
        if (c2 < 0) break;                                    // the same in every lane
        if (lane == 0) huff_merge(w, c1, c2);
        __syncthreads();
    }
    bool ok = true;
    if (lane == 0) ok = huff_finish(w, counts, values, n_values, codes, depth);
    return ok;
}

// tables: one wave per (image, table) of an optimised image: the code table for sizes and write, and the table's DHT segment
__global__ __launch_bounds__(64) void jpeg_enc_tables_kernel(EncArgs a) {
    __shared__ HuffWork w;
    const int img = blockIdx.x >> 2, t = blockIdx.x & 3;
    const FearJpegEncImage* r = a.rec + img;
    if (!enc_optimized(r->flags)) return;
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    uint8_t* opt = a.ws + r->work_offset + g.bytes;
    uint32_t* info = reinterpret_cast<uint32_t*>(opt + kEncOptInfoAt);
    if (enc_mode(r->sampling) == FEAR_JPEG_ENC_GRAY && t >= 2) {         // gray has table 0 alone: no segment, and no code, so that
        uint32_t* codes = reinterpret_cast<uint32_t*>(opt) + t * 256;     // sizes and write copy zeros and not what the workspace held
        for (int i = threadIdx.x; i < 256; i += 64) codes[i] = 0u;
        if (threadIdx.x == 0) info[t] = info[4 + t] = 0u;
        return;
    }
    const uint32_t* freq = reinterpret_cast<const uint32_t*>(a.ws + r->stream_offset - kEncCountBytes) + t * 256;
    uint8_t* dht = opt + kEncOptDhtAt + (size_t)t * kEncDhtPitch;
    int32_t n_values = 0, depth = 0;
    const bool ok = enc_huff_table(w, freq, dht + 5, dht + 21, &n_values, reinterpret_cast<uint32_t*>(opt) + t * 256, &depth);
    if (threadIdx.x != 0) return;
    dht[0] = 0xFF;
    dht[1] = 0xC4;
    dht[2] = (uint8_t)((19 + n_values) >> 8);
    dht[3] = (uint8_t)((19 + n_values) & 255);
    dht[4] = (uint8_t)((t & 1) << 4 | t >> 1);
    info[t] = ok ? (uint32_t)(21 + n_values) : 0u;
    info[4 + t] = ok ? 0u : 1u;
}

// fear_jpeg_huff_optimal: the same table stage on histograms of the caller's
struct EncHuffArgs {
    const uint32_t* freq;
    uint8_t* counts;
    uint8_t* values;
    int32_t* n_values;
    uint32_t* codes;
    int32_t* status;
};

__global__ __launch_bounds__(64) void jpeg_enc_huff_optimal_kernel(EncHuffArgs a) {
    __shared__ HuffWork w;
    const size_t i = blockIdx.x;
    int32_t n_values = 0, depth = 0;
    const bool ok = enc_huff_table(w, a.freq + i * 256, a.counts + i * 16, a.values + i * 256, &n_values, a.codes + i * 256, &depth);
    if (threadIdx.x != 0) return;
    a.n_values[i] = n_values;
    a.status[i] = ok ? FEAR_TRAIN_OK : FEAR_JPEG_ENC_HUFF_DEPTH;
}

// An optimised image's header: the record's bytes with the tables' DHT segments put in at enc_dht_at.  `deep`: a table was refused.
struct EncHeader {
    const uint8_t* head;
    const uint8_t* dht;                  // null for a plain image
    uint32_t split, dht_bytes[4], bytes;
    bool deep;
};

__device__ __forceinline__ EncHeader enc_header(const FearJpegEncImage* r, const uint8_t* work, const EncGeom& g) {
    EncHeader h;
    h.head = r->header;
    h.dht = nullptr;
    h.split = h.bytes = r->header_bytes;
    h.deep = false;
    if (enc_optimized(r->flags)) {
        const uint32_t* info = reinterpret_cast<const uint32_t*>(work + g.bytes + kEncOptInfoAt);
        h.dht = work + g.bytes + kEncOptDhtAt;
        h.split = enc_dht_at(enc_mode(r->sampling));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            h.dht_bytes[t] = min(info[t], kEncDhtMax);
            h.bytes += h.dht_bytes[t];
            h.deep = h.deep || info[4 + t] != 0;
        }
    }
    return h;
}

// segments: one workgroup per restart segment.  bits[] becomes each block's bit offset in its segment, seg[s] the segment's bytes.
__global__ __launch_bounds__(256) void jpeg_enc_segments_kernel(EncArgs a) {
    __shared__ uint32_t lds4[4];
    const int img = enc_find(a.rec, a.n, 2, blockIdx.x);
    const FearJpegEncImage* r = a.rec + img;
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    uint8_t* work = a.ws + r->work_offset;
    uint32_t* bits = reinterpret_cast<uint32_t*>(work + g.bits_at);
    const uint32_t s = blockIdx.x - r->start[2];
    const uint32_t first = s * g.interval * (uint32_t)g.B, last = min((s + 1) * g.interval, g.n_mcu) * (uint32_t)g.B;
    uint32_t carry = 0;
    for (uint32_t at = first; at < last; at += 256) {
        const uint32_t i = at + threadIdx.x;
        const uint32_t v = i < last ? bits[i] : 0u;
        uint32_t sum;
        const uint32_t ex = enc_wg_exscan(v, lds4, &sum);
        if (i < last) bits[i] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(work + g.seg_at)[s] = (carry + 7) >> 3;
}

// offsets (LENGTHS false): one workgroup per image; seg[] becomes each segment's byte offset in the unstuffed stream, seg[n_seg] and
// state[0] its length, state[1] whether that exceeds the stream's capacity.
// lengths (LENGTHS true): chunk[] becomes the FF bytes in front of each chunk; the file's length and the verdict.
template <bool LENGTHS>
__global__ __launch_bounds__(256) void jpeg_enc_image_scan_kernel(EncArgs a) {
    __shared__ uint32_t lds4[4];
    const int img = blockIdx.x;
    const FearJpegEncImage* r = a.rec + img;
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    uint8_t* work = a.ws + r->work_offset;
    uint32_t* state = reinterpret_cast<uint32_t*>(work + g.state_at);
    uint32_t* v = reinterpret_cast<uint32_t*>(work + (LENGTHS ? g.chunk_at : g.seg_at));
    const bool over = LENGTHS && state[1];
    const uint32_t count = LENGTHS ? (over ? 0u : (state[0] + kEncChunk - 1) / kEncChunk) : g.n_seg;
    uint32_t carry = 0;
    for (uint32_t at = 0; at < count; at += 256) {
        const uint32_t i = at + threadIdx.x;
        const uint32_t x = i < count ? v[i] : 0u;
        uint32_t sum;
        const uint32_t ex = enc_wg_exscan(x, lds4, &sum);
        if (i < count) v[i] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x != 0) return;
    const EncHeader h = enc_header(r, work, g);
    if (!LENGTHS) {
        v[g.n_seg] = carry;
        state[0] = carry;
        state[1] = carry > r->stream_cap || h.deep ? 1u : 0u;   // (a refused table: nothing of the image is written either)
    } else {
        // header, stream, a 00 per FF, two bytes per restart marker, EOI
        const uint64_t total = (uint64_t)h.bytes + state[0] + carry + 2ull * (g.n_seg - 1) + 2;
        const bool fits = !over && total <= r->out_cap;
        a.length[img] = fits ? (int32_t)total : 0;
        a.status[img] = fits ? FEAR_TRAIN_OK : h.deep ? FEAR_JPEG_ENC_HUFF_DEPTH : FEAR_JPEG_ENC_OVERFLOW;
    }
}

__device__ __forceinline__ uint32_t enc_count_ff(uint32_t w) {
    return (uint32_t)((w & 0xFFu) == 0xFFu) + (uint32_t)((w & 0xFF00u) == 0xFF00u) + (uint32_t)((w & 0xFF0000u) == 0xFF0000u) +
           (uint32_t)((w & 0xFF000000u) == 0xFF000000u);
}

// count (STORE false) and assemble (STORE true): one workgroup per chunk of the unstuffed stream, 16 bytes per lane.  The bytes behind
// the stream's end are the memset's zeros: they count as no FF and are not stored.
template <bool STORE>
__global__ __launch_bounds__(256) void jpeg_enc_stuff_kernel(EncArgs a) {
    __shared__ uint32_t lds4[4];
    const int img = enc_find(a.rec, a.n, 3, blockIdx.x);
    const FearJpegEncImage* r = a.rec + img;
    const EncGeom g = enc_geom(r->width, r->height, r->restart_interval, r->stream_cap, r->sampling);
    uint8_t* work = a.ws + r->work_offset;
    const uint32_t* state = reinterpret_cast<const uint32_t*>(work + g.state_at);
    const uint32_t U = state[0], c = blockIdx.x - r->start[3];
    if (state[1] || c * (uint32_t)kEncChunk >= U) return;     // the same for the whole workgroup
    if (STORE && a.status[img] != FEAR_TRAIN_OK) return;
    uint32_t* chunk = reinterpret_cast<uint32_t*>(work + g.chunk_at);
    const uint32_t i0 = c * kEncChunk + threadIdx.x * 16;
    const uint4 q = i0 < U ? reinterpret_cast<const uint4*>(a.ws + r->stream_offset)[i0 >> 4] : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
    uint32_t sum;
    const uint32_t ex = enc_wg_exscan(enc_count_ff(q.x) + enc_count_ff(q.y) + enc_count_ff(q.z) + enc_count_ff(q.w), lds4, &sum);
    if (!STORE) {
        if (threadIdx.x == 0) chunk[c] = sum;
        return;
    }
    uint8_t* out = r->out;
    const EncHeader h = enc_header(r, work, g);
    const uint32_t hb = h.bytes;
    if (c == 0) {
        for (uint32_t i = threadIdx.x; i < h.split; i += 256) out[i] = h.head[i];
        if (h.dht) {                                          // the image's own tables, then the rest of the record's header
            uint32_t at = h.split;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                for (uint32_t i = threadIdx.x; i < h.dht_bytes[t]; i += 256) out[at + i] = h.dht[t * kEncDhtPitch + i];
                at += h.dht_bytes[t];
            }
            for (uint32_t i = h.split + threadIdx.x; i < r->header_bytes; i += 256) out[at + i - h.split] = h.head[i];
        }
    }
    if (i0 >= U) return;
    // the segment of byte i0: the last one whose offset is not above it
    const uint32_t* seg_at = reinterpret_cast<const uint32_t*>(work + g.seg_at);
    uint32_t s = 0;
    if (g.n_seg > 1) {
        uint32_t lo = 0, hi = g.n_seg - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (seg_at[mid] <= i0) lo = mid;
            else hi = mid - 1;
        }
        s = lo;
    }
    uint32_t ff = chunk[c] + ex;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t i = i0 + j;
        if (i >= U) break;
        while (s + 1 < g.n_seg && seg_at[s + 1] <= i) ++s;
        size_t at = (size_t)hb + i + ff + 2 * (size_t)s;
        if (s > 0 && seg_at[s] == i) {                        // the restart marker in front of segment s
            out[at - 2] = 0xFF;
            out[at - 1] = (uint8_t)(0xD0 + ((s - 1) & 7));
        }
        const uint8_t byte = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
        out[at++] = byte;
        if (byte == 0xFF) {
            out[at++] = 0;
            ++ff;
        }
        if (i == U - 1) {
            out[at] = 0xFF;
            out[at + 1] = 0xD9;
        }
    }
}

bool enc_record_ok(const FearJpegEncImage& r) {
    return r.width >= 1 && r.width <= FEAR_JPEG_MAX_SIDE && r.height >= 1 && r.height <= FEAR_JPEG_MAX_SIDE && r.quality >= 1 &&
           r.quality <= 100 && r.restart_interval >= 0 && r.restart_interval <= 65535 && r.header_bytes >= 1 && r.header_bytes <= 4096 &&
           enc_sampling_ok(r.sampling) && (r.flags & ~(uint32_t)FEAR_JPEG_ENC_OPTIMIZE) == 0 &&
           (!enc_optimized(r.flags) || r.header_bytes > enc_dht_at(enc_mode(r.sampling)));
}

// the longest unstuffed stream: every block at its longest, and up to a byte of padding per segment
uint32_t enc_stream_bound(int W, int H, int restart_interval, uint32_t sampling, uint32_t flags = 0) {
    const EncGeom g = enc_geom(W, H, restart_interval, 0, sampling);
    const int L = enc_luma(enc_mode(sampling));
    uint64_t mcu_bits = (uint64_t)L * kEncLumaBits + (uint64_t)(g.B - L) * kEncChromaBits;   // 9952, 6636, 4978, 1658
    if (enc_optimized(flags)) mcu_bits = (uint64_t)g.B * kEncOptBits;  // 9990, 6660, 4995, 1665
    return (uint32_t)((g.n_mcu * mcu_bits + 7) / 8 + g.n_seg);          // 8192 x 8192: 326 MB in 4:2:0, 652 MB in 4:4:4
}

size_t enc_source_bytes(const FearJpegEncImage& r) {
    const bool one = enc_mode(r.sampling) == FEAR_JPEG_ENC_GRAY && !enc_gray_rgb(r.sampling);
    return (size_t)r.width * r.height * (one ? 1 : 3);
}

// The plan of a call: per image what fear_jpeg_encode_plan writes; the workspace's size and the four grids.  False for a call the
// operator refuses by its shape.
struct EncPlan {
    size_t stream_bytes, bytes;
    uint64_t grid[4];
    bool optimized;                      // some record is: the call runs stats and tables
};

bool enc_plan(const FearJpegEncImage* images, int n, FearJpegEncImage* fill, EncPlan* plan) {
    if (n < 0 || n > 65535) return false;
    for (int i = 0; i < n; ++i)
        if (!enc_record_ok(images[i])) return false;
    EncPlan p{};
    for (int i = 0; i < n; ++i) p.optimized = p.optimized || enc_optimized(images[i].flags);
    size_t at = FEAR_JPEG_ENC_TABLE_BYTES(n);
    const size_t stream0 = at;
    for (int pass = 0; pass < 2; ++pass) {                    // all streams first (one memset), then every image's scratch
        for (int i = 0; i < n; ++i) {
            const FearJpegEncImage& r = images[i];
            const uint32_t cap = (std::min(enc_stream_bound(r.width, r.height, r.restart_interval, r.sampling, r.flags), r.out_cap) + 4 + 15) & ~15u;
            const EncGeom g = enc_geom(r.width, r.height, r.restart_interval, cap, r.sampling);
            const bool opt = enc_optimized(r.flags);
            if (pass == 0) {
                if (opt) at += kEncCountBytes;                // the symbol counts, in the memset's reach
                if (fill) {
                    fill[i].stream_offset = at;
                    fill[i].stream_cap = cap;
                }
                at += cap;
            } else {
                if (fill) {
                    fill[i].work_offset = at;
                    fill[i].start[0] = (uint32_t)p.grid[0];
                    fill[i].start[1] = (uint32_t)p.grid[1];
                    fill[i].start[2] = (uint32_t)p.grid[2];
                    fill[i].start[3] = (uint32_t)p.grid[3];
                    fill[i].plan_sampling = r.sampling | r.flags << 16;   // (sampling and flags themselves are the caller's and stay)
                }
                at += g.bytes + (opt ? kEncOptBytes : 0);
                const uint32_t per = (uint32_t)enc_mcus(enc_mode(r.sampling));
                p.grid[0] += (g.n_mcu + per - 1) / per;
                p.grid[1] += (g.n_blocks + kEncGroup - 1) / kEncGroup;
                p.grid[2] += g.n_seg;
                p.grid[3] += g.n_chunks;
            }
        }
        if (pass == 0) p.stream_bytes = at - stream0;
    }
    p.bytes = at;
    for (int k = 0; k < 4; ++k)
        if (p.grid[k] > 0x7fffffffull) return false;
    *plan = p;
    return true;
}

}  // namespace

extern "C" {

int fear_jpeg_encode_header_flags(int width, int height, int quality, int restart_interval, int sampling, uint32_t flags, uint8_t* out,
                                  size_t out_cap, size_t* out_used) {
    if (!out || !out_used) return FEAR_TRAIN_ERR_NULL;
    if ((flags & ~(uint32_t)FEAR_JPEG_ENC_OPTIMIZE) != 0) return FEAR_TRAIN_ERR_SHAPE;
    if (width < 1 || width > FEAR_JPEG_MAX_SIDE || height < 1 || height > FEAR_JPEG_MAX_SIDE || quality < 1 || quality > 100 ||
        restart_interval < 0 || restart_interval > 65535 || sampling < FEAR_JPEG_ENC_420 || sampling > FEAR_JPEG_ENC_GRAY)
        return FEAR_TRAIN_ERR_SHAPE;
    const bool gray = sampling == FEAR_JPEG_ENC_GRAY;
    const int tables = gray ? 1 : 2;
    uint8_t h[FEAR_JPEG_ENC_HEADER_MAX];
    size_t at = 0;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) h[at++] = (uint8_t)b; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < tables; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int z = 0; z < 64; ++z) h[at++] = (uint8_t)std::min(std::max(((int)fear_jpeg::kBaseQuant[t * 64 + fear_jpeg::kZigzag[z]] * scale + 50) / 100, 1), 255);
    }
    if (gray) put({0xFF, 0xC0, 0, 11, 8, height >> 8, height & 255, width >> 8, width & 255, 1, 1, 0x11, 0});
    else
        put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1,
             sampling == FEAR_JPEG_ENC_420 ? 0x22 : sampling == FEAR_JPEG_ENC_422 ? 0x21 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2 * tables && !enc_optimized(flags); ++t) {      // (an optimised file's tables are the device's to put here)
        const int total = kEncStd[t].total;
        put({0xFF, 0xC4, (19 + total) >> 8, (19 + total) & 255, (t & 1) << 4 | t >> 1});
        for (int i = 0; i < 16; ++i) h[at++] = kEncStd[t].counts[i];
        for (int i = 0; i < total; ++i) h[at++] = kEncStd[t].values[i];
    }
    if (restart_interval) put({0xFF, 0xDD, 0, 4, restart_interval >> 8, restart_interval & 255});
    if (gray) put({0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0});
    else put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    if (at > out_cap) return FEAR_TRAIN_ERR_WORKSPACE;
    std::memcpy(out, h, at);
    *out_used = at;
    return FEAR_TRAIN_OK;
}

int fear_jpeg_encode_header_mode(int width, int height, int quality, int restart_interval, int sampling, uint8_t* out, size_t out_cap,
                                 size_t* out_used) {
    return fear_jpeg_encode_header_flags(width, height, quality, restart_interval, sampling, 0, out, out_cap, out_used);
}

int fear_jpeg_encode_header(int width, int height, int quality, int restart_interval, uint8_t* out, size_t out_cap, size_t* out_used) {
    return fear_jpeg_encode_header_mode(width, height, quality, restart_interval, FEAR_JPEG_ENC_420, out, out_cap, out_used);
}

size_t fear_jpeg_encode_bound_flags(int width, int height, int restart_interval, int sampling, uint32_t flags) {
    if (width < 1 || width > FEAR_JPEG_MAX_SIDE || height < 1 || height > FEAR_JPEG_MAX_SIDE || restart_interval < 0 ||
        restart_interval > 65535 || sampling < FEAR_JPEG_ENC_420 || sampling > FEAR_JPEG_ENC_GRAY ||
        (flags & ~(uint32_t)FEAR_JPEG_ENC_OPTIMIZE) != 0)
        return 0;
    const EncGeom g = enc_geom(width, height, restart_interval, 0, (uint32_t)sampling);
    const size_t header = (sampling == FEAR_JPEG_ENC_GRAY ? 328 : 623) + (restart_interval ? 6 : 0);
    // the header with or without DRI; every stream byte stuffed; a marker in front of every segment but the first; EOI
    // (an optimised file's header is never longer: a table lists the symbols its scan has, at most the standard table's 12 or 162)
    return header + 2 * (size_t)enc_stream_bound(width, height, restart_interval, (uint32_t)sampling, flags) + 2 * ((size_t)g.n_seg - 1) + 2;
}

size_t fear_jpeg_encode_bound_mode(int width, int height, int restart_interval, int sampling) {
    return fear_jpeg_encode_bound_flags(width, height, restart_interval, sampling, 0);
}

size_t fear_jpeg_encode_bound(int width, int height, int restart_interval) {
    return fear_jpeg_encode_bound_mode(width, height, restart_interval, FEAR_JPEG_ENC_420);
}

int fear_jpeg_encode_plan(FearJpegEncImage* images, int n) {
    if (n < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!images) return FEAR_TRAIN_ERR_NULL;
    EncPlan plan;
    return enc_plan(images, n, images, &plan) ? FEAR_TRAIN_OK : FEAR_TRAIN_ERR_SHAPE;
}

size_t fear_jpeg_encode_workspace_bytes(const FearJpegEncImage* images, int n) {
    EncPlan plan;
    if (!images || n <= 0 || !enc_plan(images, n, nullptr, &plan)) return 0;
    return plan.bytes;
}

int fear_jpeg_encode_u8(const FearJpegEncImage* images, int n, void* workspace, size_t workspace_bytes, int32_t* length_dev,
                        int32_t* status_dev, void* stream) {
    if (n < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!images || !length_dev || !status_dev) return FEAR_TRAIN_ERR_NULL;
    for (int i = 0; i < n; ++i)
        if (!images[i].src || !images[i].out || !images[i].header) return FEAR_TRAIN_ERR_NULL;
    EncPlan plan;
    std::vector<FearJpegEncImage> want(images, images + n);
    if (!enc_plan(images, n, want.data(), &plan)) return FEAR_TRAIN_ERR_SHAPE;
    if (std::memcmp(want.data(), images, (size_t)n * sizeof(FearJpegEncImage)) != 0) return FEAR_TRAIN_ERR_SHAPE;   // not fear_jpeg_encode_plan's
    for (int i = 0; i < n; ++i) {                             // a source that a slot overlaps (its own or another's)
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(images[i].src), s1 = s0 + enc_source_bytes(images[i]);
        for (int j = 0; j < n; ++j) {
            const uintptr_t o0 = reinterpret_cast<uintptr_t>(images[j].out), o1 = o0 + images[j].out_cap;
            if (s0 < o1 && o0 < s1) return FEAR_TRAIN_ERR_SHAPE;
        }
    }
    if (!workspace || workspace_bytes < plan.bytes) return FEAR_TRAIN_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    EncArgs a{};
    a.rec = static_cast<const FearJpegEncImage*>(workspace);
    a.ws = static_cast<uint8_t*>(workspace);
    a.length = length_dev;
    a.status = status_dev;
    a.n = n;
    if (hipMemsetAsync(a.ws + FEAR_JPEG_ENC_TABLE_BYTES(n), 0, plan.stream_bytes, st) != hipSuccess) return FEAR_TRAIN_ERR_HIP;
    hipLaunchKernelGGL(jpeg_enc_transform_kernel, dim3((unsigned)plan.grid[0]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    if (plan.optimized) {                                     // (the memset above has zeroed the counts)
        hipLaunchKernelGGL(jpeg_enc_stats_kernel, dim3((unsigned)plan.grid[1]), dim3(256), 0, st, a);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_enc_tables_kernel, dim3(4u * (unsigned)n), dim3(64), 0, st, a);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(jpeg_enc_code_kernel<false>, dim3((unsigned)plan.grid[1]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_segments_kernel, dim3((unsigned)plan.grid[2]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_image_scan_kernel<false>, dim3((unsigned)n), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_code_kernel<true>, dim3((unsigned)plan.grid[1]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel<false>, dim3((unsigned)plan.grid[3]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_image_scan_kernel<true>, dim3((unsigned)n), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel<true>, dim3((unsigned)plan.grid[3]), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_jpeg_huff_optimal(const uint32_t* freq_dev, int n, uint8_t* counts_dev, uint8_t* values_dev, int32_t* nvalues_dev,
                           uint32_t* codes_dev, int32_t* status_dev, void* stream) {
    if (n < 0 || n > 65535 * 4) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!freq_dev || !counts_dev || !values_dev || !nvalues_dev || !codes_dev || !status_dev) return FEAR_TRAIN_ERR_NULL;
    const EncHuffArgs a{freq_dev, counts_dev, values_dev, nvalues_dev, codes_dev, status_dev};
    hipLaunchKernelGGL(jpeg_enc_huff_optimal_kernel, dim3((unsigned)n), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
