// fear_train_jpeg.h — ImageCompression of the reference's PHOTOMETRIC_AUGMENTATIONS (dataset/aug.py:19-22) on gfx950: the lossy part of
// a baseline JPEG round trip as libjpeg computes it (4:2:0, jpeg_set_quality(q, force_baseline), islow DCT both ways, fancy
// upsampling), in integers and without the entropy coding, which is lossless (DESIGN.md section 11 states the contract;
// train_data.jpeg_roundtrip_u8_host restates it in numpy and the two agree bit for bit).  cv2 reads albumentations' RGB crop as BGR, so
// libjpeg's R is channel 2 of the crop and its B is channel 0.
//
// Two launches, because fancy upsampling reads chroma across MCU borders:
//   jpeg_blocks_kernel  colour conversion, h2v2 downsampling, forward DCT, quantiser, dequantiser, inverse DCT; the decoded Y, Cb and Cr
//                       planes go to the workspace.  One workgroup per four MCUs (24 blocks in LDS); eight lanes per block, each one
//                       row or one column; the column lane keeps its column in registers from the second FDCT pass through the
//                       quantiser to the first IDCT pass.
//   jpeg_merge_kernel   h2v2 fancy upsampling, colour conversion back, store.  A crop whose quality is outside 1..100 is copied here.
// Included by fear_train.hip behind fear_train_data.h.

#include "fear_jpeg_tables.h"                                  // the base quantiser tables: fear_jpeg::kBaseQuantDev

namespace {

constexpr int kJpMcus = 4, kJpBlocks = kJpMcus * 6;
// ints per block in LDS: 64 + 8, so that the column reads of four neighbouring blocks (one ds_read_b32 lane group) fall on 32 banks
constexpr int kJpPitch = 72;

// jfdctint / jidctint: FIX(x) = rint(x * 2^13) (CONST_BITS 13, PASS1_BITS 2)
constexpr int kF0_298 = 2446, kF0_390 = 3196, kF0_541 = 4433, kF0_765 = 6270, kF0_899 = 7373, kF1_175 = 9633;
constexpr int kF1_501 = 12299, kF1_847 = 15137, kF1_961 = 16069, kF2_053 = 16819, kF2_562 = 20995, kF3_072 = 25172;

template <int N>
__device__ __forceinline__ int jp_descale(int x) {
    return (x + (1 << (N - 1))) >> N;
}

// One pass of jfdctint over eight values in place.  FIRST: a row (results scaled up by 4), else a column (that factor removed, the
// DCT's 8 kept).  Every intermediate fits 32 bits for 8-bit samples, as libjpeg's own 32-bit builds rely on.
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct(int* d) {
    constexpr int N = FIRST ? 11 : 15;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : jp_descale<2>(t10 + t11);
    d[4] = FIRST ? (t10 - t11) * 4 : jp_descale<2>(t10 - t11);
    int z1 = (t12 + t13) * kF0_541;
    d[2] = jp_descale<N>(z1 + t13 * kF0_765);
    d[6] = jp_descale<N>(z1 - t12 * kF1_847);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * kF1_175;
    t4 *= kF0_298; t5 *= kF2_053; t6 *= kF3_072; t7 *= kF1_501;
    z1 *= -kF0_899; z2 *= -kF2_562;
    z3 = z3 * -kF1_961 + z5;
    z4 = z4 * -kF0_390 + z5;
    d[7] = jp_descale<N>(t4 + z1 + z3);
    d[5] = jp_descale<N>(t5 + z2 + z4);
    d[3] = jp_descale<N>(t6 + z2 + z3);
    d[1] = jp_descale<N>(t7 + z1 + z4);
}

// One pass of jidctint (islow) over eight values in place.  FIRST: a column of dequantised coefficients, else a row, with the final
// descale by CONST_BITS + PASS1_BITS + 3.
template <bool FIRST>
__device__ __forceinline__ void jpeg_idct(int* d) {
    constexpr int N = FIRST ? 11 : 18;
    int z1 = (d[2] + d[6]) * kF0_541;
    int t2 = z1 - d[6] * kF1_847, t3 = z1 + d[2] * kF0_765;
    int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * kF1_175;
    t0 *= kF0_298; t1 *= kF2_053; t2 *= kF3_072; t3 *= kF1_501;
    z1 *= -kF0_899; z2 *= -kF2_562;
    z3 = z3 * -kF1_961 + z5;
    z4 = z4 * -kF0_390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d[0] = jp_descale<N>(t10 + t3); d[7] = jp_descale<N>(t10 - t3);
    d[1] = jp_descale<N>(t11 + t2); d[6] = jp_descale<N>(t11 - t2);
    d[2] = jp_descale<N>(t12 + t1); d[5] = jp_descale<N>(t12 - t1);
    d[3] = jp_descale<N>(t13 + t0); d[4] = jp_descale<N>(t13 - t0);
}

struct JpegArgs {
    const uint8_t* in;       // [n][H][W][3]
    const int32_t* quality;  // [n]
    uint8_t* planes;         // [n] x (Y [H][W] | Cb [H/2][W/2] | Cr [H/2][W/2]), 16-byte aligned
    uint8_t* out;            // [n][H][W][3]
    int H, W;
};

__global__ __launch_bounds__(256) void jpeg_blocks_kernel(JpegArgs a) {
    __shared__ __attribute__((aligned(16))) int blk[kJpBlocks * kJpPitch];
    __shared__ int qt[128];
    const int crop = blockIdx.y, tid = threadIdx.x;
    const int quality = a.quality[crop];
    if (quality < 1 || quality > 100) return;                 // the same for the whole workgroup: jpeg_merge_kernel copies the crop
    const int H = a.H, W = a.W, mw = W >> 4, n_mcu = mw * (H >> 4);
    const long hw = (long)H * W;
    if (tid < 128) {                                          // jpeg_set_quality(quality, force_baseline)
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        qt[tid] = min(max(((int)fear_jpeg::kBaseQuantDev.v[tid] * scale + 50) / 100, 1), 255);
    }
    {
        // one 2 x 2 quad of one MCU per lane: four Y samples and one sample each of Cb and Cr (jccolor, jcsample's h2v2 without smoothing)
        const int g = tid >> 6, qy = (tid >> 3) & 7, qx = tid & 7;
        const int mcu = blockIdx.x * kJpMcus + g;
        int* yb = blk + (g * 6 + (qy >> 2) * 2 + (qx >> 2)) * kJpPitch + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
        int cb = 0, cr = 0;
        if (mcu < n_mcu) {
            const int my = mcu / mw, mx = mcu - my * mw;
            const uint8_t* src = a.in + (crop * hw + (long)(my * 16 + 2 * qy) * W + (mx * 16 + 2 * qx)) * 3;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const uint8_t* p = src + ((long)dy * W + dx) * 3;
                    const int r = p[2], gg = p[1], b = p[0];
                    yb[dy * 8 + dx] = ((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) - 128;
                    cb += (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
                    cr += (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
                }
            const int bias = 1 + (qx & 1);                    // 1, 2, 1, 2 along a row of the downsampled plane
            cb = ((cb + bias) >> 2) - 128;
            cr = ((cr + bias) >> 2) - 128;
        } else {                                              // an MCU past the crop's last: zeros through the transforms, no store
            yb[0] = yb[1] = yb[8] = yb[9] = 0;
        }
        blk[(g * 6 + 4) * kJpPitch + qy * 8 + qx] = cb;
        blk[(g * 6 + 5) * kJpPitch + qy * 8 + qx] = cr;
    }
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
    if (lane_on) {                                            // FDCT columns, quantise, dequantise, IDCT columns
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = col[i * 8];
        jpeg_fdct<false>(d);
        const int* q = qt + ((b % 6) >= 4 ? 64 : 0) + k;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int qq = q[i * 8];
            const unsigned div = (unsigned)qq << 3;
            const int mag = (int)(((unsigned)abs(d[i]) + (div >> 1)) / div);
            d[i] = (d[i] < 0 ? -mag : mag) * qq;
        }
        jpeg_idct<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) col[i * 8] = d[i];
    }
    __syncthreads();
    if (lane_on) {                                            // IDCT rows, level shift, clamp, one 8-byte store
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        jpeg_idct<false>(d);
        const int g = b / 6, comp = b - g * 6;
        const int mcu = blockIdx.x * kJpMcus + g;
        if (mcu < n_mcu) {
            const int my = mcu / mw, mx = mcu - my * mw;
            uint32_t lo = 0u, hi = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo |= (uint32_t)min(max(d[i] + 128, 0), 255) << (8 * i);
                hi |= (uint32_t)min(max(d[i + 4] + 128, 0), 255) << (8 * i);
            }
            uint8_t* planes = a.planes + crop * (hw + hw / 2);
            uint8_t* dst;
            if (comp < 4) dst = planes + (long)(my * 16 + (comp >> 1) * 8 + k) * W + (mx * 16 + (comp & 1) * 8);
            else dst = planes + hw + (comp - 4) * (hw / 4) + (long)(my * 8 + k) * (W >> 1) + mx * 8;
            *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);      // W is a multiple of 16: every block row is 8-byte aligned
        }
    }
}

// One output pixel per lane; H W is a multiple of 256, so the grid covers the crop exactly.
__global__ __launch_bounds__(256) void jpeg_merge_kernel(JpegArgs a) {
    const int crop = blockIdx.y, H = a.H, W = a.W;
    const long hw = (long)H * W, px = (long)blockIdx.x * 256 + threadIdx.x;
    const uint8_t* src = a.in + (crop * hw + px) * 3;
    uint8_t* dst = a.out + (crop * hw + px) * 3;
    const int quality = a.quality[crop];
    if (quality < 1 || quality > 100) {
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        return;
    }
    const int y = (int)(px / W), x = (int)(px - (long)y * W);
    const uint8_t* planes = a.planes + crop * (hw + hw / 2);
    const int cw = W >> 1, ch = H >> 1, cy = y >> 1, cx = x >> 1;
    // h2v2 fancy upsampling: 3 near + far on both axes; an edge sample is its own neighbour
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
    const int round = (x & 1) ? 7 : 8;
    auto up = [&](const uint8_t* c) {
        const int v0 = 3 * c[cy * cw + cx] + c[fy * cw + cx];
        const int v1 = 3 * c[cy * cw + nx] + c[fy * cw + nx];
        return ((3 * v0 + v1 + round) >> 4) - 128;
    };
    const int Y = planes[px], cb = up(planes + hw), cr = up(planes + hw + hw / 4);
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int b = Y + ((116130 * cb + 32768) >> 16);
    const int g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    dst[0] = (uint8_t)min(max(b, 0), 255);
    dst[1] = (uint8_t)min(max(g, 0), 255);
    dst[2] = (uint8_t)min(max(r, 0), 255);
}

bool jpeg_shape_ok(int n, int H, int W) {
    return n >= 0 && n <= 65535 && H >= 16 && W >= 16 && (H & 15) == 0 && (W & 15) == 0 && (long)H * W <= 0x7fffffffL / 3;
}

}  // namespace

extern "C" {

size_t fear_jpeg_workspace_bytes(int n, int H, int W) {
    if (!jpeg_shape_ok(n, H, W)) return 0;
    return (size_t)n * ((size_t)H * W * 3 / 2) + 16;          // + 16: the planes start at the next 16-byte boundary
}

int fear_jpeg_u8(const uint8_t* crops_in, int n, int H, int W, const int32_t* quality, void* workspace, size_t workspace_bytes,
                 uint8_t* crops_out, void* stream) {
    if (!jpeg_shape_ok(n, H, W)) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!crops_in || !quality || !crops_out) return FEAR_TRAIN_ERR_NULL;
    if (crops_in == crops_out) return FEAR_TRAIN_ERR_SHAPE;
    if (!workspace || workspace_bytes < fear_jpeg_workspace_bytes(n, H, W)) return FEAR_TRAIN_ERR_WORKSPACE;
    JpegArgs a{};
    a.in = crops_in;
    a.quality = quality;
    a.planes = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    a.out = crops_out;
    a.H = H; a.W = W;
    const unsigned n_mcu = (unsigned)((H >> 4) * (W >> 4));
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((n_mcu + kJpMcus - 1) / kJpMcus, (unsigned)n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_merge_kernel, dim3((unsigned)((long)H * W / 256), (unsigned)n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
