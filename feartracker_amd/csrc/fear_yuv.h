// 4:2:0 YUV frames (NV12, I420) for the crop path: a full-frame conversion to packed RGB and a multi-format crop kernel that
// reads the Y and chroma planes directly.  Included by fear_engine.hip after fear_kernels.h (linear_tap, the crop's resize).
//
// Colour conversion: OpenCV 4.x's integer BT.601 limited-range form of cvtColor(COLOR_YUV2RGB_NV12 / _I420)
// (color_yuv.simd.hpp), nearest chroma — pixel (x, y) takes chroma sample (x >> 1, y >> 1):
//   uu = U - 128, vv = V - 128, yv = max(0, Y - 16) * 1220542
//   R = sat_u8((yv + (1 << 19) + 1673527 * vv) >> 20)
//   G = sat_u8((yv + (1 << 19) - 852492 * vv - 409993 * uu) >> 20)
//   B = sat_u8((yv + (1 << 19) + 2116026 * uu) >> 20)        (arithmetic shift: floor)
// Every sum stays inside int32: |yv| <= 239 * 1220542, |chroma term| <= 128 * 2116026 + 2^19.
#pragma once

#include <stdint.h>

namespace fear {

struct PlanarFrame {            // the layout of fear_frame_planar (include/fear_hip.h)
    const uint8_t* plane[3];    // RGB: [0] = (H, W, 3) rows; NV12: [0] = Y, [1] = interleaved UV; I420: [0] = Y, [1] = U, [2] = V
    int32_t pitch[3];           // bytes between rows of each plane
    int32_t H, W, format;       // FEAR_FMT_*
};

constexpr int kFmtRGB = 0, kFmtNV12 = 1, kFmtI420 = 2;   // FEAR_FMT_RGB / _NV12 / _I420

// Chroma terms of one (U, V) sample, the rounding half-unit folded in (OpenCV's uvToRGBuv).
struct ChromaTerms {
    int r, g, b;
};

__device__ __forceinline__ ChromaTerms chroma_terms(int u, int v) {
    const int uu = u - 128, vv = v - 128;
    return ChromaTerms{(1 << 19) + 1673527 * vv, (1 << 19) - 852492 * vv - 409993 * uu, (1 << 19) + 2116026 * uu};
}

__device__ __forceinline__ int sat_u8(int v) { return min(max(v, 0), 255); }

// One luma sample with its chroma terms -> R, G, B (OpenCV's yRGBuvToRGBA).
__device__ __forceinline__ void yuv_rgb(int y, const ChromaTerms& t, int& r, int& g, int& b) {
    const int yv = max(0, y - 16) * 1220542;
    r = sat_u8((yv + t.r) >> 20);
    g = sat_u8((yv + t.g) >> 20);
    b = sat_u8((yv + t.b) >> 20);
}

// A table entry the kernels may read: known format, even sizes for the 4:2:0 formats, non-null planes, pitches that hold a row.
// What fear_crop_normalize_planar cannot check on the host (its table lives on the device) is checked here: an entry that fails
// reads no pixel, like an index outside the table.
__device__ __forceinline__ bool planar_frame_ok(const PlanarFrame& f) {
    if (f.H < 1 || f.W < 1 || !f.plane[0]) return false;
    if (f.format == kFmtRGB) return (long)f.pitch[0] >= 3L * f.W;
    if ((f.H | f.W) & 1) return false;
    if (f.format == kFmtNV12) return f.plane[1] && f.pitch[0] >= f.W && f.pitch[1] >= f.W;
    if (f.format == kFmtI420)
        return f.plane[1] && f.plane[2] && f.pitch[0] >= f.W && f.pitch[1] >= f.W / 2 && f.pitch[2] >= f.W / 2;
    return false;
}

// ------------------------------------------------------------------------------------------------
// Full-frame NV12 / I420 -> contiguous (H, W, 3) uint8 RGB.  One thread per 2 x 2 luma block: one chroma fetch serves its four
// pixels.  The host entry (fear_yuv_to_rgb) has validated the frame.
struct YuvToRgbArgs {
    PlanarFrame f;
    uint8_t* rgb;   // [H][W][3]
};

__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(YuvToRgbArgs a) {
    const int cw = a.f.W >> 1, chh = a.f.H >> 1;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long)cw * chh) return;
    const int cy = (int)(p / cw), cx = (int)(p % cw);
    int u, v;
    if (a.f.format == kFmtNV12) {
        const uint8_t* uv = a.f.plane[1] + (long)cy * a.f.pitch[1] + 2 * cx;
        u = uv[0];
        v = uv[1];
    } else {
        u = a.f.plane[1][(long)cy * a.f.pitch[1] + cx];
        v = a.f.plane[2][(long)cy * a.f.pitch[2] + cx];
    }
    const ChromaTerms t = chroma_terms(u, v);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const long row = 2L * cy + dy;
        const uint8_t* ys = a.f.plane[0] + row * a.f.pitch[0] + 2 * cx;
        uint8_t* o = a.rgb + (row * a.f.W + 2 * cx) * 3;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            int r, g, b;
            yuv_rgb(ys[dx], t, r, g, b);
            o[3 * dx] = (uint8_t)r;
            o[3 * dx + 1] = (uint8_t)g;
            o[3 * dx + 2] = (uint8_t)b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// crop_resize_normalize_kernel over a table of frames of any format (RGB with a row pitch, NV12, I420): crop i reads
// frames[frame_idx[i]].  Each tap is resolved to its RGB bytes once, for all three channels (border taps take the pad colour);
// the resize arithmetic after that — identity, exact-half 2 x 2 box, 11-bit bilinear — and the normalisation are the RGB
// kernel's, term for term, so a crop equals crop_resize_normalize_kernel on the converted RGB frame bit for bit.
struct PlanarCropArgs {
    const PlanarFrame* frames;  // [n_frames] device table
    const int* frame_idx;       // [n]; an index outside the table, or an entry planar_frame_ok rejects, reads no pixel
    const int* ctx;             // [n][4] context box x, y, w, h
    const uint8_t* pad;         // [n][3] border colour
    float* out;                 // [n][3][S][S]
    int n_frames, S, n;
    float mean[3], inv_std[3];
};

// The RGB bytes of frame pixel (fx, fy), or the border colour outside the frame.
__device__ __forceinline__ void planar_rgb(const PlanarFrame& f, bool ok, int fx, int fy, const uint8_t* pad, int& r, int& g,
                                           int& b) {
    if (!ok || fx < 0 || fx >= f.W || fy < 0 || fy >= f.H) {
        r = pad[0]; g = pad[1]; b = pad[2];
        return;
    }
    if (f.format == kFmtRGB) {
        const uint8_t* s = f.plane[0] + (long)fy * f.pitch[0] + 3L * fx;
        r = s[0]; g = s[1]; b = s[2];
        return;
    }
    const int y = f.plane[0][(long)fy * f.pitch[0] + fx];
    const long crow = (long)(fy >> 1);
    int u, v;
    if (f.format == kFmtNV12) {
        const uint8_t* uv = f.plane[1] + crow * f.pitch[1] + (fx & ~1);
        u = uv[0];
        v = uv[1];
    } else {
        u = f.plane[1][crow * f.pitch[1] + (fx >> 1)];
        v = f.plane[2][crow * f.pitch[2] + (fx >> 1)];
    }
    yuv_rgb(y, chroma_terms(u, v), r, g, b);
}

__global__ __launch_bounds__(256) void crop_resize_normalize_planar_kernel(PlanarCropArgs a) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int plane = a.S * a.S;
    if (p >= (long)a.n * plane) return;
    const int crop = p / plane, px = p % plane;
    const int dy = px / a.S, dx = px % a.S;
    const int cx = a.ctx[crop * 4], cy = a.ctx[crop * 4 + 1], cw = a.ctx[crop * 4 + 2], ch = a.ctx[crop * 4 + 3];
    const int fi = a.frame_idx[crop];
    PlanarFrame fr{};
    bool ok = false;
    if ((unsigned)fi < (unsigned)a.n_frames) {
        fr = a.frames[fi];
        ok = planar_frame_ok(fr);
    }
    const uint8_t* pad = a.pad + crop * 3;
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    linear_tap<true>(dx, a.S, cw, x0, x1, ax0, ax1);
    linear_tap<false>(dy, a.S, ch, y0, y1, ay0, ay1);
    const bool same = (cw == a.S) && (ch == a.S);           // the reference's resize is the identity then
    const bool half = (cw == 2 * a.S) && (ch == 2 * a.S);   // cv::resize runs an exact 2x2 decimation as the 2x2 box mean
    int v[3];
    if (same) {
        planar_rgb(fr, ok, cx + dx, cy + dy, pad, v[0], v[1], v[2]);
    } else {
        // the four taps: the 2 x 2 box of the decimation, or the bilinear neighbours
        const int xa = half ? 2 * dx : x0, xb = half ? 2 * dx + 1 : x1;
        const int ya = half ? 2 * dy : y0, yb = half ? 2 * dy + 1 : y1;
        int s00[3], s10[3], s01[3], s11[3];
        planar_rgb(fr, ok, cx + xa, cy + ya, pad, s00[0], s00[1], s00[2]);
        planar_rgb(fr, ok, cx + xb, cy + ya, pad, s10[0], s10[1], s10[2]);
        planar_rgb(fr, ok, cx + xa, cy + yb, pad, s01[0], s01[1], s01[2]);
        planar_rgb(fr, ok, cx + xb, cy + yb, pad, s11[0], s11[1], s11[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (half) {
                v[c] = (s00[c] + s10[c] + s01[c] + s11[c] + 2) >> 2;
            } else {
                const int r0 = s00[c] * ax0 + s10[c] * ax1;
                const int r1 = s01[c] * ax0 + s11[c] * ax1;
                int t = (((ay0 * (r0 >> 4)) >> 16) + ((ay1 * (r1 >> 4)) >> 16) + 2) >> 2;
                v[c] = min(max(t, 0), 255);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f = (float)v[c];
        f -= a.mean[c];
        f *= a.inv_std[c];
        a.out[((long)crop * 3 + c) * plane + px] = f;
    }
}

}  // namespace fear
