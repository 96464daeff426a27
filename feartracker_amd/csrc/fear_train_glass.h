// fear_train_glass.h — the body of fear_glass_u8 (include/fear_train.h): GlassBlur, the fifth member of the blur
// group of the reference's PHOTOMETRIC_AUGMENTATIONS (model_training/dataset/aug.py:8-25), with albumentations' defaults (sigma 0.7,
// max_delta 4, two iterations, mode "fast") on one uint8 HWC crop: cv2's 8-bit Gaussian at 5 x 5, two iterations of pixel swaps, the
// Gaussian again.
//
// One workgroup makes one 32 x 32 tile of the output.  The four stages reach 2 + 4 + 4 + 2 = 12 pixels, so the tile stages its
// neighbourhood of 56 x 56 pixels in LDS, three planes of one byte per pixel, in two buffers the stages alternate between; each stage
// works on the region the stages behind it still need, cut to the crop.  An iteration's scatter is written as a gather: a destination
// looks at the 8 x 8 sources that can reach it, in the order of falling element number n, and takes the first whose offset points at
// it.  The offsets are Philox words, evaluated once per pixel and iteration into a fourth plane.  No atomics, no scratch.
//
// Like fear_train_hls.h the body names no HIP built-in of its own: fear_train_data.h includes it for the device with the defaults
// below; tools/glass_kernel_host.cpp defines the macros for a host build (one thread per lane, a barrier for the sync) that runs under
// the sanitizers.  Integers only.
#ifndef FEAR_GL_DEV
#define FEAR_GL_DEV __device__ __forceinline__
#define FEAR_GL_SYNC() __syncthreads()
#endif

constexpr int kGlassBlur = 5;                               // FEAR_PHOTO_BLUR_GLASS
constexpr int kGlDelta = 4;                                 // max_delta: offsets in [-4, 3]
constexpr int kGlTile = 32, kGlHalo = 12, kGlPitch = kGlTile + 2 * kGlHalo, kGlPlane = kGlPitch * kGlPitch;

struct GlassShared {
    uint8_t a[3 * kGlPlane], b[3 * kGlPlane];               // the crop's three channels around the tile, one byte per pixel
    uint8_t off[kGlPlane];                                  // an iteration's offsets: dy + 4 in bits 0-2, dx + 4 in bits 3-5
};

struct GlassTile {                                          // the tile's origin in the crop, and the crop's sides
    int x0, y0, H, W;
};

struct GlassRegion {                                        // rows [ya, yb), columns [xa, xb) of the crop
    int ya, yb, xa, xb;
};

// The tile grown by `halo` on every side, cut to the crop.
FEAR_GL_DEV GlassRegion gl_region(const GlassTile& t, int halo) {
    GlassRegion r;
    r.ya = t.y0 - halo < 0 ? 0 : t.y0 - halo;
    r.yb = t.y0 + kGlTile + halo > t.H ? t.H : t.y0 + kGlTile + halo;
    r.xa = t.x0 - halo < 0 ? 0 : t.x0 - halo;
    r.xb = t.x0 + kGlTile + halo > t.W ? t.W : t.x0 + kGlTile + halo;
    return r;
}

// Where pixel (y, x) of the crop lies in a plane: every pixel of every region lies within the halo of 12 around the tile.
FEAR_GL_DEV int gl_at(const GlassTile& t, int y, int x) {
    return (y - t.y0 + kGlHalo) * kGlPitch + (x - t.x0 + kGlHalo);
}

FEAR_GL_DEV int gl_reflect(int i, int n) {                 // BORDER_REFLECT_101 at radius 2, n >= 4
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

// The pixels the swaps start from: rows 5 .. H - 4, columns 5 .. W - 4 (none when a side is 8 or less).
FEAR_GL_DEV bool gl_interior(const GlassTile& t, int y, int x) {
    return y > kGlDelta && y <= t.H - kGlDelta && x > kGlDelta && x <= t.W - kGlDelta;
}

// Philox4x32-10 (Salmon et al., Random123) of counter (c0, c1, c2, 0) and key (k0, k1): word 0.
FEAR_GL_DEV uint32_t gl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
    uint32_t c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0; c1 = (uint32_t)p1; c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// cv2.GaussianBlur(ksize (0, 0), sigma 0.7) on 8 bits at pixel (y, x) of one plane: the weights (2, 53, 146, 53, 2) on both axes,
// one rounding.  The taps lie within 2 of the pixel or, reflected, within 2 of the crop's edge behind it: inside the region the
// plane holds.
FEAR_GL_DEV uint8_t gl_gauss(const uint8_t* plane, const GlassTile& t, int y, int x) {
    constexpr int w[5] = {2, 53, 146, 53, 2};
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = gl_reflect(x + j - 2, t.W) - t.x0 + kGlHalo;
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = plane + (gl_reflect(y + i - 2, t.H) - t.y0 + kGlHalo) * kGlPitch;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) s += w[j] * (int)row[xs[j]];
        acc += w[i] * s;
    }
    return (uint8_t)((acc + 32768) >> 16);
}

// One iteration's offsets over the region `r`, for the pixels the swaps start from: 6 bits of word 0 of Philox(counter (x, y, 1 + i, 0)).
FEAR_GL_DEV void gl_offsets(uint8_t* off, const GlassTile& t, const GlassRegion& r, uint32_t iteration, uint32_t k0, uint32_t k1, int tid,
                            int nthr) {
    const int rw = r.xb - r.xa, cnt = rw * (r.yb - r.ya);
    for (int i = tid; i < cnt; i += nthr) {
        const int y = r.ya + i / rw, x = r.xa + i % rw;
        if (gl_interior(t, y, x)) off[gl_at(t, y, x)] = (uint8_t)(gl_philox((uint32_t)x, (uint32_t)y, 1u + iteration, k0, k1) & 63u);
    }
}

// One iteration over the region `r`: `in` holds the image before it (x0) on `r` grown by 4, `off` its offsets there.
//   x[h, w], x[h + dy, w + dx] = x[h + dy, w + dx], x[h, w]      for element n = (H - 4 - h) + (H - 8) (W - 4 - w) of the interior
// A pixel the second assignment reaches takes x0 of the source with the largest n that points at it: the smallest w, then the smallest
// h, of the 8 x 8 sources q - d, d in [-4, 3].  Any other pixel keeps the first assignment's x0[q + d(q)] inside the interior, x0[q]
// outside.
FEAR_GL_DEV void gl_swap(const uint8_t* in, uint8_t* out, const uint8_t* off, const GlassTile& t, const GlassRegion& r, int tid, int nthr) {
    const int rw = r.xb - r.xa, cnt = rw * (r.yb - r.ya);
    for (int i = tid; i < cnt; i += nthr) {
        const int y = r.ya + i / rw, x = r.xa + i % rw;
        int sy = y, sx = x;
        if (gl_interior(t, y, x)) {
            const int o = off[gl_at(t, y, x)];
            sy = y + (o & 7) - kGlDelta; sx = x + ((o >> 3) & 7) - kGlDelta;
        }
        bool found = false;
        for (int ix = 0; ix < 8 && !found; ++ix) {
            const int cx = x - 3 + ix;
            if (cx <= kGlDelta || cx > t.W - kGlDelta) continue;
            for (int iy = 0; iy < 8; ++iy) {
                const int cy = y - 3 + iy;
                if (cy <= kGlDelta || cy > t.H - kGlDelta) continue;
                // the source (cy, cx) reaches (y, x) with dy = 3 - iy and dx = 3 - ix
                if ((int)off[gl_at(t, cy, cx)] == ((7 - iy) | ((7 - ix) << 3))) { sy = cy; sx = cx; found = true; break; }
            }
        }
        const int from = gl_at(t, sy, sx), to = gl_at(t, y, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * kGlPlane + to] = in[c * kGlPlane + from];
    }
}

// One tile of one crop: src, dst (H, W, 3) uint8, distinct; `glass` whether the crop drew the member (a copy otherwise), k0, k1 its
// Philox key; lane `tid` of `nthr`.  Every lane of the workgroup takes the same branches, so every lane meets every barrier or none
// does.
FEAR_GL_DEV void glass_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const GlassTile& t, bool glass, uint32_t k0,
                            uint32_t k1, GlassShared& sh, int tid, int nthr) {
    const GlassRegion tile = gl_region(t, 0);
    const int tw = tile.xb - tile.xa, tcnt = tw * (tile.yb - tile.ya);
    if (!glass) {
        for (int i = tid; i < tcnt * 3; i += nthr) {
            const long at = ((long)(tile.ya + i / (tw * 3)) * t.W + tile.xa) * 3 + i % (tw * 3);
            dst[at] = src[at];
        }
        return;
    }
    {   // the crop around the tile
        const GlassRegion r = gl_region(t, kGlHalo);
        const int rb = (r.xb - r.xa) * 3, cnt = rb * (r.yb - r.ya);
        for (int i = tid; i < cnt; i += nthr) {
            const int y = r.ya + i / rb, j = i % rb, x = r.xa + j / 3;
            sh.a[(j % 3) * kGlPlane + gl_at(t, y, x)] = src[((long)y * t.W + r.xa) * 3 + j];
        }
    }
    FEAR_GL_SYNC();
    {   // the Gaussian, and the first iteration's offsets
        const GlassRegion r = gl_region(t, kGlHalo - 2);
        const int rw = r.xb - r.xa, cnt = rw * (r.yb - r.ya);
        for (int i = tid; i < cnt * 3; i += nthr) {
            const int c = i / cnt, j = i - c * cnt, y = r.ya + j / rw, x = r.xa + j % rw;
            sh.b[c * kGlPlane + gl_at(t, y, x)] = gl_gauss(sh.a + c * kGlPlane, t, y, x);
        }
        gl_offsets(sh.off, t, r, 0u, k0, k1, tid, nthr);
    }
    FEAR_GL_SYNC();
    gl_swap(sh.b, sh.a, sh.off, t, gl_region(t, kGlHalo - 2 - kGlDelta), tid, nthr);
    FEAR_GL_SYNC();
    gl_offsets(sh.off, t, gl_region(t, kGlHalo - 2 - kGlDelta), 1u, k0, k1, tid, nthr);
    FEAR_GL_SYNC();
    gl_swap(sh.a, sh.b, sh.off, t, gl_region(t, 2), tid, nthr);
    FEAR_GL_SYNC();
    for (int i = tid; i < tcnt * 3; i += nthr) {            // the Gaussian again, to the crop's bytes in their order
        const int j = i / 3, c = i - j * 3, y = tile.ya + j / tw, x = tile.xa + j % tw;
        dst[((long)y * t.W + x) * 3 + c] = gl_gauss(sh.b + c * kGlPlane, t, y, x);
    }
}
