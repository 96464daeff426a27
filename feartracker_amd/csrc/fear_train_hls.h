// fear_train_hls.h — the body of fear_hls_u8 (include/fear_train.h): the members of the reference's
// PHOTOMETRIC_AUGMENTATIONS (model_training/dataset/aug.py:8-25) that work in HLS — ISONoise of the noise group, RandomRain and
// RandomShadow of the weather group — on one uint8 HWC crop.  One workgroup works on one crop, so the member branch is uniform and what
// a member needs of the whole crop stays in LDS: a one-bit-per-pixel mask (the drops' or the polygons' edges' rasters), two integer sums
// (exact whatever the order of the additions) and ISONoise's Poisson CDF.
//
// Like fear_train_colour.h the body names no HIP built-in of its own: fear_train_data.h includes it for the device with the defaults
// below; tools/hls_kernel_host.cpp defines the macros for a host build (one thread per lane, a barrier for the sync) that runs under
// the sanitizers.  Every float and double product, sum and quotient is rounded on its own (`fp contract(off)` in each function that has
// any); no exponential, logarithm or trigonometric function is evaluated here: ISONoise's come from the caller's tables.
#ifndef FEAR_HL_DEV
#define FEAR_HL_DEV __device__ __forceinline__
#define FEAR_HL_SYNC() __syncthreads()
#define FEAR_HL_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define FEAR_HL_ATOMIC_OR(p, v) atomicOr((p), (v))
#endif

struct HlsOp {               // the layout of FearHlsOp (include/fear_train.h)
    int32_t kind, seg_offset, seg_count;
    float hue_scale;
    double intensity;
    uint32_t key[2];
};

constexpr int kHlsIso = 1, kHlsRain = 2, kHlsShadow = 3;
constexpr int kHlsMaxSide = 256, kHlsMaskWords = kHlsMaxSide * kHlsMaxSide / 32, kHlsCdf = 160, kHlsRainRows = 16;

struct HlsShared {
    unsigned long long s1, s2;           // ISONoise: the sums of (max + min) and of its square over the crop
    double cdf[kHlsCdf];                 // ISONoise: the Poisson CDF, built by lane 0
    unsigned int mask[kHlsMaskWords];    // rain, shadow: bit y W + x
};

FEAR_HL_DEV int hl_round_u8(float f) {                     // rint half to even, saturated
    return (int)fminf(fmaxf(rintf(f), 0.f), 255.f);
}

// cv2 COLOR_RGB2HLS on fp32 in [0, 1]: hls = (h in [0, 360), l, s).
FEAR_HL_DEV void hl_rgb_to_hls(float r, float g, float b, float* hls) {
#pragma clang fp contract(off)
    const float vmax = fmaxf(fmaxf(r, g), b), vmin = fminf(fminf(r, g), b);
    const float d = vmax - vmin, total = vmax + vmin;
    const float l = total * 0.5f;
    float h = 0.f, s = 0.f;
    if (d > 1.1920929e-7f) {                                // FLT_EPSILON
        s = l < 0.5f ? d / total : d / ((2.f - vmax) - vmin);
        const float k = 60.f / d;
        if (vmax == r) h = (g - b) * k;
        else if (vmax == g) h = (b - r) * k + 120.f;
        else h = (r - g) * k + 240.f;
        if (h < 0.f) h = h + 360.f;
    }
    hls[0] = h; hls[1] = l; hls[2] = s;
}

// cv2 COLOR_HLS2RGB on fp32, hscale = 6 / the hue range: rgb in [0, 1].
FEAR_HL_DEV void hl_hls_to_rgb(float h, float l, float s, float hscale, float* rgb) {
#pragma clang fp contract(off)
    float r = l, g = l, b = l;
    if (s != 0.f) {
        const float p2 = l <= 0.5f ? l * (1.f + s) : (l + s) - l * s;
        const float p1 = 2.f * l - p2;
        float hh = h * hscale;
        if (hh < 0.f) hh = hh + 6.f;
        if (hh >= 6.f) hh = hh - 6.f;
        const float sector = floorf(hh), f = hh - sector;
        const int k = (int)fminf(fmaxf(sector, 0.f), 5.f);
        const float span = p2 - p1;
        const float t2 = p1 + span * (1.f - f), t3 = p1 + span * f;
        // tab = {p2, p1, t2, t3}; (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], two bits per sector
        constexpr unsigned kB = 1u | 1u << 2 | 3u << 4 | 0u << 6 | 0u << 8 | 2u << 10;
        constexpr unsigned kG = 3u | 0u << 2 | 0u << 4 | 2u << 6 | 1u << 8 | 1u << 10;
        constexpr unsigned kR = 0u | 2u << 2 | 1u << 4 | 1u << 6 | 3u << 8 | 0u << 10;
        auto pick = [&](unsigned table) {
            const unsigned i = (table >> (2 * k)) & 3u;
            return i == 0u ? p2 : (i == 1u ? p1 : (i == 2u ? t2 : t3));
        };
        b = pick(kB); g = pick(kG); r = pick(kR);
    }
    rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// The 8-bit round trip with the lightness scaled in between, in place: p = (r, g, b).  `shift`: L >> 1 (RandomShadow's L 0.5);
// otherwise trunc(fp32(L) fp32(0.7)) (RandomRain's).
FEAR_HL_DEV void hl_darken_u8(int* p, bool shift) {
#pragma clang fp contract(off)
    const float k = (float)(1.0 / 255.0);
    float hls[3], rgb[3];
    hl_rgb_to_hls((float)p[0] * k, (float)p[1] * k, (float)p[2] * k, hls);
    const int H8 = hl_round_u8(hls[0] * 0.5f), S8 = hl_round_u8(hls[2] * 255.f);
    int L8 = hl_round_u8(hls[1] * 255.f);
    L8 = shift ? L8 >> 1 : (int)((float)L8 * 0.7f);
    hl_hls_to_rgb((float)H8, (float)L8 * k, (float)S8 * k, (float)(6.0 / 180.0), rgb);
    p[0] = hl_round_u8(rgb[0] * 255.f); p[1] = hl_round_u8(rgb[1] * 255.f); p[2] = hl_round_u8(rgb[2] * 255.f);
}

// Philox4x32-10 (Salmon et al., Random123) of counter (c0, c1, 0, 0) and key (k0, k1): words 0 and 1.
FEAR_HL_DEV void hl_philox2(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t* out) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0; c1 = (uint32_t)p1; c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1;
}

FEAR_HL_DEV int hl_reflect(int i, int n) {                 // BORDER_REFLECT_101 at radius <= 3, n >= 4
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

// The raster of the segment s = (x0, y0, x1, y1) into the mask, clipped to the crop: OpenCV's 8-connected line as train_data.line_u8
// states it, left to right, one pixel per step of the longer axis.
FEAR_HL_DEV void hl_raster(HlsShared& sh, int H, int W, const int16_t* s) {
    int x = s[0], y = s[1], dx = (int)s[2] - (int)s[0], dy = (int)s[3] - (int)s[1];
    if (dx < 0) { x = s[2]; y = s[3]; dx = -dx; dy = -dy; }
    const int step_y = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    const bool steep = dy > dx;
    const int major = steep ? dy : dx, minor = steep ? dx : dy;
    int err = major - 2 * minor;
    for (int i = 0; i <= major; ++i) {
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const int bit = y * W + x;                      // < 65536: H, W <= 256
            FEAR_HL_ATOMIC_OR(&sh.mask[bit >> 5], 1u << (bit & 31));
        }
        const bool diag = err < 0;
        err += -2 * minor + (diag ? 2 * major : 0);
        if (steep) { y += step_y; x += diag ? 1 : 0; }
        else { x += 1; y += diag ? step_y : 0; }
    }
}

// A polygon's rows in `seg`: row i holds its edge count (cut to the rows there are), its edges follow.
FEAR_HL_DEV int hl_edge_count(const int16_t* seg, int i, int cnt) {
    const int n = seg[(long)i * 4];
    return n < 0 ? 0 : (n > cnt - i - 1 ? cnt - i - 1 : n);
}

// One crop: src, dst (H, W, 3) uint8, distinct, H, W <= 256; seg the segment table, q the 4096 normal quantiles, exp_table exp(-i / 16)
// for i = 0 .. 1024; lane `tid` of `nthr`.  Every lane of the workgroup takes the same branches, so every lane meets every barrier or
// none does.
FEAR_HL_DEV void hls_crop(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, const HlsOp* __restrict__ opp,
                          const int16_t* __restrict__ seg, const float* __restrict__ q, const double* __restrict__ exp_table,
                          HlsShared& sh, int tid, int nthr) {
#pragma clang fp contract(off)
    const int npx = H * W;
    int kind = opp->kind;
    const int cnt = opp->seg_count;
    // a record the host cannot have drawn (an unknown kind, a negative offset or count) copies the crop
    if ((kind == kHlsRain || kind == kHlsShadow) && (opp->seg_offset < 0 || cnt < 0)) kind = 0;
    if (kind < kHlsIso || kind > kHlsShadow) {
        for (int i = tid; i < npx * 3; i += nthr) dst[i] = src[i];
        return;
    }
    if (kind == kHlsIso) {
        if (tid == 0) { sh.s1 = 0ull; sh.s2 = 0ull; }
        FEAR_HL_SYNC();
        unsigned long long a = 0ull, b = 0ull;
        for (int i = tid; i < npx; i += nthr) {
            const int r = src[i * 3], g = src[i * 3 + 1], bl = src[i * 3 + 2];
            const int hi = r > g ? (r > bl ? r : bl) : (g > bl ? g : bl), lo = r < g ? (r < bl ? r : bl) : (g < bl ? g : bl);
            const unsigned long long t = (unsigned long long)(hi + lo);
            a += t; b += t * t;
        }
        FEAR_HL_ATOMIC_ADD(&sh.s1, a);
        FEAR_HL_ATOMIC_ADD(&sh.s2, b);
        FEAR_HL_SYNC();
        if (tid == 0) {
            // lambda = sigma_L intensity 255 with sigma_L the standard deviation of l = (max + min) / 510, quantised to sixteenths and cut
            // to [0, 64]; then the CDF p_0 = exp(-lambda), p_j = p_{j-1} lambda / j, summed in order
            const double n = (double)npx, mean = (double)sh.s1 / n;
            double var = (double)sh.s2 / n - mean * mean;
            if (!(var > 0.0)) var = 0.0;
            double lam = ((sqrt(var) / 510.0) * opp->intensity) * 255.0;
            lam = rint(lam * 16.0) / 16.0;
            if (!(lam >= 0.0)) lam = 0.0;
            if (lam > 64.0) lam = 64.0;
            double p = exp_table[(int)(lam * 16.0)], acc = p;
            sh.cdf[0] = acc;
            for (int j = 1; j < kHlsCdf; ++j) {
                p = (p * lam) / (double)j;
                acc = acc + p;
                sh.cdf[j] = acc;
            }
        }
        FEAR_HL_SYNC();
        const float k255 = (float)(1.0 / 255.0), hue_scale = opp->hue_scale;
        const uint32_t k0 = opp->key[0], k1 = opp->key[1];
        for (int i = tid; i < npx; i += nthr) {
            const int y = i / W, x = i - y * W;
            uint32_t rnd[2];
            hl_philox2((uint32_t)x, (uint32_t)y, k0, k1, rnd);
            const double u = (double)rnd[0] * (1.0 / 4294967296.0);
            int lo = 0, hi = kHlsCdf;                      // the number of CDF entries <= u
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sh.cdf[mid] <= u) lo = mid + 1; else hi = mid;
            }
            const int k = lo < kHlsCdf - 1 ? lo : kHlsCdf - 1;
            const float noise = q[rnd[1] >> 20] * hue_scale;
            float hls[3], rgb[3];
            hl_rgb_to_hls((float)src[i * 3] * k255, (float)src[i * 3 + 1] * k255, (float)src[i * 3 + 2] * k255, hls);
            float h = hls[0] + noise;
            if (h < 0.f) h = h + 360.f;
            if (h > 360.f) h = h - 360.f;
            const float gain = (float)k * k255;
            const float l = hls[1] + gain * (1.f - hls[1]);
            hl_hls_to_rgb(h, l, hls[2], (float)(6.0 / 360.0), rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (uint8_t)(int)fminf(fmaxf(rgb[c] * 255.f, 0.f), 255.f);
        }
        return;
    }
    // ---- rain, shadow: the mask first
    const int16_t* rows = seg + (long)opp->seg_offset * 4;
    for (int w = tid; w < (npx + 31) / 32; w += nthr) sh.mask[w] = 0u;
    FEAR_HL_SYNC();
    if (kind == kHlsRain) {
        for (int d = tid; d < cnt; d += nthr) hl_raster(sh, H, W, rows + (long)d * 4);
    } else {
        for (int i = 0; i < cnt;) {                         // (uniform: every lane walks the polygons, the edges are dealt out)
            const int n = hl_edge_count(rows, i, cnt);
            for (int e = i + 1 + tid; e <= i + n; e += nthr) hl_raster(sh, H, W, rows + (long)e * 4);
            i += 1 + n;
        }
    }
    FEAR_HL_SYNC();
    if (kind == kHlsRain) {
        // 200 along the drops, cv2.blur at 7 x 7 (BORDER_REFLECT_101, (sum + 24) / 49 in integers), then L 0.7 on every pixel.  A lane
        // walks kHlsRainRows rows of one column with the window's three sums kept: a row of seven enters and one leaves per pixel
        // (integer sums: the same value as the 49 taps added afresh)
        const int chunks = (H + kHlsRainRows - 1) / kHlsRainRows;
        for (int item = tid; item < W * chunks; item += nthr) {
            const int c = item / W, x = item - c * W, y0 = c * kHlsRainRows, y1 = y0 + kHlsRainRows < H ? y0 + kHlsRainRows : H;
            int xs[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) xs[j] = hl_reflect(x + j - 3, W);
            int s[3] = {0, 0, 0};
            auto add_row = [&](int yy, int sign) {
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const int bit = yy * W + xs[j];
                    const bool drop = (sh.mask[bit >> 5] >> (bit & 31)) & 1u;
                    const uint8_t* p = src + (long)bit * 3;
                    s[0] += sign * (drop ? 200 : (int)p[0]); s[1] += sign * (drop ? 200 : (int)p[1]); s[2] += sign * (drop ? 200 : (int)p[2]);
                }
            };
#pragma unroll 1
            for (int dy = -3; dy <= 3; ++dy) add_row(hl_reflect(y0 + dy, H), 1);
#pragma unroll 1
            for (int y = y0; y < y1; ++y) {
                if (y > y0) {
                    add_row(hl_reflect(y + 3, H), 1);
                    add_row(hl_reflect(y - 4, H), -1);
                }
                int v[3] = {(s[0] + 24) / 49, (s[1] + 24) / 49, (s[2] + 24) / 49};
                hl_darken_u8(v, false);
                uint8_t* o = dst + ((long)y * W + x) * 3;
                o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
            }
        }
        return;
    }
    // RandomShadow: inside the raster of an edge, or inside a polygon by the even-odd rule (an edge counts when y0 <= y < y1 and the
    // pixel lies left of it, by integer cross-multiplication): L 0.5
    for (int i = tid; i < npx; i += nthr) {
        const int y = i / W, x = i - y * W;
        bool inside = (sh.mask[i >> 5] >> (i & 31)) & 1u;
        for (int r = 0; r < cnt && !inside;) {
            const int n = hl_edge_count(rows, r, cnt);
            bool odd = false;
            for (int e = r + 1; e <= r + n; ++e) {
                const int16_t* s = rows + (long)e * 4;
                long x0 = s[0], y0 = s[1], x1 = s[2], y1 = s[3];
                if (y0 == y1) continue;
                if (y0 > y1) { const long tx = x0, ty = y0; x0 = x1; y0 = y1; x1 = tx; y1 = ty; }
                if (y >= y0 && y < y1 && (x - x0) * (y1 - y0) < (y - y0) * (x1 - x0)) odd = !odd;
            }
            inside = odd;
            r += 1 + n;
        }
        int v[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
        if (inside) hl_darken_u8(v, true);
        dst[i * 3] = (uint8_t)v[0]; dst[i * 3 + 1] = (uint8_t)v[1]; dst[i * 3 + 2] = (uint8_t)v[2];
    }
}
