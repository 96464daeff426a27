// fear_train_colour.h — the body of fear_colour_u8 (include/fear_train.h): the members of the reference's p = 0.5
// colour OneOf (model_training/dataset/aug.py:35-48) that are no per-value lookup table — Equalize, HueSaturationValue, ColorJitter and
// Emboss — on one uint8 HWC crop.  One workgroup works on one crop, so the member branch is uniform and the per-crop statistics (three
// 256-bin histograms, the sum of the gray plane) stay in LDS: integer sums, exact whatever the order of the additions.
//
// The body names no HIP built-in of its own: a lane knows its index and the workgroup's size, meets the others at FEAR_CL_SYNC() and adds
// to shared memory with FEAR_CL_ATOMIC_ADD().  fear_train_data.h includes it for the device with the defaults below;
// tools/colour_kernel_host.cpp defines the three macros for a host build (one thread per lane, a barrier for the sync) that runs under the
// sanitizers.  Every float product and sum is rounded on its own (`fp contract(off)` in each function that has any: the pragma covers
// the operators written in its block, not those of inlined callees).
#ifndef FEAR_CL_DEV
#define FEAR_CL_DEV __device__ __forceinline__
#define FEAR_CL_SYNC() __syncthreads()
#define FEAR_CL_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#endif

struct ColourOp {            // the layout of FearColourOp (include/fear_train.h)
    int32_t kind;
    uint8_t order[4];
    double contrast;
    float alpha, beta;
    float taps[9];
    int32_t reserved;
};

struct ColourShared {
    unsigned long long gray_sum;     // ColorJitter: the sum of the gray plane in front of the contrast operation
    unsigned int hist[768];          // Equalize: [channel][value]
    int sdiv[256], hdiv[256];        // RGB -> HSV: rint((255 << 12) / i), rint((180 << 12) / (6 i)), entry 0 = 0
    uint8_t lut[768];                // Equalize: the three tables built here.  HueSaturationValue: the host's lh | ls | lv.
                                     // ColorJitter: the host's brightness | lh, then the contrast table built here
};

constexpr int kColourEqualize = 5, kColourHsv = 6, kColourJitter = 7, kColourEmboss = 8;
constexpr int kJitBrightness = 0, kJitContrast = 1, kJitSaturation = 2, kJitHue = 3;

FEAR_CL_DEV int cl_gray(const int* p) {                    // cv2 COLOR_RGB2GRAY on 8u: 14-bit fixed point
    return (4899 * p[0] + 9617 * p[1] + 1868 * p[2] + 8192) >> 14;
}

FEAR_CL_DEV int cl_round_u8(float f) {                     // rint half to even, saturated
    return (int)fminf(fmaxf(rintf(f), 0.f), 255.f);
}

// cv2 COLOR_RGB2HSV on 8u (H in [0, 180)), in place: p = (r, g, b) -> (h, s, v).
FEAR_CL_DEV void cl_rgb_to_hsv(const ColourShared& sh, int* p) {
    const int r = p[0], g = p[1], b = p[2];
    const int v = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int lo = r < g ? (r < b ? r : b) : (g < b ? g : b);
    const int d = v - lo;
    const int s = (d * sh.sdiv[v] + 2048) >> 12;
    const int hp = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
    int h = (hp * sh.hdiv[d] + 2048) >> 12;                // (arithmetic shift of a negative sum)
    h += h < 0 ? 180 : 0;
    p[0] = h; p[1] = s; p[2] = v;
}

// cv2 COLOR_HSV2RGB on 8u, in place: p = (h, s, v) -> (r, g, b), through fp32 as OpenCV's 8u path does.
FEAR_CL_DEV void cl_hsv_to_rgb(int* p) {
#pragma clang fp contract(off)
    const float hf = (float)p[0] * (float)(6.0 / 180.0), sf = (float)p[1] * (float)(1.0 / 255.0), vf = (float)p[2] * (float)(1.0 / 255.0);
    float r = vf, g = vf, b = vf;
    if (p[1] != 0) {
        float sector = floorf(hf), f = hf - sector;
        if (sector < 0.f || sector > 5.f) { sector = 0.f; f = 0.f; }
        const int k = (int)sector;
        const float t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
        // tab = {vf, t1, t2, t3}; (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], two bits per sector
        constexpr unsigned kB = 1u | 1u << 2 | 3u << 4 | 0u << 6 | 0u << 8 | 2u << 10;
        constexpr unsigned kG = 3u | 0u << 2 | 0u << 4 | 2u << 6 | 1u << 8 | 1u << 10;
        constexpr unsigned kR = 0u | 2u << 2 | 1u << 4 | 1u << 6 | 3u << 8 | 0u << 10;
        auto pick = [&](unsigned table) {
            const unsigned i = (table >> (2 * k)) & 3u;
            return i == 0u ? vf : (i == 1u ? t1 : (i == 2u ? t2 : t3));
        };
        b = pick(kB); g = pick(kG); r = pick(kR);
    }
    p[0] = cl_round_u8(r * 255.f); p[1] = cl_round_u8(g * 255.f); p[2] = cl_round_u8(b * 255.f);
}

// ColorJitter's operations o0..o3 on one pixel, each on the previous one's uint8 result.  `stats`: stop in front of the contrast
// operation (whose table needs the mean of exactly this intermediate image).
FEAR_CL_DEV void cl_jitter(const ColourShared& sh, int o0, int o1, int o2, int o3, float alpha, float beta, bool stats, int* p) {
#pragma clang fp contract(off)
    const int order[4] = {o0, o1, o2, o3};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = order[k];                             // uniform over the workgroup
        if (o == kJitBrightness) {
            p[0] = sh.lut[p[0]]; p[1] = sh.lut[p[1]]; p[2] = sh.lut[p[2]];
        } else if (o == kJitContrast) {
            if (stats) return;
            p[0] = sh.lut[512 + p[0]]; p[1] = sh.lut[512 + p[1]]; p[2] = sh.lut[512 + p[2]];
        } else if (o == kJitSaturation) {
            const float g = (float)cl_gray(p) * beta;
            p[0] = cl_round_u8((float)p[0] * alpha + g);
            p[1] = cl_round_u8((float)p[1] * alpha + g);
            p[2] = cl_round_u8((float)p[2] * alpha + g);
        } else {
            cl_rgb_to_hsv(sh, p);
            p[0] = sh.lut[256 + p[0]];
            cl_hsv_to_rgb(p);
        }
    }
}

FEAR_CL_DEV int cl_reflect(int i, int n) {                 // BORDER_REFLECT_101 at radius 1, n >= 2
    return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

// One crop: src, dst (H, W, 3) uint8, distinct; aux (3, 256) the host's tables; lane `tid` of `nthr`.  Every lane of the workgroup takes
// the same branches, so every lane meets every barrier or none does.
FEAR_CL_DEV void colour_crop(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, const ColourOp* __restrict__ opp,
                             const uint8_t* __restrict__ aux, ColourShared& sh, int tid, int nthr) {
#pragma clang fp contract(off)
    const long npx = (long)H * W;
    int kind = opp->kind;
    const int o0 = opp->order[0], o1 = opp->order[1], o2 = opp->order[2], o3 = opp->order[3];
    // a record the host cannot have drawn (an unknown kind, an order that is no permutation of the four operations) copies the crop
    if (kind == kColourJitter && (o0 > 3 || o1 > 3 || o2 > 3 || o3 > 3 || ((1 << o0) | (1 << o1) | (1 << o2) | (1 << o3)) != 15)) kind = 0;
    if (kind < kColourEqualize || kind > kColourEmboss) {
        for (long i = tid; i < npx * 3; i += nthr) dst[i] = src[i];
        return;
    }
    if (kind == kColourEmboss) {
        // cv2.filter2D on uint8 with the record's 3 x 3 taps, as fear_photometric_u8's MotionBlur defines it: correlation, anchor at the
        // centre, BORDER_REFLECT_101, the non-zero taps in row-major order, fp32 accumulation, rint half to even, saturate
        float w[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = opp->taps[t];
        for (long i = tid; i < npx; i += nthr) {
            const int y = (int)(i / W), x = (int)(i - (long)y * W);
            float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (w[t] != 0.f) {
                    const int yy = cl_reflect(y + t / 3 - 1, H), xx = cl_reflect(x + t % 3 - 1, W);
                    const uint8_t* q = src + ((long)yy * W + xx) * 3;
                    acc[0] = acc[0] + w[t] * (float)q[0];
                    acc[1] = acc[1] + w[t] * (float)q[1];
                    acc[2] = acc[2] + w[t] * (float)q[2];
                }
            }
            dst[i * 3] = (uint8_t)cl_round_u8(acc[0]);
            dst[i * 3 + 1] = (uint8_t)cl_round_u8(acc[1]);
            dst[i * 3 + 2] = (uint8_t)cl_round_u8(acc[2]);
        }
        return;
    }
    // ---- set-up: the division tables, the host's tables, the statistics zeroed
    for (int t = tid; t < 768; t += nthr) {
        if (kind == kColourEqualize) sh.hist[t] = 0u;
        else sh.lut[t] = aux[t];
        if (t < 256) {       // no quotient is a tie (1044480 and 122880 are 2^13 times an odd number), so this is rint of the quotient
            sh.sdiv[t] = t == 0 ? 0 : (1044480 + (t >> 1)) / t;
            sh.hdiv[t] = t == 0 ? 0 : (122880 + (t >> 1)) / t;
        }
    }
    if (tid == 0) sh.gray_sum = 0ull;
    FEAR_CL_SYNC();
    if (kind == kColourHsv) {
        for (long i = tid; i < npx; i += nthr) {
            int p[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
            cl_rgb_to_hsv(sh, p);
            p[0] = sh.lut[p[0]]; p[1] = sh.lut[256 + p[1]]; p[2] = sh.lut[512 + p[2]];
            cl_hsv_to_rgb(p);
            dst[i * 3] = (uint8_t)p[0]; dst[i * 3 + 1] = (uint8_t)p[1]; dst[i * 3 + 2] = (uint8_t)p[2];
        }
        return;
    }
    if (kind == kColourEqualize) {
        // cv2.equalizeHist per channel: lut[i] = rint(fp32(sum of hist(i0, i]) * fp32(255) / fp32(total - hist[i0])), i0 the first
        // non-empty bin; a channel with one value keeps it
        for (long i = tid; i < npx; i += nthr) {
            FEAR_CL_ATOMIC_ADD(&sh.hist[src[i * 3]], 1u);
            FEAR_CL_ATOMIC_ADD(&sh.hist[256 + src[i * 3 + 1]], 1u);
            FEAR_CL_ATOMIC_ADD(&sh.hist[512 + src[i * 3 + 2]], 1u);
        }
        FEAR_CL_SYNC();
        const unsigned total = (unsigned)npx;
        for (int t = tid; t < 768; t += nthr) {
            const unsigned* h = sh.hist + (t & ~255);
            const int i = t & 255;
            int i0 = 0;
            while (i0 < 255 && h[i0] == 0u) ++i0;
            const unsigned first = h[i0];
            int out = i;
            if (first != total) {
                unsigned sum = 0u;
                for (int j = i0 + 1; j <= i; ++j) sum += h[j];
                const float scale = 255.f / (float)(total - first);
                out = cl_round_u8((float)sum * scale);
            }
            sh.lut[t] = (uint8_t)out;
        }
        FEAR_CL_SYNC();
        for (long i = tid; i < npx; i += nthr) {
            dst[i * 3] = sh.lut[src[i * 3]];
            dst[i * 3 + 1] = sh.lut[256 + src[i * 3 + 1]];
            dst[i * 3 + 2] = sh.lut[512 + src[i * 3 + 2]];
        }
        return;
    }
    // ---- ColorJitter: the gray sum in front of the contrast operation, its table, then all four operations
    const float alpha = opp->alpha, beta = opp->beta;
    const double contrast = opp->contrast;
    unsigned long long part = 0ull;
    for (long i = tid; i < npx; i += nthr) {
        int p[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
        cl_jitter(sh, o0, o1, o2, o3, alpha, beta, true, p);
        part += (unsigned long long)cl_gray(p);
    }
    FEAR_CL_ATOMIC_ADD(&sh.gray_sum, part);
    FEAR_CL_SYNC();
    {
        const double mean = (double)sh.gray_sum / (double)npx;
        const double offset = mean * (1.0 - contrast);
        for (int i = tid; i < 256; i += nthr) sh.lut[512 + i] = (uint8_t)(int)fmin(fmax((double)i * contrast + offset, 0.0), 255.0);
    }
    FEAR_CL_SYNC();
    for (long i = tid; i < npx; i += nthr) {
        int p[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
        cl_jitter(sh, o0, o1, o2, o3, alpha, beta, false, p);
        dst[i * 3] = (uint8_t)p[0]; dst[i * 3 + 1] = (uint8_t)p[1]; dst[i * 3 + 2] = (uint8_t)p[2];
    }
}
