// fear_jpeg_decode.h — the device half of the JPEG frame decoder (include/fear_train.h): from the packed quantised
// coefficients the host's Huffman stage leaves (fear_jpeg_entropy.h) to uint8 RGB frames, as libjpeg computes them with its defaults
// (islow IDCT, fancy upsampling).  jpeg_frames.jpeg_decode_host restates the contract in numpy and the two agree bit for bit.
//
// The batch is ragged — images of any sizes and sampling modes — and each kernel is one launch for all of it: a workgroup finds its image in
// a prefix table of workgroups per image (device memory, the same address for every lane: scalar loads, at most 16 steps).
//   jpeg_decode_blocks_kernel  32 blocks per workgroup, eight lanes per block as in jpeg_blocks_kernel: the stored values un-zigzagged into
//                              a zeroed block and dequantised, jpeg_idct<true> down the columns, jpeg_idct<false> along the rows, + 128,
//                              clamp, one 8-byte store per block row to the component's padded plane in the workspace
//   jpeg_decode_merge_kernel   one pixel per lane: upsampling by the image's mode at the true edges of the chroma planes, YCbCr -> RGB,
//                              store; pixels past the image's last are not stored
// The device never sees the bitstream: every loop is bounded by a constant, and a block reads at most 64 values whatever its offsets say.
// fear_jpeg_decode_u8_rows_dev runs the same two bodies (jd_blocks<true>, jd_merge<true>: the tests on the band are the only difference)
// for the pixel rows [y0, y1) of each image, read from device memory (jr_band; DESIGN.md section 14, "Rows from the device").
// The pieces every pixel kernel is made of are written once, here, and fear_jpeg_scaled.h uses them too: the block load (jd_load_block),
// the block's home (jd_home), the sample pack (js_sample, jd_pack4), the upsampling filters (jd_taps, jd_h2v1, jd_h2v2), the colour conversion and
// store (jd_store_rgb), the full-size pixel stage of a workgroup that knows its image (jd_merge_image), and on the host the one check of
// records and workspace (jd_check).
// Included by fear_train.hip behind fear_train_jpeg.h, whose transforms and LDS pitch it uses.

namespace {

struct JpegDecodeArgs {
    const uint32_t* table;   // the caller's device table: two prefix tables of n + 1 entries, padding, n FearJpegImage records
    uint8_t* planes;         // the workspace, 16-byte aligned
    int n;
    int m;                   // the side of a block in frame pixels: 8, and 8 / scale = 4, 2 or 1 in fear_jpeg_scaled.h, whose second
                             // prefix table counts scaled pixels; 0 in fear_jpeg_decode_mixed_u8: every record carries its own
};

// The m of a record of fear_jpeg_decode_mixed_u8, from the scale in its reserved[0]: 0 and 1 are full size, and so is, on the device,
// whatever the host's check would have refused (jd_scale_ok) — the side is one of 8, 4, 2, 1 whatever the word holds.
__host__ __device__ __forceinline__ int jd_record_m(int scale) {
    return scale == 2 ? 4 : (scale == 4 ? 2 : (scale == 8 ? 1 : 8));
}

// The image a workgroup belongs to: the i in [0, n) with start[i] <= group < start[i + 1].  n <= 65535: at most 16 halvings.
__device__ __forceinline__ int jd_find_image(const uint32_t* start, int n, uint32_t group) {
    int lo = 0, hi = n;
#pragma unroll 1
    for (int step = 0; step < 16 && hi - lo > 1; ++step) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= group) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ const FearJpegImage* jd_records(const JpegDecodeArgs& a) {
    return reinterpret_cast<const FearJpegImage*>(reinterpret_cast<const char*>(a.table) + FEAR_JPEG_TABLE_RECORDS(a.n));
}

// Block and plane geometry of one image, the same arithmetic on the host and in both kernels.
struct JdGeom {
    int bw0, bwc;            // blocks per row of the luma plane | of a chroma plane
    long n0, nc;             // blocks of the luma plane | of one chroma plane (0 with one component)
};

__host__ __device__ __forceinline__ JdGeom jd_geom(int W, int H, int components, int h, int v) {
    const int mcus_x = (W + 8 * h - 1) / (8 * h), mcus_y = (H + 8 * v - 1) / (8 * v);
    JdGeom g;
    g.bw0 = mcus_x * h;
    g.bwc = mcus_x;
    g.n0 = (long)g.bw0 * (mcus_y * v);
    g.nc = components == 3 ? (long)mcus_x * mcus_y : 0;
    return g;
}

// The band of MCU rows a .. b) that covers the pixel rows [y0, y1) of an image of mcus_y MCU rows of mcu_h pixel rows and `limit` rows in
// all, one MCU row more on each side with `halo`: false, and a = b = 0, for the empty band y0 >= y1 (after the clip to [0, limit]).  The
// one rule of fear_jpeg_huffman_indexed_rows_dev and fear_jpeg_decode_u8_rows_dev; JpegStore.decode_rows states it.
__device__ __forceinline__ bool jr_band(int y0, int y1, int limit, int mcu_h, int mcus_y, bool halo, int* a, int* b) {
    y0 = min(max(y0, 0), limit);
    y1 = min(max(y1, 0), limit);
    *a = *b = 0;
    if (y0 >= y1) return false;
    const int h = halo ? 1 : 0;
    *a = max(y0 / mcu_h - h, 0);
    *b = min((y1 + mcu_h - 1) / mcu_h + h, mcus_y);                      // y1 <= 8192: no overflow
    return *a < *b;
}

// The component of block b of an image (the planes' blocks follow one another: luma, Cb, Cr) and the block's home in its plane.
__device__ __forceinline__ int jd_comp(const JdGeom& g, long b) {
    return b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
}

struct JdHome {
    long rb, by, bx;         // the block within its plane | its row and column of blocks
    int pw;                  // blocks per row of the plane
};

__device__ __forceinline__ JdHome jd_home(const JdGeom& g, int comp, long b) {
    JdHome at;
    at.rb = b - (comp == 0 ? 0 : (comp == 1 ? g.n0 : g.n0 + g.nc));
    at.pw = comp == 0 ? g.bw0 : g.bwc;
    at.by = at.rb / at.pw;
    at.bx = at.rb - at.by * at.pw;
    return at;
}

// Block b of component comp into `base` (the block's 64 ints of LDS; lane k of its eight): zeroed, then — `on` — the stored values from
// zigzag to natural order, times the quantiser.  At most 64 values are read whatever the offsets say.  Two barriers: every lane of the
// workgroup calls it.
__device__ __forceinline__ void jd_load_block(int* base, int k, bool on, const FearJpegImage* im, long b, int comp) {
#pragma unroll
    for (int i = 0; i < 8; ++i) base[k * 8 + i] = 0;
    __syncthreads();
    if (on) {
        const uint32_t s = im->block_start[b], e = im->block_start[b + 1];
        const int cnt = e > s ? (int)min(e - s, 64u) : 0;
        const int16_t* c = im->coef + s;
        const uint16_t* q = im->qt[comp];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = k + 8 * j;
            if (i < cnt) {
                const int nat = fear_jpeg::kZigzagDev.v[i];
                base[nat] = (int)c[i] * (int)q[nat];
            }
        }
    }
    __syncthreads();
}

// Level shift and clamp of one sample | four of them in one word, the first in the low byte.
__device__ __forceinline__ uint32_t js_sample(int x) {
    return (uint32_t)min(max(x + 128, 0), 255);
}

__device__ __forceinline__ uint32_t jd_pack4(const int* d) {
    return js_sample(d[0]) | js_sample(d[1]) << 8 | js_sample(d[2]) << 16 | js_sample(d[3]) << 24;
}

// libjpeg's fancy upsampling.  The chroma columns pixel column x reads on a plane of true width cw: its own and the nearer neighbour's
// (an edge sample is its own neighbour).  h2v1: 3 this + neighbour, in the plane's row that starts at `row`.  h2v2: 3 near + far on
// both axes (the rows that start at `near` and `far`), as jpeg_merge_kernel.
struct JdTaps {
    int cx, nx;
    bool odd;
};

__device__ __forceinline__ JdTaps jd_taps(int x, int cw) {
    const int cx = x >> 1;
    return JdTaps{cx, (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), (x & 1) != 0};
}

__device__ __forceinline__ int jd_h2v1(const uint8_t* plane, long row, const JdTaps& t) {
    return (3 * plane[row + t.cx] + plane[row + t.nx] + (t.odd ? 2 : 1)) >> 2;
}

__device__ __forceinline__ int jd_h2v2(const uint8_t* plane, long near, long far, const JdTaps& t) {
    return (3 * (3 * plane[near + t.cx] + plane[far + t.cx]) + 3 * plane[near + t.nx] + plane[far + t.nx] + (t.odd ? 7 : 8)) >> 4;
}

// jdcolor's YCbCr -> RGB in 16-bit fixed point, clamp, store.  cb = cr = 128 is gray: every product is 0 and the pixel is Y three times.
__device__ __forceinline__ void jd_store_rgb(int Y, int cb, int cr, uint8_t* dst) {
    cb -= 128; cr -= 128;
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int b = Y + ((116130 * cb + 32768) >> 16);
    const int g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    dst[0] = (uint8_t)min(max(r, 0), 255);
    dst[1] = (uint8_t)min(max(g, 0), 255);
    dst[2] = (uint8_t)min(max(b, 0), 255);
}

// The block stage at full size.  ROWS: a block whose MCU row lies outside the band of `rows_dev` (device memory; null otherwise) is
// skipped, and a workgroup all of whose blocks are skipped returns in front of its work.
template <bool ROWS>
__device__ __forceinline__ void jd_blocks(const JpegDecodeArgs& a, const int32_t* rows_dev) {
    __shared__ __attribute__((aligned(16))) int blk[FEAR_JPEG_GROUP_BLOCKS * kJpPitch];
    const int tid = threadIdx.x, lb = tid >> 3, k = tid & 7;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const JdGeom g = jd_geom(im->width, im->height, im->components, im->h, im->v);
    const long b = (long)(blockIdx.x - a.table[img]) * FEAR_JPEG_GROUP_BLOCKS + lb;
    bool on = b < g.n0 + 2 * g.nc;
    const int comp = jd_comp(g, b);
    if (ROWS) {
        const int v = im->v == 2 ? 2 : 1, mcus_y = (im->height + 8 * v - 1) / (8 * v);
        int ba, bb;
        const bool some = jr_band(rows_dev[2 * img], rows_dev[2 * img + 1], im->height, 8 * v, mcus_y, v == 2, &ba, &bb);
        if (on) {
            const long row = jd_home(g, comp, b).by / (comp == 0 ? v : 1);            // the block's MCU row
            on = some && row >= ba && row < bb;
        }
        if (!__syncthreads_or(on)) return;                    // the same for the whole workgroup
    }
    int* base = blk + lb * kJpPitch;
    jd_load_block(base, k, on, im, b, comp);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = base[i * 8 + k];       // columns
    jpeg_idct<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) base[i * 8 + k] = d[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = base[k * 8 + i];       // rows, level shift, clamp, one 8-byte store
    jpeg_idct<false>(d);
    if (on) {
        const JdHome at = jd_home(g, comp, b);
        // plane_offset is a multiple of 16, a plane's size one of 64, a row of blocks' one of 8: every block row is 8-byte aligned
        uint8_t* dst = a.planes + im->plane_offset + (b - at.rb) * 64 + ((at.by * 8 + k) * at.pw + at.bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(jd_pack4(d), jd_pack4(d + 4));
    }
}

__global__ __launch_bounds__(256) void jpeg_decode_blocks_kernel(JpegDecodeArgs a) { jd_blocks<false>(a, nullptr); }

__global__ __launch_bounds__(256) void jpeg_decode_blocks_rows_dev_kernel(JpegDecodeArgs a, const int32_t* rows_dev) {
    jd_blocks<true>(a, rows_dev);
}

// The pixel stage at full size, one pixel per lane.  ROWS: of the rows [y0, y1) of `rows_dev` alone.  Their luma lies in the band's MCU
// rows without the halo and every chroma row they read — one above and below with v == 2 — in the band with it, or the row is clamped at
// a true edge of the image: no plane byte is read that jd_blocks<true> has not written in the same call.
// jd_merge_image is the stage for a workgroup that knows its image (`img`, record `im`, `first` its first workgroup); jd_merge finds it.
template <bool ROWS>
__device__ __forceinline__ void jd_merge_image(const JpegDecodeArgs& a, const int32_t* rows_dev, const FearJpegImage* im, int img,
                                               uint32_t first) {
    const int W = im->width, H = im->height, h = im->h, v = im->v;
    const long px = (long)(blockIdx.x - first) * FEAR_JPEG_GROUP_PIXELS + threadIdx.x;
    if (px >= (long)H * W) return;
    const int y = (int)(px / W), x = (int)(px - (long)y * W);
    if (ROWS && (y < min(max(rows_dev[2 * img], 0), H) || y >= min(max(rows_dev[2 * img + 1], 0), H))) return;   // the clip to [0, H]
    const JdGeom g = jd_geom(W, H, im->components, h, v);
    const uint8_t* planes = a.planes + im->plane_offset;
    const int Y = planes[(long)y * (g.bw0 * 8) + x];
    int cb = 128, cr = 128;
    if (im->components == 3) {
        const uint8_t* pcb = planes + g.n0 * 64;
        const uint8_t* pcr = pcb + g.nc * 64;
        const long pwc = g.bwc * 8;
        const int cw = (W + h - 1) / h, ch = (H + v - 1) / v;  // the true size of a chroma plane
        if (h == 1 || cw <= 2) {                               // no upsampling | replication (libjpeg does not filter a plane this narrow)
            const long at = (long)(y / v) * pwc + x / h;
            cb = pcb[at]; cr = pcr[at];
        } else if (v == 1) {
            const long row = (long)y * pwc;
            const JdTaps t = jd_taps(x, cw);
            cb = jd_h2v1(pcb, row, t); cr = jd_h2v1(pcr, row, t);
        } else {
            const int cy = y >> 1;
            const long near = (long)cy * pwc, far = (long)((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * pwc;
            const JdTaps t = jd_taps(x, cw);
            cb = jd_h2v2(pcb, near, far, t); cr = jd_h2v2(pcr, near, far, t);
        }
    }
    jd_store_rgb(Y, cb, cr, im->out + px * 3);
}

template <bool ROWS>
__device__ __forceinline__ void jd_merge(const JpegDecodeArgs& a, const int32_t* rows_dev) {
    const uint32_t* start = a.table + (a.n + 1);
    const int img = jd_find_image(start, a.n, blockIdx.x);
    jd_merge_image<ROWS>(a, rows_dev, jd_records(a) + img, img, start[img]);
}

__global__ __launch_bounds__(256) void jpeg_decode_merge_kernel(JpegDecodeArgs a) { jd_merge<false>(a, nullptr); }

__global__ __launch_bounds__(256) void jpeg_decode_merge_rows_dev_kernel(JpegDecodeArgs a, const int32_t* rows_dev) {
    jd_merge<true>(a, rows_dev);
}

bool jd_mode_ok(int components, int h, int v) {
    if (components == 1) return h == 1 && v == 1;
    return components == 3 && ((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2));
}

// What the two launches of a pixel stage take: the kernels' argument and the two grids.  block_groups == 0: nothing to launch (n == 0).
struct JdLaunch {
    JpegDecodeArgs a;
    unsigned block_groups, pixel_groups;
};

bool jd_scale_ok(int scale) {
    return scale == 0 || scale == 1 || scale == 2 || scale == 4 || scale == 8;
}

// The one check of the records and the workspace, for frames of m / 8 of the images' sizes (m = 8: full size; m = 0: each record's own,
// jd_record_m of its reserved[0], which is then part of the record's shape), in the order the ABI
// states: n, the null pointers of the call (`missing`: one the entry point has tested itself), each record's, each record's shape, the
// workspace, the grids.  fear_jpeg_decode_workspace_bytes' bound holds at every m: the scaled planes are no larger.
int jd_check(const FearJpegImage* images, int n, const uint32_t* group_start, bool missing, int m, void* workspace, size_t workspace_bytes,
             JdLaunch* out) {
    *out = JdLaunch{};
    if (n < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!images || !group_start || missing) return FEAR_TRAIN_ERR_NULL;
    uint64_t block_groups = 0, pixel_groups = 0;
    for (int i = 0; i < n; ++i) {
        const FearJpegImage& im = images[i];
        if (!im.coef || !im.block_start || !im.out) return FEAR_TRAIN_ERR_NULL;
        if (im.width < 1 || im.width > FEAR_JPEG_MAX_SIDE || im.height < 1 || im.height > FEAR_JPEG_MAX_SIDE ||
            !jd_mode_ok(im.components, im.h, im.v) || (im.plane_offset & 15) != 0 || (m == 0 && !jd_scale_ok(im.reserved[0])))
            return FEAR_TRAIN_ERR_SHAPE;
    }
    if (!workspace) return FEAR_TRAIN_ERR_WORKSPACE;
    for (int i = 0; i < n; ++i) {
        const FearJpegImage& im = images[i];
        const JdGeom g = jd_geom(im.width, im.height, im.components, im.h, im.v);
        const uint64_t blocks = (uint64_t)(g.n0 + 2 * g.nc);
        if (workspace_bytes < 16 || im.plane_offset > workspace_bytes - 16 || blocks * 64 > workspace_bytes - 16 - im.plane_offset)
            return FEAR_TRAIN_ERR_WORKSPACE;
        const uint64_t mi = (uint64_t)(m ? m : jd_record_m(im.reserved[0]));
        const uint64_t sw = ((uint64_t)im.width * mi + 7) / 8, sh = ((uint64_t)im.height * mi + 7) / 8;
        block_groups += (blocks + FEAR_JPEG_GROUP_BLOCKS - 1) / FEAR_JPEG_GROUP_BLOCKS;
        pixel_groups += (sw * sh + FEAR_JPEG_GROUP_PIXELS - 1) / FEAR_JPEG_GROUP_PIXELS;
    }
    if (block_groups > 0x7fffffffu || pixel_groups > 0x7fffffffu) return FEAR_TRAIN_ERR_SHAPE;
    out->a.table = group_start;
    out->a.planes = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    out->a.n = n;
    out->a.m = m;
    out->block_groups = (unsigned)block_groups;
    out->pixel_groups = (unsigned)pixel_groups;
    return FEAR_TRAIN_OK;
}

}  // namespace

extern "C" {

size_t fear_jpeg_decode_workspace_bytes(const FearJpegInfo* infos, int n) {
    if (!infos || n < 0 || n > 65535) return 0;
    size_t sum = 16;                                          // the planes start at the next 16-byte boundary
    for (int i = 0; i < n; ++i) sum += (size_t)infos[i].total_blocks * 64;
    return sum;
}

// The check and the two launches of fear_jpeg_decode_u8 and fear_jpeg_decode_u8_rows_dev (`rows`: the second).
static int jd_decode_u8(const FearJpegImage* images, int n, const uint32_t* group_start, const int32_t* rows_dev, bool rows, void* workspace,
                        size_t workspace_bytes, void* stream) {
    JdLaunch l;
    const int status = jd_check(images, n, group_start, rows && !rows_dev, 8, workspace, workspace_bytes, &l);
    if (status != FEAR_TRAIN_OK || l.block_groups == 0) return status;
    if (rows) {
        hipLaunchKernelGGL(jpeg_decode_blocks_rows_dev_kernel, dim3(l.block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a, rows_dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_decode_merge_rows_dev_kernel, dim3(l.pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a, rows_dev);
        LAUNCH_CHECK();
        return FEAR_TRAIN_OK;
    }
    hipLaunchKernelGGL(jpeg_decode_blocks_kernel, dim3(l.block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_decode_merge_kernel, dim3(l.pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_jpeg_decode_u8(const FearJpegImage* images, int n, const uint32_t* group_start, void* workspace, size_t workspace_bytes,
                        void* stream) {
    return jd_decode_u8(images, n, group_start, nullptr, false, workspace, workspace_bytes, stream);
}

int fear_jpeg_decode_u8_rows_dev(const FearJpegImage* images, int n, const uint32_t* group_start, const int32_t* rows_dev, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return jd_decode_u8(images, n, group_start, rows_dev, true, workspace, workspace_bytes, stream);
}

}  // extern "C"
