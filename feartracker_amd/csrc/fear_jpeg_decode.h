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
// fear_jpeg_decode_u8_rows_dev runs the same two kernels for the pixel rows [y0, y1) of each image, read from device memory (jr_band,
// jpeg_decode_blocks_rows_dev_kernel, jpeg_decode_merge_rows_dev_kernel; DESIGN.md section 14, "Rows from the device").
// Included by fear_train.hip behind fear_train_jpeg.h, whose transforms and LDS pitch it uses.

namespace {

__device__ const uint8_t kJdZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegDecodeArgs {
    const uint32_t* table;   // the caller's device table: two prefix tables of n + 1 entries, padding, n FearJpegImage records
    uint8_t* planes;         // the workspace, 16-byte aligned
    int n;
};

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

__global__ __launch_bounds__(256) void jpeg_decode_blocks_kernel(JpegDecodeArgs a) {
    __shared__ __attribute__((aligned(16))) int blk[FEAR_JPEG_GROUP_BLOCKS * kJpPitch];
    const int tid = threadIdx.x, lb = tid >> 3, k = tid & 7;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const JdGeom g = jd_geom(im->width, im->height, im->components, im->h, im->v);
    const long b = (long)(blockIdx.x - a.table[img]) * FEAR_JPEG_GROUP_BLOCKS + lb;
    const bool on = b < g.n0 + 2 * g.nc;
    const int comp = b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
    int* base = blk + lb * kJpPitch;
#pragma unroll
    for (int i = 0; i < 8; ++i) base[k * 8 + i] = 0;
    __syncthreads();
    if (on) {                                                 // the stored values: zigzag -> natural order, times the quantiser
        const uint32_t s = im->block_start[b], e = im->block_start[b + 1];
        const int cnt = e > s ? (int)min(e - s, 64u) : 0;
        const int16_t* c = im->coef + s;
        const uint16_t* q = im->qt[comp];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = k + 8 * j;
            if (i < cnt) {
                const int nat = kJdZigzag[i];
                base[nat] = (int)c[i] * (int)q[nat];
            }
        }
    }
    __syncthreads();
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
        const long rb = b - (comp == 0 ? 0 : (comp == 1 ? g.n0 : g.n0 + g.nc));
        const int pw = comp == 0 ? g.bw0 : g.bwc;
        const long by = rb / pw, bx = rb - by * pw;
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)min(max(d[i] + 128, 0), 255) << (8 * i);
            hi |= (uint32_t)min(max(d[i + 4] + 128, 0), 255) << (8 * i);
        }
        // plane_offset is a multiple of 16, a plane's size one of 64, a row of blocks' one of 8: every block row is 8-byte aligned
        uint8_t* dst = a.planes + im->plane_offset + (b - rb) * 64 + ((by * 8 + k) * pw + bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

__global__ __launch_bounds__(256) void jpeg_decode_merge_kernel(JpegDecodeArgs a) {
    const uint32_t* start = a.table + (a.n + 1);
    const int img = jd_find_image(start, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const int W = im->width, H = im->height, h = im->h, v = im->v;
    const long px = (long)(blockIdx.x - start[img]) * FEAR_JPEG_GROUP_PIXELS + threadIdx.x;
    if (px >= (long)H * W) return;
    const int y = (int)(px / W), x = (int)(px - (long)y * W);
    const JdGeom g = jd_geom(W, H, im->components, h, v);
    const uint8_t* planes = a.planes + im->plane_offset;
    const int Y = planes[(long)y * (g.bw0 * 8) + x];
    int r = Y, gg = Y, b = Y;
    if (im->components == 3) {
        const uint8_t* pcb = planes + g.n0 * 64;
        const uint8_t* pcr = pcb + g.nc * 64;
        const long pwc = g.bwc * 8;
        const int cw = (W + h - 1) / h, ch = (H + v - 1) / v;  // the true size of a chroma plane
        int cb, cr;
        if (h == 1 || cw <= 2) {                               // no upsampling | replication (libjpeg does not filter a plane this narrow)
            const long at = (long)(y / v) * pwc + x / h;
            cb = pcb[at]; cr = pcr[at];
        } else if (v == 1) {                                   // h2v1 fancy: 3 this + neighbour; an edge sample is its own neighbour
            const int cx = x >> 1, nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), round = (x & 1) ? 2 : 1;
            const long row = (long)y * pwc;
            cb = (3 * pcb[row + cx] + pcb[row + nx] + round) >> 2;
            cr = (3 * pcr[row + cx] + pcr[row + nx] + round) >> 2;
        } else {                                               // h2v2 fancy: 3 near + far on both axes, as jpeg_merge_kernel
            const int cy = y >> 1, cx = x >> 1;
            const long near = (long)cy * pwc, far = (long)((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * pwc;
            const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), round = (x & 1) ? 7 : 8;
            cb = (3 * (3 * pcb[near + cx] + pcb[far + cx]) + 3 * pcb[near + nx] + pcb[far + nx] + round) >> 4;
            cr = (3 * (3 * pcr[near + cx] + pcr[far + cx]) + 3 * pcr[near + nx] + pcr[far + nx] + round) >> 4;
        }
        cb -= 128; cr -= 128;
        r = Y + ((91881 * cr + 32768) >> 16);
        b = Y + ((116130 * cb + 32768) >> 16);
        gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    }
    uint8_t* dst = im->out + px * 3;
    dst[0] = (uint8_t)min(max(r, 0), 255);
    dst[1] = (uint8_t)min(max(gg, 0), 255);
    dst[2] = (uint8_t)min(max(b, 0), 255);
}

// The two kernels of fear_jpeg_decode_u8_rows_dev.  They repeat the two above line for line, with the tests on the band added, instead of
// sharing a template with them: the code of the kernels above is pinned (their disassembly is compared with the last release's, DESIGN.md
// section 14, "Rows from the device"), and hipcc orders the operands of the IDCT's additions differently once the body is inlined from a
// template.  A block whose MCU row lies outside the band of `rows_dev` (device memory) is skipped, and a workgroup all of whose blocks are
// skipped returns in front of its work.
__global__ __launch_bounds__(256) void jpeg_decode_blocks_rows_dev_kernel(JpegDecodeArgs a, const int32_t* rows_dev) {
    __shared__ __attribute__((aligned(16))) int blk[FEAR_JPEG_GROUP_BLOCKS * kJpPitch];
    const int tid = threadIdx.x, lb = tid >> 3, k = tid & 7;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const JdGeom g = jd_geom(im->width, im->height, im->components, im->h, im->v);
    const long b = (long)(blockIdx.x - a.table[img]) * FEAR_JPEG_GROUP_BLOCKS + lb;
    bool on = b < g.n0 + 2 * g.nc;
    const int comp = b < g.n0 ? 0 : (b < g.n0 + g.nc ? 1 : 2);
    const int v = im->v == 2 ? 2 : 1, mcus_y = (im->height + 8 * v - 1) / (8 * v);
    int ba, bb;
    const bool some = jr_band(rows_dev[2 * img], rows_dev[2 * img + 1], im->height, 8 * v, mcus_y, v == 2, &ba, &bb);
    if (on) {
        const long rb = b - (comp == 0 ? 0 : (comp == 1 ? g.n0 : g.n0 + g.nc));
        const long row = rb / (comp == 0 ? g.bw0 : g.bwc) / (comp == 0 ? v : 1);      // the block's MCU row
        on = some && row >= ba && row < bb;
    }
    if (!__syncthreads_or(on)) return;                        // the same for the whole workgroup
    int* base = blk + lb * kJpPitch;
#pragma unroll
    for (int i = 0; i < 8; ++i) base[k * 8 + i] = 0;
    __syncthreads();
    if (on) {                                                 // the stored values: zigzag -> natural order, times the quantiser
        const uint32_t s = im->block_start[b], e = im->block_start[b + 1];
        const int cnt = e > s ? (int)min(e - s, 64u) : 0;
        const int16_t* c = im->coef + s;
        const uint16_t* q = im->qt[comp];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = k + 8 * j;
            if (i < cnt) {
                const int nat = kJdZigzag[i];
                base[nat] = (int)c[i] * (int)q[nat];
            }
        }
    }
    __syncthreads();
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
        const long rb = b - (comp == 0 ? 0 : (comp == 1 ? g.n0 : g.n0 + g.nc));
        const int pw = comp == 0 ? g.bw0 : g.bwc;
        const long by = rb / pw, bx = rb - by * pw;
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (uint32_t)min(max(d[i] + 128, 0), 255) << (8 * i);
            hi |= (uint32_t)min(max(d[i + 4] + 128, 0), 255) << (8 * i);
        }
        // plane_offset is a multiple of 16, a plane's size one of 64, a row of blocks' one of 8: every block row is 8-byte aligned
        uint8_t* dst = a.planes + im->plane_offset + (b - rb) * 64 + ((by * 8 + k) * pw + bx) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

// One pixel per lane, of the rows [y0, y1) of `rows_dev` alone.  Their luma lies in the band's MCU rows without the halo and every chroma
// row they read — one above and below with v == 2 — in the band with it, or the row is clamped at a true edge of the image: no plane byte
// is read that jpeg_decode_blocks_rows_dev_kernel has not written in the same call.
__global__ __launch_bounds__(256) void jpeg_decode_merge_rows_dev_kernel(JpegDecodeArgs a, const int32_t* rows_dev) {
    const uint32_t* start = a.table + (a.n + 1);
    const int img = jd_find_image(start, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const int W = im->width, H = im->height, h = im->h, v = im->v;
    const long px = (long)(blockIdx.x - start[img]) * FEAR_JPEG_GROUP_PIXELS + threadIdx.x;
    if (px >= (long)H * W) return;
    const int y = (int)(px / W), x = (int)(px - (long)y * W);
    if (y < min(max(rows_dev[2 * img], 0), H) || y >= min(max(rows_dev[2 * img + 1], 0), H)) return;   // the clip to [0, H]
    const JdGeom g = jd_geom(W, H, im->components, h, v);
    const uint8_t* planes = a.planes + im->plane_offset;
    const int Y = planes[(long)y * (g.bw0 * 8) + x];
    int r = Y, gg = Y, b = Y;
    if (im->components == 3) {
        const uint8_t* pcb = planes + g.n0 * 64;
        const uint8_t* pcr = pcb + g.nc * 64;
        const long pwc = g.bwc * 8;
        const int cw = (W + h - 1) / h, ch = (H + v - 1) / v;  // the true size of a chroma plane
        int cb, cr;
        if (h == 1 || cw <= 2) {                               // no upsampling | replication (libjpeg does not filter a plane this narrow)
            const long at = (long)(y / v) * pwc + x / h;
            cb = pcb[at]; cr = pcr[at];
        } else if (v == 1) {                                   // h2v1 fancy: 3 this + neighbour; an edge sample is its own neighbour
            const int cx = x >> 1, nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), round = (x & 1) ? 2 : 1;
            const long row = (long)y * pwc;
            cb = (3 * pcb[row + cx] + pcb[row + nx] + round) >> 2;
            cr = (3 * pcr[row + cx] + pcr[row + nx] + round) >> 2;
        } else {                                               // h2v2 fancy: 3 near + far on both axes, as jpeg_merge_kernel
            const int cy = y >> 1, cx = x >> 1;
            const long near = (long)cy * pwc, far = (long)((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * pwc;
            const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0), round = (x & 1) ? 7 : 8;
            cb = (3 * (3 * pcb[near + cx] + pcb[far + cx]) + 3 * pcb[near + nx] + pcb[far + nx] + round) >> 4;
            cr = (3 * (3 * pcr[near + cx] + pcr[far + cx]) + 3 * pcr[near + nx] + pcr[far + nx] + round) >> 4;
        }
        cb -= 128; cr -= 128;
        r = Y + ((91881 * cr + 32768) >> 16);
        b = Y + ((116130 * cb + 32768) >> 16);
        gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    }
    uint8_t* dst = im->out + px * 3;
    dst[0] = (uint8_t)min(max(r, 0), 255);
    dst[1] = (uint8_t)min(max(gg, 0), 255);
    dst[2] = (uint8_t)min(max(b, 0), 255);
}

bool jd_mode_ok(int components, int h, int v) {
    if (components == 1) return h == 1 && v == 1;
    return components == 3 && ((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2));
}

}  // namespace

extern "C" {

size_t fear_jpeg_decode_workspace_bytes(const FearJpegInfo* infos, int n) {
    if (!infos || n < 0 || n > 65535) return 0;
    size_t sum = 16;                                          // the planes start at the next 16-byte boundary
    for (int i = 0; i < n; ++i) sum += (size_t)infos[i].total_blocks * 64;
    return sum;
}

// The checks and the two launches of fear_jpeg_decode_u8 and fear_jpeg_decode_u8_rows_dev (`rows_dev` null: the first).
static int jd_decode_u8(const FearJpegImage* images, int n, const uint32_t* group_start, const int32_t* rows_dev, bool rows, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (n < 0 || n > 65535) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!images || !group_start || (rows && !rows_dev)) return FEAR_TRAIN_ERR_NULL;
    uint64_t block_groups = 0, pixel_groups = 0;
    for (int i = 0; i < n; ++i) {
        const FearJpegImage& im = images[i];
        if (!im.coef || !im.block_start || !im.out) return FEAR_TRAIN_ERR_NULL;
        if (im.width < 1 || im.width > FEAR_JPEG_MAX_SIDE || im.height < 1 || im.height > FEAR_JPEG_MAX_SIDE ||
            !jd_mode_ok(im.components, im.h, im.v) || (im.plane_offset & 15) != 0)
            return FEAR_TRAIN_ERR_SHAPE;
    }
    if (!workspace) return FEAR_TRAIN_ERR_WORKSPACE;
    for (int i = 0; i < n; ++i) {
        const FearJpegImage& im = images[i];
        const JdGeom g = jd_geom(im.width, im.height, im.components, im.h, im.v);
        const uint64_t blocks = (uint64_t)(g.n0 + 2 * g.nc);
        if (workspace_bytes < 16 || im.plane_offset > workspace_bytes - 16 || blocks * 64 > workspace_bytes - 16 - im.plane_offset)
            return FEAR_TRAIN_ERR_WORKSPACE;
        block_groups += (blocks + FEAR_JPEG_GROUP_BLOCKS - 1) / FEAR_JPEG_GROUP_BLOCKS;
        pixel_groups += ((uint64_t)im.width * im.height + FEAR_JPEG_GROUP_PIXELS - 1) / FEAR_JPEG_GROUP_PIXELS;
    }
    if (block_groups > 0x7fffffffu || pixel_groups > 0x7fffffffu) return FEAR_TRAIN_ERR_SHAPE;
    JpegDecodeArgs a{};
    a.table = group_start;
    a.planes = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    a.n = n;
    if (rows) {
        hipLaunchKernelGGL(jpeg_decode_blocks_rows_dev_kernel, dim3((unsigned)block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                           rows_dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_decode_merge_rows_dev_kernel, dim3((unsigned)pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                           rows_dev);
        LAUNCH_CHECK();
        return FEAR_TRAIN_OK;
    }
    hipLaunchKernelGGL(jpeg_decode_blocks_kernel, dim3((unsigned)block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_decode_merge_kernel, dim3((unsigned)pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), a);
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
