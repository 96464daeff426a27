// fear_jpeg_scaled.h — the JPEG frame decoder at 1/2, 1/4 and 1/8 size (include/fear_train.h: fear_jpeg_decode_scaled_u8; DESIGN.md
// section 14, "Reduced-size decoding"): libjpeg's scale_denom decode (jdmaster.c, jidctred.c), what Pillow's Image.draft runs, from the
// same packed coefficients and the same 448-byte records as fear_jpeg_decode_u8.  jpeg_frames.jpeg_decode_host(scale=) restates it in
// numpy and the two agree bit for bit.  With m = 8 / scale the frame is ceil(H m / 8) x ceil(W m / 8) and a component runs an ss x ss
// inverse transform in place of the 8 x 8 one: ss = m, doubled while the component's plane stays within the frame (js_transform), so
// that the chroma of 4:2:0 takes the 2 m transform and is not upsampled at all, and the chroma of 4:2:2 keeps m and is upsampled
// horizontally.
//   jpeg_scaled_blocks_kernel  32 blocks per workgroup and eight lanes per block, as jpeg_decode_blocks_kernel (the first prefix table is
//                              therefore fear_jpeg_decode_u8's): the stored values un-zigzagged into a zeroed block and dequantised, the
//                              block's transform down the columns (lane k: column k) and along the rows (lane k < ss: row k), + 128,
//                              clamp, one store of ss bytes per row to the component's plane of ss ss bytes per block — the planes of
//                              an image follow one another, so they take at most the 64 bytes per block that
//                              fear_jpeg_decode_workspace_bytes counts: that bound stays valid at every scale
//   jpeg_scaled_merge_kernel   one SCALED pixel per lane (the second prefix table counts scaled pixels): h2v1 upsampling of 4:2:2 at the
//                              true edge of the scaled chroma plane — fancy when m > 1 and that plane is wider than 2, replication
//                              otherwise: libjpeg turns fancy upsampling off at 1/8 — YCbCr -> RGB, store
//   jpeg_mixed_blocks_kernel, jpeg_mixed_merge_kernel   fear_jpeg_decode_mixed_u8: the same block stage (js_blocks) and, by the image's
//                              own m, this pixel stage (js_merge_image) or the full-size one (jd_merge_image); m from the record's
//                              reserved[0], the second prefix table counting each image's own scaled pixels
// Integer width: libjpeg computes these transforms in `long`; the device computes in 32 bits, as the islow pair of fear_train_jpeg.h
// does.  The two agree while the dequantised coefficients stay within +-2^13 (an 8-bit sample's DCT cannot leave +-2^13; the largest
// term is dc << 14 twice over, 2^13 2^2 2^14 = 2^29), which every file an encoder writes does.
// As in fear_jpeg_decode.h the device never trusts the data: every loop is bounded by a constant, a block reads at most 64 stored values
// whatever its offsets say, there are no atomics and every store is a plain vector store.
// Included by fear_train.hip behind fear_jpeg_decode.h.  Its own are the transforms, their dispatch and the store widths; the argument
// struct (JpegDecodeArgs with m), the records, geometry and image search, the block load, the block's home, the sample pack, the h2v1
// filter, the colour conversion and the host's check (jd_check) are fear_jpeg_decode.h's.

namespace {

// The side of a component's transform (libjpeg's jdmaster.c): m, doubled while it is below 8 and the plane stays within the frame on
// both axes.  hc, vc: the component's sampling factors; h, v: the largest (the luma's).  At most three doublings.
__host__ __device__ __forceinline__ int js_transform(int m, int h, int v, int hc, int vc) {
    int ss = m;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (ss < 8 && (h * m) % (hc * ss * 2) == 0 && (v * m) % (vc * ss * 2) == 0) ss *= 2;
    return ss;
}

// jidctred.c's 4 x 4 transform, one pass over d[0..7] (d[4] is never read) -> d[0..3].  N: 12 down a column, 19 along a row.
template <int N>
__device__ __forceinline__ void js_idct4(int* d) {
    const int t0 = d[0] * 16384, t2 = 15137 * d[2] - 6270 * d[6];
    const int t10 = t0 + t2, t12 = t0 - t2;
    const int o0 = -1730 * d[7] + 11893 * d[5] - 17799 * d[3] + 8697 * d[1];
    const int o2 = -4176 * d[7] - 4926 * d[5] + 7373 * d[3] + 20995 * d[1];
    d[0] = jp_descale<N>(t10 + o2);
    d[1] = jp_descale<N>(t12 + o0);
    d[2] = jp_descale<N>(t12 - o0);
    d[3] = jp_descale<N>(t10 - o2);
}

// jidctred.c's 2 x 2 transform, one pass over d[0], d[1], d[3], d[5], d[7] -> d[0..1].  N: 13 down a column, 20 along a row.
template <int N>
__device__ __forceinline__ void js_idct2(int* d) {
    const int t10 = d[0] * 32768;
    const int t0 = -5906 * d[7] + 6967 * d[5] - 10426 * d[3] + 29692 * d[1];
    d[0] = jp_descale<N>(t10 + t0);
    d[1] = jp_descale<N>(t10 - t0);
}

// The block stage at m / 8 of the size: a workgroup finds its image and takes `m` from the kernel's argument (0: from the image's record,
// fear_jpeg_decode_mixed_u8).  m is the same for the whole workgroup, which belongs to one image; ss, the transform's side, is the same
// for the eight lanes of a block.  At m == 8 js_transform gives ss == 8 for every component (its loop needs ss < 8), the planes are 64
// bytes per block with the chroma at n0 64 and (n0 + nc) 64, and the block's home is jd_blocks': the layout jd_merge_image reads.
__device__ __forceinline__ void js_blocks(const JpegDecodeArgs& a) {
    __shared__ __attribute__((aligned(16))) int blk[FEAR_JPEG_GROUP_BLOCKS * kJpPitch];
    const int tid = threadIdx.x, lb = tid >> 3, k = tid & 7;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const int m = a.m ? a.m : jd_record_m(im->reserved[0]);
    const JdGeom g = jd_geom(im->width, im->height, im->components, im->h, im->v);
    const long b = (long)(blockIdx.x - a.table[img]) * FEAR_JPEG_GROUP_BLOCKS + lb;
    const bool on = b < g.n0 + 2 * g.nc;
    const int comp = jd_comp(g, b);
    const int ss0 = js_transform(m, im->h, im->v, im->h, im->v), ssc = js_transform(m, im->h, im->v, 1, 1);
    const int ss = comp == 0 ? ss0 : ssc;                      // 1, 2, 4 or 8; the same for the eight lanes of a block
    int* base = blk + lb * kJpPitch;
    jd_load_block(base, k, on, im, b, comp);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = base[i * 8 + k];       // columns: lane k takes column k (one the row pass never reads is wasted work)
    if (ss == 8) jpeg_idct<true>(d);
    else if (ss == 4) js_idct4<12>(d);
    else if (ss == 2) js_idct2<13>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < ss) base[i * 8 + k] = d[i];                   // ss == 1 writes d[0] back: the dc
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = base[(k < ss ? k : 0) * 8 + i];   // rows: lane k < ss takes row k
    if (ss == 8) jpeg_idct<false>(d);
    else if (ss == 4) js_idct4<19>(d);
    else if (ss == 2) js_idct2<20>(d);
    else d[0] = jp_descale<3>(d[0]);
    if (on && k < ss) {
        const JdHome at = jd_home(g, comp, b);
        // the planes of an image follow one another: luma n0 ss0^2 bytes, then Cb and Cr of nc ssc^2 bytes each
        const long plane = comp == 0 ? 0 : (long)g.n0 * ss0 * ss0 + (comp == 2 ? (long)g.nc * ssc * ssc : 0);
        // plane_offset is a multiple of 16 and a row of a block starts at a multiple of ss within its plane; a chroma plane starts at a
        // multiple of ssc as well: n0 ss0^2 is one where ssc == ss0, and where ssc == 2 ss0 (4:2:0) n0 is a multiple of 4
        uint8_t* dst = a.planes + im->plane_offset + plane + ((at.by * ss + k) * at.pw + at.bx) * ss;
        const uint32_t lo = jd_pack4(d);
        if (ss == 8) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(lo, jd_pack4(d + 4));
        } else if (ss == 4) {
            *reinterpret_cast<uint32_t*>(dst) = lo;
        } else if (ss == 2) {
            *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(lo & 0xffffu);
        } else {
            *dst = (uint8_t)(lo & 0xffu);
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_scaled_blocks_kernel(JpegDecodeArgs a) { js_blocks(a); }

// The pixel stage at m / 8 of the size, m < 8, for a workgroup that knows its image (`first`: its first workgroup): one scaled pixel
// per lane.
__device__ __forceinline__ void js_merge_image(const JpegDecodeArgs& a, const FearJpegImage* im, int m, uint32_t first) {
    const int h = im->h, v = im->v;
    const int W = (im->width * m + 7) >> 3, H = (im->height * m + 7) >> 3;      // the scaled frame
    const long px = (long)(blockIdx.x - first) * FEAR_JPEG_GROUP_PIXELS + threadIdx.x;
    if (px >= (long)H * W) return;
    const int y = (int)(px / W), x = (int)(px - (long)y * W);
    const JdGeom g = jd_geom(im->width, im->height, im->components, h, v);
    const int ss0 = js_transform(m, h, v, h, v), ssc = js_transform(m, h, v, 1, 1);
    const uint8_t* planes = a.planes + im->plane_offset;
    const int Y = planes[(long)y * (g.bw0 * ss0) + x];
    int cb = 128, cr = 128;
    if (im->components == 3) {
        const uint8_t* pcb = planes + (long)g.n0 * ss0 * ss0;
        const uint8_t* pcr = pcb + (long)g.nc * ssc * ssc;
        const long row = (long)y * (g.bwc * ssc);              // no supported mode is left with vertical upsampling: h m == ssc or v == 1
        if (h * m == ssc) {                                    // 4:4:4, and 4:2:0 through the larger transform: no upsampling
            cb = pcb[row + x]; cr = pcr[row + x];
        } else {                                               // 4:2:2: h2v1 on the true width of the scaled chroma plane
            const int cw = (im->width * ssc + 8 * h - 1) / (8 * h);
            if (m > 1 && cw > 2) {                             // fancy
                const JdTaps t = jd_taps(x, cw);
                cb = jd_h2v1(pcb, row, t); cr = jd_h2v1(pcr, row, t);
            } else {                                           // replication: a plane this narrow, and every plane at 1/8
                cb = pcb[row + (x >> 1)]; cr = pcr[row + (x >> 1)];
            }
        }
    }
    jd_store_rgb(Y, cb, cr, im->out + px * 3);
}

__global__ __launch_bounds__(256) void jpeg_scaled_merge_kernel(JpegDecodeArgs a) {
    const uint32_t* start = a.table + (a.n + 1);
    const int img = jd_find_image(start, a.n, blockIdx.x);
    js_merge_image(a, jd_records(a) + img, a.m, start[img]);
}

// fear_jpeg_decode_mixed_u8: the same two stages with each image's m from its record (a.m == 0).  A workgroup belongs to one image, so
// m is workgroup-uniform: one scalar load and one uniform branch, in front of the per-lane work, choose between the full-size pixel
// stage (jd_merge_image: h2v2 and h2v1 at the true chroma edges, replication for cw <= 2) and the scaled one.
__global__ __launch_bounds__(256) void jpeg_mixed_blocks_kernel(JpegDecodeArgs a) { js_blocks(a); }

__global__ __launch_bounds__(256) void jpeg_mixed_merge_kernel(JpegDecodeArgs a) {
    const uint32_t* start = a.table + (a.n + 1);
    const int img = jd_find_image(start, a.n, blockIdx.x);
    const FearJpegImage* im = jd_records(a) + img;
    const int m = jd_record_m(im->reserved[0]);
    if (m == 8) jd_merge_image<false>(a, nullptr, im, img, start[img]);
    else js_merge_image(a, im, m, start[img]);
}

}  // namespace

extern "C" {

int fear_jpeg_decode_scaled_u8(const FearJpegImage* images, int n, const uint32_t* group_start, int scale, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (scale != 2 && scale != 4 && scale != 8) return FEAR_TRAIN_ERR_SHAPE;
    JdLaunch l;
    const int status = jd_check(images, n, group_start, false, 8 / scale, workspace, workspace_bytes, &l);
    if (status != FEAR_TRAIN_OK || l.block_groups == 0) return status;
    hipLaunchKernelGGL(jpeg_scaled_blocks_kernel, dim3(l.block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_scaled_merge_kernel, dim3(l.pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_jpeg_decode_mixed_u8(const FearJpegImage* images, int n, const uint32_t* group_start, void* workspace, size_t workspace_bytes,
                              void* stream) {
    JdLaunch l;
    const int status = jd_check(images, n, group_start, false, 0, workspace, workspace_bytes, &l);
    if (status != FEAR_TRAIN_OK || l.block_groups == 0) return status;
    hipLaunchKernelGGL(jpeg_mixed_blocks_kernel, dim3(l.block_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_mixed_merge_kernel, dim3(l.pixel_groups), dim3(256), 0, static_cast<hipStream_t>(stream), l.a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
