// fear_jpeg_store.h — scans resident on the device and the index a baseline scan lacks (include/fear_train.h: fear_jpeg_index_build,
// fear_jpeg_huffman_indexed, fear_jpeg_huffman_indexed_rows, fear_jpeg_huffman_indexed_rows_dev, fear_jpeg_huffman_indexed_windows; DESIGN.md section 14, "The resident store").  fear_jpeg_index_build is the second instantiation of
// jpeg_huffman_kernel (fear_jpeg_huffman.h), which stores every lane's true entry in front of its write pass.  With those entries a later
// decode is the write pass alone: jpeg_huffman_indexed_kernel gives every subsequence of an image a lane of its own, whatever segment it
// lies in.  jpeg_huffman.jpeg_scan_index_host and jpeg_entropy_indexed_host restate both in Python.  fear_jpeg_huffman_indexed_rows is
// the same lane for a band of MCU rows: only the subsequences in which the band's blocks lie get a lane (the caller's row_sub table,
// jpeg_huffman.scan_row_sub), and only the band's blocks are stored, as the dense coefficients of an image of those rows alone.
// fear_jpeg_huffman_indexed_windows is the band's lane for a range of MCU columns as well: a lane of the band that its own entry and the
// next one show to hold no MCU of those columns returns early, and the blocks are stored window-dense.
// The four kernels share one lane (ji_lane<FORM, STAGED>) and the four entry points one host function (ji_launch).  The *_host entry
// points are the same four for bytes in pinned host memory ("Bytes on the host"): the lane's second byte-fetch
// policy, under which a workgroup copies its lanes' byte range into LDS first (ji_stage_range, fear_jpeg_stage_range).
// Included by fear_train.hip behind fear_jpeg_huffman.h, whose jh_decode, jh_peek, jh_block_base and JhSegment it uses, and
// fear_jpeg_decode.h's jd_find_image and jr_band.

namespace {

struct JpegIndexedArgs {
    const uint32_t* table;   // the caller's device table: n + 1 prefix sums of workgroups, padding, n FearJpegIndexed records
    int16_t* coef;
    int32_t* status;
    int n, subsequence_bits;
    int stage_bytes;         // the staged kernels alone: the launch's dynamic LDS, a multiple of 16, at most kJiStageCap
};

constexpr int kJiStageCap = 64 << 10;   // the most a workgroup stages; what lies behind goes through the direct fetch

// The bytes byte0 .. byte1) that the subsequences sub_first .. sub_first + sub_count) of a prepared scan cover: consecutive
// subsequences are consecutive bytes, across segments too (an empty segment has no subsequence), so the union of the lanes'
// [seg_start[seg] + k SB, min(... + SB, seg_start[seg + 1])) is one range, from the first lane's first byte to the last lane's end.
// Two searches of sub_start side by side, 21 steps at most (n_seg <= 2^20); both ends clamped to n_bytes; 0, 0 for no lane, for
// n_seg == 0 and for a sub_start that is not this scan's.  The staged kernels and fear_jpeg_stage_range share it;
// jpeg_huffman.stage_range_host restates it.
__host__ __device__ inline void ji_stage_range(const uint32_t* seg_start, const uint32_t* sub_start, uint32_t n_seg, uint32_t n_bytes,
                                               uint32_t sub_first, uint32_t sub_count, uint32_t subsequence_bytes, uint32_t* byte0,
                                               uint32_t* byte1) {
    *byte0 = *byte1 = 0;
    if (sub_count == 0 || n_seg == 0) return;
    const uint32_t sub_last = sub_first + (sub_count - 1);
    uint32_t s0 = 0, h0 = n_seg, s1 = 0, h1 = n_seg;                     // the last segment that starts at or in front of each
    for (int step = 0; step < 21 && (h0 - s0 > 1 || h1 - s1 > 1); ++step) {
        if (h0 - s0 > 1) {
            const uint32_t mid = (s0 + h0) >> 1;
            if (sub_start[mid] <= sub_first) s0 = mid; else h0 = mid;
        }
        if (h1 - s1 > 1) {
            const uint32_t mid = (s1 + h1) >> 1;
            if (sub_start[mid] <= sub_last) s1 = mid; else h1 = mid;
        }
    }
    const uint32_t f0 = sub_start[s0], f1 = sub_start[s1];
    if (f0 > sub_first || f1 > sub_last) return;
    const uint64_t lo = (uint64_t)seg_start[s0] + (uint64_t)(sub_first - f0) * subsequence_bytes;
    uint64_t hi = (uint64_t)seg_start[s1] + ((uint64_t)(sub_last - f1) + 1) * subsequence_bytes;
    if (hi > seg_start[s1 + 1]) hi = seg_start[s1 + 1];
    if (hi > n_bytes) hi = n_bytes;
    if (lo >= hi) return;
    *byte0 = (uint32_t)lo;
    *byte1 = (uint32_t)hi;
}

__device__ __forceinline__ const FearJpegIndexed* ji_records(const JpegIndexedArgs& a) {
    return reinterpret_cast<const FearJpegIndexed*>(reinterpret_cast<const char*>(a.table) + FEAR_JPEG_SCAN_TABLE_RECORDS(a.n));
}

// The statuses' zeros; an image without a subsequence has no lane to judge it and owes blocks: it fails here.
__global__ __launch_bounds__(kJhLanes) void jpeg_indexed_status_kernel(JpegIndexedArgs a) {
    const int i = blockIdx.x * kJhLanes + threadIdx.x;
    if (i < a.n) a.status[i] = ji_records(a)[i].n_sub == 0 ? FEAR_TRAIN_ERR_FORMAT : FEAR_TRAIN_OK;
}

// One lane of the indexed decode.  FORM 1: fear_jpeg_huffman_indexed_rows' instantiation, whose lanes are the record's sub_count
// subsequences from sub0 and which stores only the blocks of the record's band of MCU rows, band-dense (jh_band_base).  FORM 2:
// fear_jpeg_huffman_indexed_rows_dev's, whose band comes from `rows_dev` (device memory; null in the other forms): the grid is the whole
// image's, a workgroup outside the band's subsequences returns in front of the table copy, a lane outside them behind the barrier, and
// the band's blocks are stored at their place in the whole image (jh_rows_base).  FORM 3: fear_jpeg_huffman_indexed_windows', FORM 1
// with the MCU columns of the record's `reserved` word (mcu_col0 | mcu_cols << 16): a lane whose MCUs — known from its entry's `begun`
// and the next entry's, or the segment's block count — all lie outside those columns returns in front of every judgement, and only the
// blocks of the band's rows and those columns are stored, window-dense (jh_window_base).
//
// STAGED is the byte-fetch policy.  false: every lane reads its words from the record's `bytes` (jh_word).  true, for bytes in pinned
// host memory (the *_host entry points): in front of the barrier the workgroup copies the one byte range its running lanes cover
// (ji_stage_range; form 2 counts the lanes of the band alone, form 3 all the band's lanes of the workgroup: no vote) into
// dynamic LDS with 16-byte loads from the 16-byte aligned address at or in front of the range, two words further than its end for the
// last lane's window, at most stage_bytes, never a word at or behind 4 ceil(n_bytes / 4) nor one in front of `bytes` (the chunks at those
// two edges are loaded word by word); a lane's fetch takes a word from LDS where it is there and from `bytes` otherwise.
template <int FORM, bool STAGED>
__device__ __forceinline__ void ji_lane(const JpegIndexedArgs& a, const int32_t* rows_dev) {
    constexpr bool WIN = FORM == 3, ROWS = FORM == 1 || WIN, DEV = FORM == 2;
    __shared__ __attribute__((aligned(16))) FearJpegHuff tabs[6];        // dc by component, then ac by component
    const int tid = threadIdx.x;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);             // the same for the whole workgroup
    const FearJpegIndexed* im = ji_records(a) + img;
    const FearJpegScan* rec = im->scan;
    uint32_t dev_first = 0, dev_last = 0, dev_row0 = 0, dev_rows = 0;    // DEV: the lanes that run, inclusive, and the band
    if (DEV) {                                                           // everything here is the same for the whole workgroup
        const int mcus_y = min(max(rec->mcus_y, 1), FEAR_JPEG_MAX_SIDE / 8), v = rec->v == 2 ? 2 : 1;
        int ba, bb;
        if (!jr_band(rows_dev[2 * img], rows_dev[2 * img + 1], 8 * v * mcus_y, 8 * v, mcus_y, v == 2, &ba, &bb)) return;
        if (im->n_sub == 0) return;
        dev_first = im->row_sub[ba];                                     // the table has mcus_y + 1 values and 0 <= ba < bb <= mcus_y
        dev_last = min(im->row_sub[bb], im->n_sub - 1u);
        const uint64_t lane0 = (uint64_t)(blockIdx.x - a.table[img]) * kJhLanes;
        if (lane0 > dev_last || lane0 + (kJhLanes - 1) < dev_first) return;   // an idle workgroup: a few loads, no table copy, no barrier
        dev_row0 = (uint32_t)ba;
        dev_rows = (uint32_t)(bb - ba);
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(rec->dc);      // the record is 16-byte aligned, the tables lie 64 bytes in
        uint4* dst = reinterpret_cast<uint4*>(tabs);
        for (int i = tid; i < (int)(sizeof(tabs) / 16); i += kJhLanes) dst[i] = src[i];
    }
    const uint32_t* stage = nullptr;
    uint32_t stage_w0 = 0, stage_n = 0;
    if constexpr (STAGED) {                                              // everything here is the same for the whole workgroup
        extern __shared__ __attribute__((aligned(16))) uint4 ji_stage[];
        const uint64_t lane0 = (uint64_t)(blockIdx.x - a.table[img]) * kJhLanes;
        uint64_t first = lane0, last = lane0 + (kJhLanes - 1);           // the lanes that run, inclusive
        if (ROWS) {
            first += im->sub0;
            last = min(last, (uint64_t)im->sub_count - 1u) + im->sub0;   // (sub_count > 0: the workgroup exists)
        }
        if (DEV) {
            first = max(first, (uint64_t)dev_first);
            last = min(last, (uint64_t)dev_last);
        }
        const uint32_t all = im->n_sub;
        uint32_t b0 = 0, b1 = 0;
        const uint32_t n_bytes = rec->n_bytes;
        if (all > 0 && first < all && first <= last)
            ji_stage_range(rec->seg_start, im->sub_start, rec->n_seg, n_bytes, (uint32_t)first, (uint32_t)(min(last, (uint64_t)all - 1u) - first) + 1u,
                           (uint32_t)a.subsequence_bits >> 3, &b0, &b1);
        if (b1 > b0) {
            // offsets from the 16-byte aligned address at or in front of `bytes`, which is 4-byte aligned: `mis` further than the bytes'
            const uintptr_t addr = reinterpret_cast<uintptr_t>(rec->bytes);
            const uint64_t mis = addr & 15u, limit = mis + 4u * (((uint64_t)n_bytes + 3u) >> 2);
            const uint64_t v0 = (b0 + mis) & ~(uint64_t)15, v1 = min(((b1 + mis + 3u) & ~(uint64_t)3) + 8u, limit);
            const uint32_t chunks = (uint32_t)min((v1 - v0 + 15u) >> 4, (uint64_t)(a.stage_bytes >> 4));
            const char* base = reinterpret_cast<const char*>(addr - mis);
            for (uint32_t i = tid; i < chunks; i += kJhLanes) {
                const uint64_t v = v0 + 16u * (uint64_t)i;
                uint4 q;
                if (v >= mis && v + 16u <= limit) {
                    q = *reinterpret_cast<const uint4*>(base + v);
                } else {                                                 // the chunk at an edge of the image's words: word by word
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint64_t vv = v + 4u * (uint32_t)j;
                        w[j] = vv >= mis && vv < limit ? *reinterpret_cast<const uint32_t*>(base + vv) : 0u;
                    }
                    q = make_uint4(w[0], w[1], w[2], w[3]);
                }
                ji_stage[i] = q;
            }
            stage = reinterpret_cast<const uint32_t*>(ji_stage);
            stage_w0 = (uint32_t)((int64_t)(v0 - mis) >> 2);             // up to three words in front of `bytes`: wraps, as jh_word expects
            stage_n = 4u * chunks;
        }
    }
    __syncthreads();                                                     // the only barrier
    const uint32_t n_sub = im->n_sub, n_seg = rec->n_seg;
    uint64_t sub64 = (uint64_t)(blockIdx.x - a.table[img]) * kJhLanes + (uint32_t)tid;
    if (ROWS) {
        if (sub64 >= im->sub_count) return;                              // lanes that do not run judge nothing
        sub64 += im->sub0;
    }
    if (DEV && (sub64 < dev_first || sub64 > dev_last)) return;          // lanes that do not run judge nothing
    if (sub64 >= n_sub || n_seg == 0) return;
    const uint32_t sub = (uint32_t)sub64;
    const uint4 e = reinterpret_cast<const uint4*>(im->index)[sub];
    // the last segment that starts at or in front of `sub`: n_seg <= 2^20
    const uint32_t* sub_start = im->sub_start;
    uint32_t seg = 0, hi = n_seg;
#pragma unroll 1
    for (int step = 0; step < 21 && hi - seg > 1; ++step) {
        const uint32_t mid = (seg + hi) >> 1;
        if (sub_start[mid] <= sub) seg = mid; else hi = mid;
    }
    const uint32_t first = sub_start[seg];
    const uint32_t SB = (uint32_t)a.subsequence_bits;
    JhSegment s;
    {
        const uint32_t n_bytes = rec->n_bytes;
        const uint32_t b0 = min(rec->seg_start[seg], n_bytes), b1 = min(max(rec->seg_start[seg + 1], b0), n_bytes);
        s.words = reinterpret_cast<const uint32_t*>(rec->bytes);
        s.n_words = (n_bytes + 3) >> 2;
        s.stage = stage;
        s.stage_w0 = stage_w0;
        s.stage_n = stage_n;
        s.byte0 = b0;
        s.bits = min(b1 - b0, FEAR_JPEG_DEVICE_SCAN_MAX) * 8u;
        const int nf = rec->components;
        s.h = max(rec->h, 1);
        s.v = max(rec->v, 1);
        s.hv = nf == 3 ? min(s.h * s.v, 4) : 1;
        s.nslots = nf == 3 ? s.hv + 2 : 1;
        s.mcus_x = max(rec->mcus_x, 1);
        const uint32_t n_mcu = (uint32_t)s.mcus_x * (uint32_t)max(rec->mcus_y, 1);
        s.n0 = n_mcu * (uint32_t)s.hv;
        s.nc = n_mcu;
        s.total_blocks = rec->total_blocks;
        const uint32_t interval = rec->restart_interval > 0 ? (uint32_t)rec->restart_interval : n_mcu;
        const uint64_t first_mcu = (uint64_t)seg * interval;
        s.first_mcu = first_mcu < n_mcu ? (uint32_t)first_mcu : n_mcu;
        s.expected = min(interval, n_mcu - s.first_mcu) * (uint32_t)s.nslots;
        s.last = seg + 1 == n_seg;
        if (ROWS) {                                                      // the band inside the image: an explicit range, no wrap-around
            const uint32_t mcus_y = (uint32_t)max(rec->mcus_y, 1);
            s.band_row0 = min(im->mcu_row0, mcus_y);
            s.band_rows = min(im->mcu_rows, mcus_y - s.band_row0);
        }
        if (DEV) {                                                       // 0 <= row0 < row0 + rows <= mcus_y by jr_band
            s.band_row0 = dev_row0;
            s.band_rows = dev_rows;
        }
        if (WIN) {                                                       // the columns inside the image, as the band's rows
            s.win_col0 = min(im->reserved & 0xFFFFu, (uint32_t)s.mcus_x);
            s.win_cols = min(im->reserved >> 16, (uint32_t)s.mcus_x - s.win_col0);
        }
    }
    if (WIN) {
        // The blocks this lane stores have the ordinals lo .. hi) of its segment: from the block open at its entry, or the first it
        // begins, to the last begun in front of the next subsequence's entry (the segment's count behind its last subsequence; blocks
        // past that count are dropped).  Their MCUs are consecutive; the lane runs if one of them lies in the window's columns, the
        // wrap over a row's end included.  Arithmetic on two loaded values: no loop.
        const bool next_inside = sub + 1 < sub_start[seg + 1] && sub + 1 < n_sub;
        const uint32_t next_begun = next_inside ? reinterpret_cast<const uint4*>(im->index)[sub + 1].y : s.expected;
        const uint32_t lo = e.y - ((e.z & 0xFFu) != 0 && e.y > 0 ? 1u : 0u), hi = min(next_begun, s.expected);
        if (hi <= lo || s.win_cols == 0) return;                         // lanes that do not run judge nothing
        const uint32_t mcus_x = (uint32_t)s.mcus_x, nslots = (uint32_t)s.nslots;
        const uint32_t m_lo = s.first_mcu + lo / nslots, count = (hi - 1) / nslots - lo / nslots + 1;
        const uint32_t x_lo = m_lo % mcus_x, x_end = x_lo + count - 1;   // count < mcus_x below: x_end < 2 mcus_x
        const uint32_t c0 = s.win_col0, c1 = s.win_col0 + s.win_cols;
        const bool touches = count >= mcus_x || (x_lo < c1 && x_end >= c0) || (x_end >= mcus_x && x_end - mcus_x >= c0);
        if (!touches) return;
    }
    int32_t* status = a.status + img;
    const uint64_t k = (uint64_t)sub - first;                            // the subsequence within its segment
    if (first > sub || k * SB >= s.bits) {                               // an index that is not this scan's
        *status = FEAR_TRAIN_ERR_FORMAT;
        return;
    }
    JhState entry;
    entry.p = e.x;
    entry.sz = min((e.z >> 8) & 0xFFu, (uint32_t)s.nslots - 1u) << 8 | min(e.z & 0xFFu, 63u);
    JhLane lane{};
    lane.begun = e.y;
    lane.dc0 = e.z >> 16;
    lane.dc1 = e.w & 0xFFFFu;
    lane.dc2 = e.w >> 16;
    const uint32_t end = ((uint32_t)k + 1u) * SB;                        // k SB < bits <= 2^27 (8 FEAR_JPEG_DEVICE_SCAN_MAX), SB <= 2^13: no overflow
    const JhState out = jh_decode<DEV ? 4 : (WIN ? 5 : (ROWS ? 3 : 2)), STAGED>(s, tabs, entry, end, a.coef + im->coef_offset, lane);
    bool failed = lane.error;
    // the segment's last subsequence: fewer complete blocks than the segment owes, as jpeg_huffman_kernel judges its true chain's end
    if (end >= s.bits && (lane.begun - ((out.sz & 255) != 0 ? 1u : 0u) < s.expected || (lane.begun == 0 && s.expected > 0))) failed = true;
    if (k == 0 && seg > 0 && sub_start[seg - 1] == first) failed = true;  // an empty segment in front owes blocks
    if (sub + 1 == n_sub && !s.last) failed = true;                       // empty segments behind the image's last subsequence
    if (failed) *status = FEAR_TRAIN_ERR_FORMAT;                          // every lane that stores stores the same value
}

__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_indexed_kernel(JpegIndexedArgs a) { ji_lane<0, false>(a, nullptr); }

__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_indexed_rows_kernel(JpegIndexedArgs a) { ji_lane<1, false>(a, nullptr); }

__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_indexed_windows_kernel(JpegIndexedArgs a) { ji_lane<3, false>(a, nullptr); }

__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_indexed_rows_dev_kernel(JpegIndexedArgs a, const int32_t* rows_dev) {
    ji_lane<2, false>(a, rows_dev);
}

// The same lane with the staged fetch, one kernel for the four forms (rows_dev is null but in form 2): the same grid and workgroup,
// stage_bytes of dynamic LDS.
template <int FORM>
__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_indexed_staged_kernel(JpegIndexedArgs a, const int32_t* rows_dev) {
    ji_lane<FORM, true>(a, rows_dev);
}

using JiStagedKernel = void (*)(JpegIndexedArgs, const int32_t*);
constexpr JiStagedKernel kJiStaged[4] = {jpeg_huffman_indexed_staged_kernel<0>, jpeg_huffman_indexed_staged_kernel<1>,
                                         jpeg_huffman_indexed_staged_kernel<2>, jpeg_huffman_indexed_staged_kernel<3>};

// With the six tables a workgroup at the cap holds more than 64 KiB of LDS: the four kernels are told so once per device.
bool ji_staged_ready() {
    static std::atomic<uint64_t> done{0};                                // (two threads that both find a bit unset set the same values)
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device > 63) return false;
    if (done.load() >> device & 1u) return true;
    for (JiStagedKernel k : kJiStaged)
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, kJiStageCap) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    done.fetch_or((uint64_t)1 << device);
    return true;
}

}  // namespace

extern "C" {

int fear_jpeg_index_build(const FearJpegScan* scans, int n, const void* table_dev, const FearJpegIndex* indexes, const void* index_table_dev,
                          int16_t* coef, int32_t* status_dev, int subsequence_bytes, void* stream) {
    if (n < 0 || n > 65535 || subsequence_bytes < 4 || subsequence_bytes > 1024 || (subsequence_bytes & 3) != 0) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!scans || !table_dev || !indexes || !index_table_dev || !coef || !status_dev) return FEAR_TRAIN_ERR_NULL;
    uint64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        if (!scans[i].bytes || !scans[i].seg_start) return FEAR_TRAIN_ERR_NULL;
        if (!jh_scan_ok(scans[i])) return FEAR_TRAIN_ERR_SHAPE;
        groups += scans[i].n_seg;
    }
    if (groups > 0x7fffffffu) return FEAR_TRAIN_ERR_SHAPE;
    for (int i = 0; i < n; ++i) {
        const FearJpegIndex& ix = indexes[i];
        if (!ix.sub_start || !ix.seg_start_host || (!ix.index && ix.n_sub != 0)) return FEAR_TRAIN_ERR_NULL;
        if ((reinterpret_cast<uintptr_t>(ix.index) & 15) != 0 || (reinterpret_cast<uintptr_t>(ix.sub_start) & 3) != 0) return FEAR_TRAIN_ERR_SHAPE;
        uint32_t n_sub = 0;                                               // the host's count (fear_jpeg_entropy.h), from the host's seg_start
        if (fear_jpeg_sub_start(ix.seg_start_host, scans[i].n_seg, scans[i].n_bytes, subsequence_bytes, nullptr, 0, &n_sub) != FEAR_TRAIN_OK ||
            n_sub != ix.n_sub)
            return FEAR_TRAIN_ERR_SHAPE;
    }
    JpegHuffArgs a{};
    a.table = static_cast<const uint32_t*>(table_dev);
    a.coef = coef;
    a.status = status_dev;
    a.n = n;
    a.subsequence_bits = subsequence_bytes * 8;
    a.indexes = static_cast<const FearJpegIndex*>(index_table_dev);
    hipLaunchKernelGGL(jpeg_huffman_status_kernel, dim3((unsigned)((n + kJhLanes - 1) / kJhLanes)), dim3(kJhLanes), 0,
                       static_cast<hipStream_t>(stream), status_dev, n);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_huffman_kernel<true>, dim3((unsigned)groups), dim3(kJhLanes), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

// The checks and the two launches of the four indexed entry points.  form: ji_lane's, 0 the image, 1 the host-planned band (the
// record's sub0 / sub_count and mcu_row0 / mcu_rows are checked and the grid counts sub_count), 2 the band of `rows_dev` (which, with
// every record's row_sub, must be there), 3 the host-planned window (form 1's checks and the columns of the record's `reserved` word).
// staged: the *_host entry points' kernels, with min(256 subsequence_bytes + 32, kJiStageCap) bytes of dynamic LDS — a workgroup's
// range, the bytes in front of it down to a 16-byte address and the last lane's two words behind it.
static int ji_launch(int form, bool staged, const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev, int16_t* coef,
                     int32_t* status_dev, int subsequence_bytes, void* stream) {
    if (n < 0 || n > 65535 || subsequence_bytes < 4 || subsequence_bytes > 1024 || (subsequence_bytes & 3) != 0) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!images || !table_dev || (form == 2 && !rows_dev) || !coef || !status_dev) return FEAR_TRAIN_ERR_NULL;
    uint64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        const FearJpegIndexed& im = images[i];
        if (!im.scan || !im.sub_start || (form == 2 && !im.row_sub) || (!im.index && im.n_sub != 0)) return FEAR_TRAIN_ERR_NULL;
        if ((reinterpret_cast<uintptr_t>(im.index) & 15) != 0 || (reinterpret_cast<uintptr_t>(im.scan) & 15) != 0 ||
            (reinterpret_cast<uintptr_t>(im.sub_start) & 3) != 0 || (form == 2 && (reinterpret_cast<uintptr_t>(im.row_sub) & 3) != 0))
            return FEAR_TRAIN_ERR_SHAPE;
        if (form == 1 || form == 3) {
            if (im.sub_count != 0 && (im.sub0 >= im.n_sub || im.sub_count > im.n_sub - im.sub0)) return FEAR_TRAIN_ERR_SHAPE;
            if (im.mcu_row0 > FEAR_JPEG_MAX_SIDE / 8 || im.mcu_rows > FEAR_JPEG_MAX_SIDE / 8 - im.mcu_row0) return FEAR_TRAIN_ERR_SHAPE;
        }
        if (form == 3) {
            const uint32_t col0 = im.reserved & 0xFFFFu, cols = im.reserved >> 16;
            if (cols == 0 || col0 > FEAR_JPEG_MAX_SIDE / 8 || cols > FEAR_JPEG_MAX_SIDE / 8 - col0) return FEAR_TRAIN_ERR_SHAPE;
        }
        groups += ((uint64_t)(form == 1 || form == 3 ? im.sub_count : im.n_sub) + kJhLanes - 1) / kJhLanes;
    }
    if (groups > 0x7fffffffu) return FEAR_TRAIN_ERR_SHAPE;
    JpegIndexedArgs a{};
    a.table = static_cast<const uint32_t*>(table_dev);
    a.coef = coef;
    a.status = status_dev;
    a.n = n;
    a.subsequence_bits = subsequence_bytes * 8;
    a.stage_bytes = staged ? min(kJhLanes * subsequence_bytes + 32, kJiStageCap) : 0;
    if (staged && !ji_staged_ready()) return FEAR_TRAIN_ERR_HIP;
    const dim3 grid((unsigned)groups), lanes(kJhLanes);
    hipLaunchKernelGGL(jpeg_indexed_status_kernel, dim3((unsigned)((n + kJhLanes - 1) / kJhLanes)), lanes, 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    if (groups == 0) return FEAR_TRAIN_OK;
    if (staged) hipLaunchKernelGGL(kJiStaged[form], grid, lanes, (size_t)a.stage_bytes, static_cast<hipStream_t>(stream), a, rows_dev);
    else if (form == 0) hipLaunchKernelGGL(jpeg_huffman_indexed_kernel, grid, lanes, 0, static_cast<hipStream_t>(stream), a);
    else if (form == 1) hipLaunchKernelGGL(jpeg_huffman_indexed_rows_kernel, grid, lanes, 0, static_cast<hipStream_t>(stream), a);
    else if (form == 3) hipLaunchKernelGGL(jpeg_huffman_indexed_windows_kernel, grid, lanes, 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(jpeg_huffman_indexed_rows_dev_kernel, grid, lanes, 0, static_cast<hipStream_t>(stream), a, rows_dev);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_jpeg_huffman_indexed(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                              int subsequence_bytes, void* stream) {
    return ji_launch(0, false, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_rows(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                   int subsequence_bytes, void* stream) {
    return ji_launch(1, false, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_rows_dev(const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev, int16_t* coef,
                                       int32_t* status_dev, int subsequence_bytes, void* stream) {
    return ji_launch(2, false, images, n, table_dev, rows_dev, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_windows(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                      int subsequence_bytes, void* stream) {
    return ji_launch(3, false, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

// The four calls for scans whose `bytes` lie in pinned, mapped host memory (JpegStore(residence="host")): the same records, checks,
// grids and results, the staged fetch.
int fear_jpeg_huffman_indexed_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                   int subsequence_bytes, void* stream) {
    return ji_launch(0, true, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_rows_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                        int subsequence_bytes, void* stream) {
    return ji_launch(1, true, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_rows_dev_host(const FearJpegIndexed* images, int n, const void* table_dev, const int32_t* rows_dev,
                                            int16_t* coef, int32_t* status_dev, int subsequence_bytes, void* stream) {
    return ji_launch(2, true, images, n, table_dev, rows_dev, coef, status_dev, subsequence_bytes, stream);
}

int fear_jpeg_huffman_indexed_windows_host(const FearJpegIndexed* images, int n, const void* table_dev, int16_t* coef, int32_t* status_dev,
                                           int subsequence_bytes, void* stream) {
    return ji_launch(3, true, images, n, table_dev, nullptr, coef, status_dev, subsequence_bytes, stream);
}

int fear_host_mapped_pointer(const void* host, void** device) {
    if (!device) return FEAR_TRAIN_ERR_NULL;
    *device = nullptr;
    if (!host) return FEAR_TRAIN_ERR_SHAPE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {          // no runtime to ask
        (void)hipGetLastError();
        return FEAR_TRAIN_ERR_HIP;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, host) != hipSuccess) {            // pageable memory the runtime has never seen
        (void)hipGetLastError();
        return FEAR_TRAIN_ERR_SHAPE;
    }
    if (attr.type != hipMemoryTypeHost || attr.isManaged || !attr.devicePointer) return FEAR_TRAIN_ERR_SHAPE;
    *device = attr.devicePointer;
    return FEAR_TRAIN_OK;
}

int fear_jpeg_stage_range(const uint32_t* seg_start, const uint32_t* sub_start, uint32_t n_seg, uint32_t n_bytes, uint32_t sub_first,
                          uint32_t sub_count, int subsequence_bytes, uint32_t* byte0, uint32_t* byte1) {
    if (!seg_start || !sub_start || !byte0 || !byte1) return FEAR_TRAIN_ERR_NULL;
    uint32_t n_sub = 0;                                                   // seg_start is this scan's, and sub_start its prefix sums
    const int rc = fear_jpeg_sub_start(seg_start, n_seg, n_bytes, subsequence_bytes, nullptr, 0, &n_sub);
    if (rc != FEAR_TRAIN_OK) return rc;
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        if (sub_start[s] != (uint32_t)total) return FEAR_TRAIN_ERR_SHAPE;
        total += ((uint64_t)(seg_start[s + 1] - seg_start[s]) + (uint32_t)subsequence_bytes - 1) / (uint32_t)subsequence_bytes;
    }
    if (sub_start[n_seg] != n_sub || sub_first > n_sub || sub_count > n_sub - sub_first) return FEAR_TRAIN_ERR_SHAPE;
    ji_stage_range(seg_start, sub_start, n_seg, n_bytes, sub_first, sub_count, (uint32_t)subsequence_bytes, byte0, byte1);
    return FEAR_TRAIN_OK;
}

}  // extern "C"
