// fear_jpeg_huffman.h — the Huffman stage of the JPEG frame decoder on the device (include/fear_train.h: fear_jpeg_huffman; DESIGN.md
// section 14): from the unstuffed scan bytes fear_jpeg_scan_prepare leaves (fear_jpeg_entropy.h) to dense quantised coefficients, the
// same values fear_jpeg_entropy_decode computes and the same verdict.  jpeg_huffman.jpeg_entropy_parallel_host restates it in Python.
//
// A baseline scan has no index; a decoder that starts in the middle does not know where a code begins, but Huffman streams re-synchronise
// by themselves (Weissenberger and Schmidt, ICPP 2018; 2021).  One workgroup of 256 lanes per restart segment walks the segment's
// sequences of 256 subsequences in order; per sequence
//   synchronise  lane 0 enters with the true state, the others guess; every lane decodes its subsequence and stores the exit state, then
//                goes on through the following subsequences until its exit equals the state stored there.  At most 255 rounds, after
//                which every stored state is the true one: lane 0's chain is true and reaches the end.  Nothing is declined.
//   count        each lane decodes its subsequence from the true entry state: the blocks that begin in it, the DC differences per
//                component modulo 2^16.  An exclusive prefix in LDS, carried from sequence to sequence.
//   write        each lane decodes its subsequence a last time and stores what it decodes, zeros of runs and behind an EOB included:
//                every position of every block is written by exactly one lane, no memset.  The verdict is judged here, on the true chain.
// Written for hostile input: a lane takes at most one symbol per bit of its subsequence, a sequence at most 255 rounds, a segment at most
// ceil(bits / (256 subsequence bits)) sequences; every read is checked against the segment's end (bits past it read as zero) and the
// image's bytes, every write against the image's 64 total_blocks values.  Only workgroup barriers: no workgroup waits for another.
// Included by fear_train.hip behind fear_jpeg_decode.h, whose jd_find_image and jd_mode_ok it uses.

namespace {

constexpr int kJhLanes = 256;

struct JpegHuffArgs {
    const uint32_t* table;   // the caller's device table: n + 1 prefix sums of segments, padding, n FearJpegScan records
    int16_t* coef;
    int32_t* status;
    int n, subsequence_bits;
    const FearJpegIndex* indexes;   // fear_jpeg_index_build alone (fear_jpeg_store.h): the device copy of the n index records
};

// What is the same for every lane of a workgroup: its segment and its image's geometry.
struct JhSegment {
    const uint32_t* words;   // the image's bytes, 4-byte aligned
    uint32_t n_words;
    uint32_t byte0;          // the segment's first byte among them
    uint32_t bits;           // the segment's length
    int nslots, hv, h, v, mcus_x;
    uint32_t n0, nc;         // blocks of the luma plane | of one chroma plane
    uint32_t total_blocks;
    uint32_t first_mcu;
    uint32_t expected;       // the blocks the segment owes
    bool last;
    uint32_t band_row0, band_rows;   // MODE 3, 4, 5 alone (fear_jpeg_store.h): the MCU rows whose blocks are stored, inside the image
    uint32_t win_col0, win_cols;     // MODE 5 alone: the MCU columns whose blocks are stored, inside the image
    const uint32_t* stage;   // the staged fetch alone (fear_jpeg_store.h): the LDS copy of the words stage_w0 .. stage_w0 + stage_n)
    uint32_t stage_w0, stage_n;
};

struct JhState {
    uint32_t p;              // bit position in the segment
    uint32_t sz;             // slot << 8 | z
};

// Word w < n_words of the image's bytes.  STAGED (the byte-fetch policy of fear_jpeg_store.h's staged kernels): from the workgroup's copy
// in LDS where the word lies in it, from `words` otherwise — whatever a lane reads behind the staged range is exact, only slower.
template <bool STAGED>
__device__ __forceinline__ uint32_t jh_word(const JhSegment& s, uint32_t w) {
    if (STAGED) {
        const uint32_t i = w - s.stage_w0;                               // a word in front of the range wraps to a large value
        if (i < s.stage_n) return s.stage[i];
    }
    return s.words[w];
}

// 32 bits from position p, the first in bit 31; bits past the segment's end are zero.
template <bool STAGED = false>
__device__ __forceinline__ uint32_t jh_peek(const JhSegment& s, uint32_t p) {
    if (p >= s.bits) return 0u;
    const uint32_t at = s.byte0 + (p >> 3), w = at >> 2;
    const uint32_t hi = w < s.n_words ? __builtin_bswap32(jh_word<STAGED>(s, w)) : 0u;
    const uint32_t lo = w + 1 < s.n_words ? __builtin_bswap32(jh_word<STAGED>(s, w + 1)) : 0u;
    const uint32_t shift = (at & 3) * 8 + (p & 7);                       // at most 31: 33 bits of the window are left
    uint32_t win = (uint32_t)((((uint64_t)hi << 32 | lo) << shift) >> 32);
    const uint32_t left = s.bits - p;
    if (left < 32) win &= ~(0xFFFFFFFFu >> left);
    return win;
}

// fear_jpeg::Bits::symbol on a window: the symbol and its length, or -1 for a code in no table.
__device__ __forceinline__ int jh_symbol(const FearJpegHuff& t, uint32_t win, int* len) {
    const uint32_t e = t.look[win >> (32 - fear_jpeg::kLookBits)];
    if (e) {
        *len = (int)(e >> 8);
        return (int)(e & 255);
    }
#pragma unroll 1
    for (int l = fear_jpeg::kLookBits + 1; l <= 16; ++l) {
        const int k = (int)(win >> (32 - l)) - t.first[l];
        if (k >= 0 && k < t.counts[l]) {
            *len = l;
            return t.values[(t.index[l] + k) & 255];
        }
    }
    return -1;
}

// `bits` of the window behind `skip`, extended to a signed value (T.81 F.2.2.1).  1 <= bits <= 15, skip + bits <= 31
__device__ __forceinline__ int jh_receive(uint32_t win, int skip, int bits) {
    const int v = (int)((win << skip) >> (32 - bits));
    return v >= (1 << (bits - 1)) ? v : v - (1 << bits) + 1;
}

// Where the block with this ordinal in the segment goes: 64 b, b the component-major, row-major index; -1 for a block that is dropped.
__device__ __forceinline__ long jh_block_base(const JhSegment& s, uint32_t ordinal, int slot) {
    if (ordinal >= s.expected) return -1;
    const uint32_t mcu = s.first_mcu + ordinal / (uint32_t)s.nslots;
    const uint32_t my = mcu / (uint32_t)s.mcus_x, mx = mcu - my * (uint32_t)s.mcus_x;
    uint32_t b;
    if (slot < s.hv) {
        const uint32_t j = (uint32_t)slot / (uint32_t)s.h, i = (uint32_t)slot - j * (uint32_t)s.h;
        b = (my * (uint32_t)s.v + j) * ((uint32_t)s.mcus_x * (uint32_t)s.h) + mx * (uint32_t)s.h + i;
    } else {
        b = s.n0 + (uint32_t)(slot - s.hv) * s.nc + my * (uint32_t)s.mcus_x + mx;
    }
    return b < s.total_blocks ? (long)b * 64 : -1;
}

// MODE 3: the same for an image that consists of the MCU rows band_row0 .. band_row0 + band_rows) alone; -1 for a block of another row.
__device__ __forceinline__ long jh_band_base(const JhSegment& s, uint32_t ordinal, int slot) {
    if (ordinal >= s.expected) return -1;
    const uint32_t mcu = s.first_mcu + ordinal / (uint32_t)s.nslots;
    const uint32_t my = mcu / (uint32_t)s.mcus_x, mx = mcu - my * (uint32_t)s.mcus_x;
    if (my < s.band_row0 || my >= s.band_row0 + s.band_rows) return -1;   // band_row0 + band_rows <= mcus_y <= 1024
    const uint32_t ry = my - s.band_row0, band_mcus = s.band_rows * (uint32_t)s.mcus_x;
    uint32_t b;
    if (slot < s.hv) {
        const uint32_t j = (uint32_t)slot / (uint32_t)s.h, i = (uint32_t)slot - j * (uint32_t)s.h;
        b = (ry * (uint32_t)s.v + j) * ((uint32_t)s.mcus_x * (uint32_t)s.h) + mx * (uint32_t)s.h + i;
    } else {
        b = band_mcus * (uint32_t)s.hv + (uint32_t)(slot - s.hv) * band_mcus + ry * (uint32_t)s.mcus_x + mx;
    }
    return b < band_mcus * (uint32_t)s.nslots ? (long)b * 64 : -1;
}

// MODE 4: the block's place in the WHOLE image (jh_block_base), but -1 for a block whose MCU row lies outside the band.
__device__ __forceinline__ long jh_rows_base(const JhSegment& s, uint32_t ordinal, int slot) {
    if (ordinal >= s.expected) return -1;
    const uint32_t my = (s.first_mcu + ordinal / (uint32_t)s.nslots) / (uint32_t)s.mcus_x;
    if (my < s.band_row0 || my >= s.band_row0 + s.band_rows) return -1;   // band_row0 + band_rows <= mcus_y <= 1024
    return jh_block_base(s, ordinal, slot);
}

// MODE 5: the block's place in an image that consists of the MCUs of the band's rows and the columns win_col0 .. win_col0 + win_cols)
// alone (window-dense); -1 for a block of another row or column.
__device__ __forceinline__ long jh_window_base(const JhSegment& s, uint32_t ordinal, int slot) {
    if (ordinal >= s.expected) return -1;
    const uint32_t mcu = s.first_mcu + ordinal / (uint32_t)s.nslots;
    const uint32_t my = mcu / (uint32_t)s.mcus_x, mx = mcu - my * (uint32_t)s.mcus_x;
    if (my < s.band_row0 || my >= s.band_row0 + s.band_rows) return -1;   // band_row0 + band_rows <= mcus_y <= 1024
    if (mx < s.win_col0 || mx >= s.win_col0 + s.win_cols) return -1;      // win_col0 + win_cols <= mcus_x <= 1024
    const uint32_t ry = my - s.band_row0, rx = mx - s.win_col0, win_mcus = s.band_rows * s.win_cols;
    uint32_t b;
    if (slot < s.hv) {
        const uint32_t j = (uint32_t)slot / (uint32_t)s.h, i = (uint32_t)slot - j * (uint32_t)s.h;
        b = (ry * (uint32_t)s.v + j) * (s.win_cols * (uint32_t)s.h) + rx * (uint32_t)s.h + i;
    } else {
        b = win_mcus * (uint32_t)s.hv + (uint32_t)(slot - s.hv) * win_mcus + ry * s.win_cols + rx;
    }
    return b < win_mcus * (uint32_t)s.nslots ? (long)b * 64 : -1;
}

template <int MODE>
__device__ __forceinline__ long jh_base(const JhSegment& s, uint32_t ordinal, int slot) {
    return MODE == 5 ? jh_window_base(s, ordinal, slot)
                     : (MODE == 4 ? jh_rows_base(s, ordinal, slot) : (MODE == 3 ? jh_band_base(s, ordinal, slot) : jh_block_base(s, ordinal, slot)));
}

// What the count pass gathers and the write pass starts from.
struct JhLane {
    uint32_t begun;          // blocks begun: in this subsequence (count) | in the segment so far (write)
    uint32_t dc0, dc1, dc2;  // DC differences summed (count) | the predictors (write), modulo 2^16, by component
    bool error;
};

// dc[comp] += v modulo 2^16, without indexing the registers by a run-time value.
__device__ __forceinline__ uint32_t jh_add_dc(JhLane& lane, int comp, uint32_t v) {
    const uint32_t d0 = lane.dc0, d1 = lane.dc1, d2 = lane.dc2;
    const uint32_t sum = ((comp == 0 ? d0 : (comp == 1 ? d1 : d2)) + v) & 0xFFFFu;
    lane.dc0 = comp == 0 ? sum : d0;
    lane.dc1 = comp == 1 ? sum : d1;
    lane.dc2 = comp == 2 ? sum : d2;
    return sum;
}

// Symbols from `st` until the position reaches `end` or the segment's end.  MODE 0: the exit state and nothing else.  1: count.  2: write.
// 3: write, but only the blocks of the band's MCU rows are stored (jh_band_base); every judgement is mode 2's.
// 4: write, only the blocks of the band's MCU rows, at their place in the whole image (jh_rows_base); every judgement is mode 2's.
// 5: write, only the blocks of the window's MCU rows and columns, window-dense (jh_window_base); every judgement is mode 2's.
// A code in no table, a DC size above 15 or an index past 63: advance one bit, z = 0.  STAGED: jh_word's fetch policy.
template <int MODE, bool STAGED = false>
__device__ __forceinline__ JhState jh_decode(const JhSegment& s, const FearJpegHuff* tabs, JhState st, uint32_t end, int16_t* coef, JhLane& io) {
    JhLane lane = io;
    uint32_t p = st.p;
    int slot = (int)(st.sz >> 8), z = (int)(st.sz & 255);
    const uint32_t stop = min(end, s.bits);
    long base = -1;                                                      // MODE 2, 3: the open block's place, -1 if it is dropped
    bool judged = false;                                                 // MODE 2, 3: the open block, or the next one, is one the segment owes
    if (MODE >= 2) {
        if (z != 0 && lane.begun > 0) base = jh_base<MODE>(s, lane.begun - 1, slot);
        judged = (z != 0 ? lane.begun - 1 : lane.begun) < s.expected && (z == 0 || lane.begun > 0);
    }
#pragma unroll 1
    for (uint32_t step = 0; step < end - st.p + 32 && p < stop; ++step) {   // a symbol is at least one bit: the count never binds
        const uint32_t win = jh_peek<STAGED>(s, p);
        const int comp = slot < s.hv ? 0 : slot - s.hv + 1;
        int len = 0;
        if (z == 0) {
            const int t = jh_symbol(tabs[comp], win, &len);
            if (t < 0 || t > 15) {
                if (MODE >= 2 && judged) lane.error = true;
                p += 1;
                continue;
            }
            const int diff = t ? jh_receive(win, len, t) : 0;
            p += (uint32_t)(len + t);
            z = 1;
            if (MODE == 1) {
                lane.begun += 1;
                jh_add_dc(lane, comp, (uint32_t)diff);
            }
            if (MODE >= 2) {
                const uint32_t dc = jh_add_dc(lane, comp, (uint32_t)diff);      // the predictor; JCOEF is 16 bits wide
                base = jh_base<MODE>(s, lane.begun, slot);
                judged = lane.begun < s.expected;
                lane.begun += 1;
                if (judged && p > s.bits) lane.error = true;              // the code or its magnitude bits run past the segment
                if (base >= 0) coef[base] = (int16_t)(uint16_t)dc;
            }
            continue;
        }
        const int rs = jh_symbol(tabs[3 + comp], win, &len);
        const int r = rs >> 4, size = rs & 15;
        if (rs < 0 || z + r > (size ? 63 : (r == 15 ? 62 : 99))) {        // an index past 63, a ZRL that runs past it included
            if (MODE >= 2 && judged) lane.error = true;
            p += 1;
            z = 0;
            if (MODE >= 2) { base = -1; judged = lane.begun < s.expected; }
            continue;
        }
        int zeros_to, value = 0;
        if (size == 0) {
            p += (uint32_t)len;
            zeros_to = r == 15 ? z + 16 : 64;                            // ZRL | EOB
        } else {
            value = jh_receive(win, len, size);
            p += (uint32_t)(len + size);
            zeros_to = z + r;
        }
        if (MODE >= 2) {
            if (judged && p > s.bits) lane.error = true;
            if (base >= 0) {
#pragma unroll 1
                for (int k = z; k < zeros_to; ++k) coef[base + k] = 0;    // zeros_to <= 64
                if (size) coef[base + zeros_to] = (int16_t)value;        // zeros_to <= 63
            }
        }
        z = size ? zeros_to + 1 : zeros_to;
        if (z == 64) {
            z = 0;
            slot = slot + 1 < s.nslots ? slot + 1 : 0;
            if (MODE >= 2) {
                // the segment's last block is complete: in front of a restart marker no whole byte may be left (Bits::restart)
                if (lane.begun == s.expected && judged && !s.last && p <= s.bits && s.bits - p >= 8) lane.error = true;
                base = -1;
                judged = lane.begun < s.expected;
            }
        }
    }
    if (MODE != 0) io = lane;
    JhState out;
    out.p = p;
    out.sz = (uint32_t)slot << 8 | (uint32_t)z;
    return out;
}

// The entry of subsequence `sub` of segment `seg`: the state and the lane with which its write pass starts, one 16-byte store, checked
// against the index's capacity.
__device__ __forceinline__ void jh_store_entry(const FearJpegIndex& ix, uint32_t seg, uint32_t sub, JhState entry, const JhLane& lane) {
    const uint64_t at = (uint64_t)ix.sub_start[seg] + sub;
    if (at >= ix.n_sub) return;
    uint4 e;
    e.x = entry.p;
    e.y = lane.begun;
    e.z = (entry.sz & 0xFFFFu) | lane.dc0 << 16;
    e.w = (lane.dc1 & 0xFFFFu) | lane.dc2 << 16;
    reinterpret_cast<uint4*>(ix.index)[at] = e;
}

__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_status_kernel(int32_t* status, int n) {
    const int i = blockIdx.x * kJhLanes + threadIdx.x;
    if (i < n) status[i] = FEAR_TRAIN_OK;
}

__global__ __launch_bounds__(kJhLanes) void jpeg_dense_block_start_kernel(uint32_t* block_start, uint32_t total_blocks) {
    const uint32_t i = blockIdx.x * (uint32_t)kJhLanes + threadIdx.x;
    if (i <= total_blocks) block_start[i] = i * 64u;
}

// INDEX: fear_jpeg_index_build's instantiation, which also stores every lane's entry in front of its write pass (fear_jpeg_store.h).
template <bool INDEX>
__global__ __launch_bounds__(kJhLanes) void jpeg_huffman_kernel(JpegHuffArgs a) {
    __shared__ __attribute__((aligned(16))) FearJpegHuff tabs[6];        // dc by component, then ac by component
    __shared__ uint32_t st_p[kJhLanes], st_sz[kJhLanes];                 // the exit state of each subsequence of the sequence
    __shared__ uint32_t scan[2][4][kJhLanes];                            // the prefix over blocks begun and the three DC sums
    __shared__ int failed;
    const int tid = threadIdx.x;
    const int img = jd_find_image(a.table, a.n, blockIdx.x);
    const FearJpegScan* rec =
        reinterpret_cast<const FearJpegScan*>(reinterpret_cast<const char*>(a.table) + FEAR_JPEG_SCAN_TABLE_RECORDS(a.n)) + img;
    const uint32_t seg = blockIdx.x - a.table[img];
    if (seg >= rec->n_seg) return;                                       // the same for the whole workgroup
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(rec->dc);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
        for (int i = tid; i < (int)(sizeof(tabs) / 4); i += kJhLanes) dst[i] = src[i];
        if (tid == 0) failed = 0;
    }
    JhSegment s;
    {
        const uint32_t n_bytes = rec->n_bytes;
        const uint32_t b0 = min(rec->seg_start[seg], n_bytes), b1 = min(max(rec->seg_start[seg + 1], b0), n_bytes);
        s.words = reinterpret_cast<const uint32_t*>(rec->bytes);
        s.n_words = (n_bytes + 3) >> 2;
        s.byte0 = b0;
        s.bits = min(b1 - b0, FEAR_JPEG_DEVICE_SCAN_MAX) * 8u;
        const int nf = rec->components;
        s.h = rec->h;
        s.v = rec->v;
        s.hv = nf == 3 ? s.h * s.v : 1;
        s.nslots = nf == 3 ? s.hv + 2 : 1;
        s.mcus_x = rec->mcus_x;
        const uint32_t n_mcu = (uint32_t)rec->mcus_x * (uint32_t)rec->mcus_y;
        s.n0 = n_mcu * (uint32_t)s.hv;
        s.nc = n_mcu;
        s.total_blocks = rec->total_blocks;
        const uint32_t interval = rec->restart_interval ? (uint32_t)rec->restart_interval : n_mcu;
        const uint64_t first = (uint64_t)seg * interval;
        s.first_mcu = first < n_mcu ? (uint32_t)first : n_mcu;
        s.expected = min(interval, n_mcu - s.first_mcu) * (uint32_t)s.nslots;
        s.last = seg + 1 == rec->n_seg;
    }
    int16_t* coef = a.coef + rec->coef_offset;
    const uint32_t SB = (uint32_t)a.subsequence_bits;
    const uint32_t n_sub = (s.bits + SB - 1) / SB, n_seq = (n_sub + kJhLanes - 1) / kJhLanes;
    JhState carry{0u, 0u};
    uint32_t begun = 0, pred[3] = {0u, 0u, 0u};
    JhLane lane{};
    __syncthreads();
#pragma unroll 1
    for (uint32_t q = 0; q < n_seq; ++q) {
        const int m = (int)min((uint32_t)kJhLanes, n_sub - q * kJhLanes);     // the lanes with a subsequence inside the segment
        const uint32_t sub = q * kJhLanes + tid;
        const bool on = tid < m;
        // synchronise
        JhState mine{sub * SB, 0u};
        if (tid == 0) mine = carry;
        bool active = on;
        if (on) {
            mine = jh_decode<0>(s, tabs, mine, (sub + 1) * SB, coef, lane);
            st_p[tid] = mine.p;
            st_sz[tid] = mine.sz;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 1; r < kJhLanes; ++r) {
            const int j = tid + r;                                      // in round r only lane j - r touches entry j
            if (active && j < m) {
                const JhState out = jh_decode<0>(s, tabs, mine, (sub + r + 1) * SB, coef, lane);
                if (out.p == st_p[j] && out.sz == st_sz[j]) {
                    active = false;                                     // synchronised: the chain from here on is already stored
                } else {
                    st_p[j] = out.p;
                    st_sz[j] = out.sz;
                    mine = out;
                }
            } else {
                active = false;
            }
            if (!__syncthreads_or(active)) break;
        }
        JhState entry = carry;
        if (on && tid > 0) { entry.p = st_p[tid - 1]; entry.sz = st_sz[tid - 1]; }
        // count, and the exclusive prefix over the lanes
        lane.begun = 0;
        lane.dc0 = lane.dc1 = lane.dc2 = 0;
        if (on) jh_decode<1>(s, tabs, entry, (sub + 1) * SB, coef, lane);
        const uint32_t own[4] = {lane.begun, lane.dc0, lane.dc1, lane.dc2};
#pragma unroll
        for (int k = 0; k < 4; ++k) scan[0][k][tid] = own[k];
        __syncthreads();
        int cur = 0;
#pragma unroll 1
        for (int d = 1; d < kJhLanes; d <<= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) scan[cur ^ 1][k][tid] = scan[cur][k][tid] + (tid >= d ? scan[cur][k][tid - d] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        uint32_t total[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) total[k] = scan[cur][k][kJhLanes - 1];
        // write
        lane.begun = begun + scan[cur][0][tid] - own[0];
        lane.dc0 = (pred[0] + scan[cur][1][tid] - own[1]) & 0xFFFFu;
        lane.dc1 = (pred[1] + scan[cur][2][tid] - own[2]) & 0xFFFFu;
        lane.dc2 = (pred[2] + scan[cur][3][tid] - own[3]) & 0xFFFFu;
        if (INDEX && on) jh_store_entry(a.indexes[img], seg, sub, entry, lane);
        if (on) jh_decode<2>(s, tabs, entry, (sub + 1) * SB, coef, lane);
        begun += total[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) pred[k] = (pred[k] + total[1 + k]) & 0xFFFFu;
        carry.p = st_p[m - 1];
        carry.sz = st_sz[m - 1];
        __syncthreads();                                                // the next sequence overwrites the states and the prefix
    }
    if (lane.error) failed = 1;                                          // every lane that stores stores the same value
    __syncthreads();
    // fewer complete blocks than the segment owes: the true chain's last block is open, or was never begun
    if (tid == 0 && (failed || begun - ((carry.sz & 255) != 0 ? 1u : 0u) < s.expected || (begun == 0 && s.expected > 0)))
        a.status[img] = FEAR_TRAIN_ERR_FORMAT;
}

bool jh_scan_ok(const FearJpegScan& sc) {
    if (!jd_mode_ok(sc.components, sc.h, sc.v)) return false;
    if (sc.mcus_x < 1 || sc.mcus_x > FEAR_JPEG_MAX_SIDE / 8 || sc.mcus_y < 1 || sc.mcus_y > FEAR_JPEG_MAX_SIDE / 8) return false;
    if (sc.restart_interval < 0 || sc.restart_interval > 65535) return false;
    const uint32_t n_mcu = (uint32_t)sc.mcus_x * (uint32_t)sc.mcus_y;
    const uint32_t per_mcu = sc.components == 3 ? (uint32_t)(sc.h * sc.v + 2) : 1u;
    const uint32_t n_seg = sc.restart_interval ? (n_mcu + (uint32_t)sc.restart_interval - 1) / (uint32_t)sc.restart_interval : 1u;
    if (sc.total_blocks != n_mcu * per_mcu || sc.n_seg != n_seg) return false;
    if ((reinterpret_cast<uintptr_t>(sc.bytes) & 3) != 0 || (reinterpret_cast<uintptr_t>(sc.seg_start) & 3) != 0) return false;
    return sc.max_seg_bytes <= FEAR_JPEG_DEVICE_SCAN_MAX && sc.max_seg_bytes <= sc.n_bytes;
}

}  // namespace

extern "C" {

int fear_jpeg_huffman(const FearJpegScan* scans, int n, const void* table_dev, int16_t* coef, int32_t* status_dev, int subsequence_bytes,
                      void* stream) {
    if (n < 0 || n > 65535 || subsequence_bytes < 4 || subsequence_bytes > 1024 || (subsequence_bytes & 3) != 0) return FEAR_TRAIN_ERR_SHAPE;
    if (n == 0) return FEAR_TRAIN_OK;
    if (!scans || !table_dev || !coef || !status_dev) return FEAR_TRAIN_ERR_NULL;
    uint64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        if (!scans[i].bytes || !scans[i].seg_start) return FEAR_TRAIN_ERR_NULL;
        if (!jh_scan_ok(scans[i])) return FEAR_TRAIN_ERR_SHAPE;
        groups += scans[i].n_seg;
    }
    if (groups > 0x7fffffffu) return FEAR_TRAIN_ERR_SHAPE;
    JpegHuffArgs a{};
    a.table = static_cast<const uint32_t*>(table_dev);
    a.coef = coef;
    a.status = status_dev;
    a.n = n;
    a.subsequence_bits = subsequence_bytes * 8;
    hipLaunchKernelGGL(jpeg_huffman_status_kernel, dim3((unsigned)((n + kJhLanes - 1) / kJhLanes)), dim3(kJhLanes), 0,
                       static_cast<hipStream_t>(stream), status_dev, n);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_huffman_kernel<false>, dim3((unsigned)groups), dim3(kJhLanes), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

int fear_jpeg_dense_block_start(uint32_t* block_start, uint32_t total_blocks, void* stream) {
    if (!block_start) return FEAR_TRAIN_ERR_NULL;
    if (total_blocks > 3u * (FEAR_JPEG_MAX_SIDE / 8) * (FEAR_JPEG_MAX_SIDE / 8)) return FEAR_TRAIN_ERR_SHAPE;
    hipLaunchKernelGGL(jpeg_dense_block_start_kernel, dim3((total_blocks + 1 + kJhLanes - 1) / kJhLanes), dim3(kJhLanes), 0,
                       static_cast<hipStream_t>(stream), block_start, total_blocks);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
