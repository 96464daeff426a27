// jpeg_entropy_host.cpp — the host half of the JPEG frame decoder (feartracker_amd/csrc/fear_jpeg_entropy.h) as a stand-alone program, so
// that it can run under the address and undefined-behaviour sanitizers without Python or a GPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o jpeg_entropy_host tools/jpeg_entropy_host.cpp
//     ./jpeg_entropy_host FILE...
//
// Per file one line: name, status of fear_jpeg_parse, status of fear_jpeg_entropy_decode, width, height, components, total_blocks, values
// stored, FNV-1a of block_start and the packed coefficients.  Every buffer is allocated at exactly the size the call is told, a second call
// gets exactly the values the first one used, and a third one value less (it must return FEAR_TRAIN_ERR_WORKSPACE).
// A file whose headers parse gets a second line for fear_jpeg_scan_prepare: name, "scan", its status, and where it accepts the bytes, the
// segments and FNV-1a of seg_start and the unstuffed bytes — the first call with the file's length and segments + 1 as capacities, a
// second with exactly the bytes the first one wrote, a third with one byte less (FEAR_TRAIN_ERR_WORKSPACE).
// A file whose scan is accepted gets a third line for fear_jpeg_sub_start: name, "sub", and per subsequence length 4 and 128 the status, n_sub
// and FNV-1a of sub_start — seg_start in an exact-size heap copy, sub_start at exactly n_seg + 1 entries; a count-only call must give the
// same n_sub, a capacity one entry short FEAR_TRAIN_ERR_WORKSPACE, offsets that do not end at n_bytes FEAR_TRAIN_ERR_SHAPE.
// tools/jpeg_entropy_check.py writes the files, runs the program and compares each line with the Python decoder's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../feartracker_amd/csrc/fear_jpeg_entropy.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static int sub_line(const char* name, const uint32_t* seg_start, const FearJpegScan& scan) {
    int failures = 0;
    const size_t entries = (size_t)scan.n_seg + 1;
    uint32_t* seg = static_cast<uint32_t*>(std::malloc(entries * sizeof(uint32_t)));
    uint32_t* sub = static_cast<uint32_t*>(std::malloc(entries * sizeof(uint32_t)));
    std::memcpy(seg, seg_start, entries * sizeof(uint32_t));
    std::printf("%s sub", name);
    for (int bytes : {4, 128}) {
        uint32_t n_sub = 0, counted = 0;
        const int rc = fear_jpeg_sub_start(seg, scan.n_seg, scan.n_bytes, bytes, sub, entries, &n_sub);
        std::printf(" %d %u %016llx", rc, n_sub, (unsigned long long)fnv(14695981039346656037ull, sub, entries * sizeof(uint32_t)));
        if (fear_jpeg_sub_start(seg, scan.n_seg, scan.n_bytes, bytes, nullptr, 0, &counted) != rc || counted != n_sub ||
            fear_jpeg_sub_start(seg, scan.n_seg, scan.n_bytes, bytes, sub, entries - 1, &counted) != FEAR_TRAIN_ERR_WORKSPACE ||
            fear_jpeg_sub_start(seg, scan.n_seg, scan.n_bytes + 1, bytes, sub, entries, &counted) != FEAR_TRAIN_ERR_SHAPE) {
            std::printf("\n%s: fear_jpeg_sub_start at %d bytes: the count-only call, a short capacity or foreign offsets\n", name, bytes);
            ++failures;
        }
    }
    std::printf("\n");
    std::free(sub);
    std::free(seg);
    return failures;
}

static int scan_line(const char* name, const unsigned char* data, size_t n, const FearJpegInfo& info) {
    int failures = 0;
    const size_t n_mcu = (size_t)info.mcus_x * (size_t)info.mcus_y;
    const size_t seg_cap = (info.restart_interval ? (n_mcu + info.restart_interval - 1) / info.restart_interval : 1) + 1;
    unsigned char* bytes = static_cast<unsigned char*>(std::malloc(n ? n : 1));
    uint32_t* seg = static_cast<uint32_t*>(std::malloc(seg_cap * sizeof(uint32_t)));
    FearJpegScan* scan = static_cast<FearJpegScan*>(std::malloc(sizeof(FearJpegScan)));
    const int rc = fear_jpeg_scan_prepare(data, n, &info, bytes, n, seg, seg_cap, scan);
    if (rc != FEAR_TRAIN_OK) {
        std::printf("%s scan %d\n", name, rc);
    } else {
        uint64_t h = fnv(14695981039346656037ull, seg, ((size_t)scan->n_seg + 1) * sizeof(uint32_t));
        h = fnv(h, bytes, scan->n_bytes);
        std::printf("%s scan %d %u %u %016llx\n", name, rc, scan->n_bytes, scan->n_seg, (unsigned long long)h);
        const size_t used = scan->n_bytes;
        unsigned char* exact = static_cast<unsigned char*>(std::malloc(used ? used : 1));
        FearJpegScan* again = static_cast<FearJpegScan*>(std::malloc(sizeof(FearJpegScan)));
        if (fear_jpeg_scan_prepare(data, n, &info, exact, used, seg, seg_cap, again) != FEAR_TRAIN_OK || again->n_bytes != used ||
            std::memcmp(exact, bytes, used) != 0 || std::memcmp(again, scan, sizeof(FearJpegScan)) != 0) {
            std::printf("%s: the scan at the exact capacity differs\n", name);
            ++failures;
        }
        if (used > 0 && fear_jpeg_scan_prepare(data, n, &info, exact, used - 1, seg, seg_cap, again) != FEAR_TRAIN_ERR_WORKSPACE) {
            std::printf("%s: a scan capacity one byte short was not refused\n", name);
            ++failures;
        }
        if (fear_jpeg_scan_prepare(data, n, &info, exact, used, seg, seg_cap - 1, again) != FEAR_TRAIN_ERR_WORKSPACE) {
            std::printf("%s: a segment capacity one entry short was not refused\n", name);
            ++failures;
        }
        std::free(again);
        std::free(exact);
        failures += sub_line(name, seg, *scan);
    }
    std::free(scan);
    std::free(seg);
    std::free(bytes);
    return failures;
}

int main(int argc, char** argv) {
    int failures = 0;
    for (int f = 1; f < argc; ++f) {
        FILE* fp = std::fopen(argv[f], "rb");
        if (!fp) { std::printf("%s unreadable\n", argv[f]); ++failures; continue; }
        std::fseek(fp, 0, SEEK_END);
        const long size = std::ftell(fp);
        std::fseek(fp, 0, SEEK_SET);
        // an exact-size heap copy: a read past the end is the sanitizer's to report
        unsigned char* data = static_cast<unsigned char*>(std::malloc(size > 0 ? (size_t)size : 1));
        const size_t n = std::fread(data, 1, (size_t)size, fp);
        std::fclose(fp);
        const char* name = std::strrchr(argv[f], '/');
        name = name ? name + 1 : argv[f];
        FearJpegInfo info;
        const int rc = fear_jpeg_parse(data, n, &info);
        if (rc != FEAR_TRAIN_OK) {
            std::printf("%s %d\n", name, rc);
            std::free(data);
            continue;
        }
        failures += scan_line(name, data, n, info);
        const size_t cap = fear_jpeg_packed_bound(&info);
        int16_t* coef = static_cast<int16_t*>(std::malloc(cap * sizeof(int16_t)));
        uint32_t* start = static_cast<uint32_t*>(std::malloc(((size_t)info.total_blocks + 1) * sizeof(uint32_t)));
        size_t used = 0;
        const int rd = fear_jpeg_entropy_decode(data, n, &info, coef, cap, start, &used);
        if (rd != FEAR_TRAIN_OK) {
            std::printf("%s %d %d\n", name, rc, rd);
        } else {
            uint64_t h = fnv(14695981039346656037ull, start, ((size_t)info.total_blocks + 1) * sizeof(uint32_t));
            h = fnv(h, coef, used * sizeof(int16_t));
            std::printf("%s %d %d %d %d %d %u %zu %016llx\n", name, rc, rd, info.width, info.height, info.components, info.total_blocks, used,
                        (unsigned long long)h);
            int16_t* exact = static_cast<int16_t*>(std::malloc(used * sizeof(int16_t)));
            size_t again = 0;
            if (fear_jpeg_entropy_decode(data, n, &info, exact, used, start, &again) != FEAR_TRAIN_OK || again != used ||
                std::memcmp(exact, coef, used * sizeof(int16_t)) != 0) {
                std::printf("%s: the call at the exact capacity differs\n", name);
                ++failures;
            }
            if (fear_jpeg_entropy_decode(data, n, &info, exact, used - 1, start, &again) != FEAR_TRAIN_ERR_WORKSPACE) {
                std::printf("%s: a capacity one value short was not refused\n", name);
                ++failures;
            }
            std::free(exact);
        }
        std::free(coef);
        std::free(start);
        std::free(data);
    }
    return failures ? 1 : 0;
}
