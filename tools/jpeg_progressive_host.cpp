// jpeg_progressive_host.cpp — the progressive decoder and transcoder (feartracker_amd/csrc/fear_jpeg_progressive.h) as a stand-alone
// program, so that they can run under the address and undefined-behaviour sanitizers without Python or a GPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o jpeg_progressive_host tools/jpeg_progressive_host.cpp
//     ./jpeg_progressive_host [--hostile N] FILE...
//
// Per file one line: name, the statuses of fear_jpeg_progressive_parse, fear_jpeg_progressive_decode and
// fear_jpeg_progressive_to_baseline, and where they accept width, height, components, total_blocks, the values stored, the transcode's
// length, FNV-1a of block_start with the packed coefficients and FNV-1a of the transcode.  Every buffer is allocated at exactly the size the
// call is told; a second call of each gets exactly what the first one used and a third one unit less (FEAR_TRAIN_ERR_WORKSPACE); the
// decode and the transcode must give one verdict; the transcode must pass fear_jpeg_parse and fear_jpeg_entropy_decode and give the same
// packed coefficients.  The first N files (--hostile N, by default none) are also run, without a line, at every prefix and with every
// single byte flipped: the three entry points on an exact-size heap copy, the two verdicts compared.
// The files are the cases of tests/golden/jpeg_progressive.npz, written out with their sizes in front so that a shell glob lists the
// smallest first:
//
//     python -c "import numpy as np; d = np.load('tests/golden/jpeg_progressive.npz'); \
//       [open('DIR/%06d_%s.jpg' % (d['jpg_%d' % i].size, n), 'wb').write(d['jpg_%d' % i].tobytes()) for i, n in enumerate(d['names'])]"
//     ./jpeg_progressive_host --hostile 2 DIR/*.jpg
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../feartracker_amd/csrc/fear_jpeg_progressive.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

struct Result {
    int parse, decode, transcode;
    FearJpegInfo info;
    size_t used, length;
    uint64_t h_coef, h_file;
};

// The three entry points on an exact-size heap copy of `src`; returns the number of broken promises.
static int run(const char* name, const unsigned char* src, size_t n, Result* r) {
    int failures = 0;
    unsigned char* data = static_cast<unsigned char*>(std::malloc(n ? n : 1));
    std::memcpy(data, src, n);
    std::memset(r, 0, sizeof(*r));
    r->parse = fear_jpeg_progressive_parse(data, n, &r->info);
    // the transcode does not need the header: a fixed, modest capacity where there is none
    const size_t out_cap = r->parse == FEAR_TRAIN_OK ? fear_jpeg_baseline_bound(&r->info) : 4096;
    unsigned char* out = static_cast<unsigned char*>(std::malloc(out_cap));
    r->transcode = fear_jpeg_progressive_to_baseline(data, n, out, out_cap, &r->length);
    if (r->parse != FEAR_TRAIN_OK) {
        r->decode = r->parse;
        if (r->transcode == FEAR_TRAIN_OK) { std::printf("%s: a transcode of a file whose headers are declined\n", name); ++failures; }
        std::free(out);
        std::free(data);
        return failures;
    }
    const size_t cap = fear_jpeg_packed_bound(&r->info), entries = (size_t)r->info.total_blocks + 1;
    int16_t* coef = static_cast<int16_t*>(std::malloc(cap * sizeof(int16_t)));
    uint32_t* start = static_cast<uint32_t*>(std::malloc(entries * sizeof(uint32_t)));
    r->decode = fear_jpeg_progressive_decode(data, n, &r->info, coef, cap, start, &r->used);
    if (r->decode != r->transcode) { std::printf("%s: the decode says %d, the transcode %d\n", name, r->decode, r->transcode); ++failures; }
    if (r->decode == FEAR_TRAIN_OK && r->transcode == FEAR_TRAIN_OK) {
        r->h_coef = fnv(fnv(14695981039346656037ull, start, entries * sizeof(uint32_t)), coef, r->used * sizeof(int16_t));
        r->h_file = fnv(14695981039346656037ull, out, r->length);
        // exact capacities, and one unit less
        int16_t* exact = static_cast<int16_t*>(std::malloc(r->used * sizeof(int16_t)));
        uint32_t* start2 = static_cast<uint32_t*>(std::malloc(entries * sizeof(uint32_t)));
        size_t again = 0;
        if (fear_jpeg_progressive_decode(data, n, &r->info, exact, r->used, start2, &again) != FEAR_TRAIN_OK || again != r->used ||
            std::memcmp(exact, coef, r->used * sizeof(int16_t)) != 0 || std::memcmp(start, start2, entries * sizeof(uint32_t)) != 0) {
            std::printf("%s: the decode at the exact capacity differs\n", name);
            ++failures;
        }
        if (fear_jpeg_progressive_decode(data, n, &r->info, exact, r->used - 1, start2, &again) != FEAR_TRAIN_ERR_WORKSPACE) {
            std::printf("%s: a coefficient capacity one value short was not refused\n", name);
            ++failures;
        }
        unsigned char* tight = static_cast<unsigned char*>(std::malloc(r->length));
        if (fear_jpeg_progressive_to_baseline(data, n, tight, r->length, &again) != FEAR_TRAIN_OK || again != r->length ||
            std::memcmp(tight, out, r->length) != 0) {
            std::printf("%s: the transcode at the exact capacity differs\n", name);
            ++failures;
        }
        if (fear_jpeg_progressive_to_baseline(data, n, tight, r->length - 1, &again) != FEAR_TRAIN_ERR_WORKSPACE) {
            std::printf("%s: a transcode capacity one byte short was not refused\n", name);
            ++failures;
        }
        // the transcode through the baseline decoder: the same packed stream
        FearJpegInfo base;
        size_t used2 = 0;
        int rc = fear_jpeg_parse(tight, r->length, &base);
        if (rc == FEAR_TRAIN_OK && base.restart_interval == base.mcus_x) {
            base.restart_interval = 0;
            if (std::memcmp(&base, &r->info, sizeof(base)) != 0) rc = FEAR_TRAIN_ERR_SHAPE;
            base.restart_interval = base.mcus_x;
        } else if (rc == FEAR_TRAIN_OK) {
            rc = FEAR_TRAIN_ERR_SHAPE;
        }
        if (rc == FEAR_TRAIN_OK) rc = fear_jpeg_entropy_decode(tight, r->length, &base, exact, r->used, start2, &used2);
        if (rc != FEAR_TRAIN_OK || used2 != r->used || std::memcmp(exact, coef, r->used * sizeof(int16_t)) != 0 ||
            std::memcmp(start, start2, entries * sizeof(uint32_t)) != 0) {
            std::printf("%s: the baseline decoder does not read the transcode as the same coefficients (status %d)\n", name, rc);
            ++failures;
        }
        std::free(tight);
        std::free(start2);
        std::free(exact);
    }
    std::free(start);
    std::free(coef);
    std::free(out);
    std::free(data);
    return failures;
}

int main(int argc, char** argv) {
    int failures = 0, hostile = 0, first = 1;
    if (argc > 2 && std::strcmp(argv[1], "--hostile") == 0) { hostile = std::atoi(argv[2]); first = 3; }
    long variants = 0, accepted = 0;
    for (int f = first; f < argc; ++f) {
        FILE* fp = std::fopen(argv[f], "rb");
        if (!fp) { std::printf("%s unreadable\n", argv[f]); ++failures; continue; }
        std::fseek(fp, 0, SEEK_END);
        const long size = std::ftell(fp);
        std::fseek(fp, 0, SEEK_SET);
        unsigned char* data = static_cast<unsigned char*>(std::malloc(size > 0 ? (size_t)size : 1));
        const size_t n = std::fread(data, 1, (size_t)size, fp);
        std::fclose(fp);
        const char* name = std::strrchr(argv[f], '/');
        name = name ? name + 1 : argv[f];
        Result r;
        failures += run(name, data, n, &r);
        if (r.decode != FEAR_TRAIN_OK)
            std::printf("%s %d %d %d\n", name, r.parse, r.decode, r.transcode);
        else
            std::printf("%s %d %d %d %d %d %d %u %zu %zu %016llx %016llx\n", name, r.parse, r.decode, r.transcode, r.info.width, r.info.height,
                        r.info.components, r.info.total_blocks, r.used, r.length, (unsigned long long)r.h_coef, (unsigned long long)r.h_file);
        if (f - first < hostile) {
            Result v;
            for (size_t k = 0; k < n; ++k) {
                failures += run(name, data, k, &v);                       // every prefix
                accepted += v.decode == FEAR_TRAIN_OK;
                data[k] ^= 0xFF;                                          // every flipped byte
                failures += run(name, data, n, &v);
                accepted += v.decode == FEAR_TRAIN_OK;
                data[k] ^= 0xFF;
                variants += 2;
            }
        }
        std::free(data);
    }
    if (hostile) std::printf("hostile: %ld variants, %ld accepted\n", variants, accepted);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
