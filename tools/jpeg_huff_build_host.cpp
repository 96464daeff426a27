// jpeg_huff_build_host.cpp — the Huffman table builder of the JPEG encoder (feartracker_amd/csrc/fear_jpeg_huff_build.h, the text the
// device's table kernel runs) as a stand-alone program, so that it can run under the address and undefined-behaviour sanitizers without
// Python or a GPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o jpeg_huff_build_host tools/jpeg_huff_build_host.cpp
//     ./jpeg_huff_build_host FILE
//
// FILE holds histograms of 256 little-endian uint32 counts one behind the other.  Per histogram one line: index, 1 if the tree was
// shallow enough, its depth before limiting, the number of values, the 16 counts, the values and the 256 codes in hex.  Every output
// buffer is a heap allocation of exactly its size.  tools/jpeg_huff_build_check.py writes FILE, builds and runs the program and compares
// each line with jpeg_encode.jpeg_optimal_table_host.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../feartracker_amd/csrc/fear_jpeg_huff_build.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    std::FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) {
        std::perror(argv[1]);
        return 2;
    }
    uint32_t* freq = static_cast<uint32_t*>(std::malloc(256 * sizeof(uint32_t)));
    for (int index = 0; std::fread(freq, sizeof(uint32_t), 256, fh) == 256; ++index) {
        uint8_t* counts = static_cast<uint8_t*>(std::malloc(16));
        uint8_t* values = static_cast<uint8_t*>(std::malloc(256));
        uint32_t* codes = static_cast<uint32_t*>(std::malloc(256 * sizeof(uint32_t)));
        int32_t n_values = -1, depth = -1;
        std::memset(values, 0, 256);
        const bool ok = huff_build_serial(freq, counts, values, &n_values, codes, &depth);
        std::printf("%d %d %d %d ", index, ok ? 1 : 0, depth, n_values);
        for (int i = 0; i < 16; ++i) std::printf("%02x", counts[i]);
        std::printf(" ");
        for (int i = 0; i < n_values; ++i) std::printf("%02x", values[i]);
        std::printf(" ");
        for (int i = 0; i < 256; ++i) std::printf("%06x", codes[i]);
        std::printf("\n");
        std::free(codes);
        std::free(values);
        std::free(counts);
    }
    std::free(freq);
    std::fclose(fh);
    return 0;
}
