// fear_jpeg_tables.h — the two constant tables of ITU-T T.81 that the JPEG code reads, each written once: the zigzag order and the base
// quantiser tables of annex K.  Plain C++17 for the host (fear_jpeg_entropy.h and fear_jpeg_progressive.h also compile stand-alone with
// g++ or clang++: tools/jpeg_entropy_host.cpp, tools/jpeg_progressive_host.cpp); under hipcc a copy of each in device memory, initialised
// from the host's as fear_jpeg_encode.h's kEncCodes is.  Host code indexes kZigzag and kBaseQuant, kernels kZigzagDev.v and kBaseQuantDev.v.
#ifndef FEAR_JPEG_TABLES_H
#define FEAR_JPEG_TABLES_H

#include <cstdint>

namespace fear_jpeg {

// zigzag position -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the standard luminance and chrominance tables (annex K.1 and K.2), natural order
constexpr uint8_t kBaseQuant[128] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99,  99,  99,  99,  18, 21, 26, 66, 99,  99,  99,  99,  24, 26, 56, 99, 99,  99,  99,  99,  47, 66, 99, 99, 99,  99,  99,  99,
    99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99};

#ifdef __HIPCC__
template <int N>
struct TableBytes {
    uint8_t v[N];
};
template <int N>
constexpr TableBytes<N> table_bytes(const uint8_t (&a)[N]) {
    TableBytes<N> t{};
    for (int i = 0; i < N; ++i) t.v[i] = a[i];
    return t;
}
__device__ const TableBytes<64> kZigzagDev = table_bytes(kZigzag);
__device__ const TableBytes<128> kBaseQuantDev = table_bytes(kBaseQuant);
#endif

}  // namespace fear_jpeg

#endif  // FEAR_JPEG_TABLES_H
