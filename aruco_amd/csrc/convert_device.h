// Device functions shared by the colour-to-grey kernels and the format conversions (k_convert.hip, k_ingest.hip, k_egress.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ah {

// cv::cvtColor(CV_BGR2GRAY) for 8-bit data: coefficients 0.114, 0.587, 0.299 in 14 bits
__device__ __forceinline__ uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }

// bytes [0, nbytes) of p as a little-endian word (the others 0); whole: p is dword aligned and all four bytes are the row's
__device__ __forceinline__ uint32_t ld32(const uint8_t* p, int nbytes, bool whole) {
    if (whole) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < nbytes) v |= (uint32_t)p[j] << (8 * j);
    return v;
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v, 0), 255); }

}  // namespace ah
