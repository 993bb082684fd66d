// Device function shared by the colour-to-grey kernels (k_convert.hip, k_ingest.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ah {

// cv::cvtColor(CV_BGR2GRAY) for 8-bit data: coefficients 0.114, 0.587, 0.299 in 14 bits
__device__ __forceinline__ uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }

}  // namespace ah
