// The bilinear sampler of the fixed-point remaps (cv::remap with CV_16SC2 maps, INTER_LINEAR, BORDER_CONSTANT 0), written once:
// remap_linear_kernel (k_undistort.hip: one cached map per camera) and plane_warp_kernel (k_rectify.hip: one map per frame) sample with it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ah {

// Channel c of a W x H frame of cn interleaved 8-bit channels (rows row_stride bytes apart) at the position (sx + ax / 32, sy + ay / 32),
// 0 <= ax, ay < 32: the four taps weighted (32 - ax)(32 - ay) * 32 and so on (15-bit weights that sum to 1 << 15), rounded by
// + (1 << 14) >> 15. A tap outside the frame counts 0. Everything but the loads is the same for every channel of a pixel.
__device__ inline int remap_bilinear(const uint8_t* src, size_t row_stride, int W, int H, int cn, int sx, int sy, int ax, int ay, int c) {
    if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) return 0;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const bool x0in = sx >= 0 && sx < W, x1in = sx + 1 >= 0 && sx + 1 < W, y0in = sy >= 0 && sy < H, y1in = sy + 1 >= 0 && sy + 1 < H;
    const int p00 = (x0in && y0in) ? src[(size_t)sy * row_stride + (size_t)sx * cn + c] : 0;
    const int p01 = (x1in && y0in) ? src[(size_t)sy * row_stride + (size_t)(sx + 1) * cn + c] : 0;
    const int p10 = (x0in && y1in) ? src[(size_t)(sy + 1) * row_stride + (size_t)sx * cn + c] : 0;
    const int p11 = (x1in && y1in) ? src[(size_t)(sy + 1) * row_stride + (size_t)(sx + 1) * cn + c] : 0;
    const int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
    return min(max(v, 0), 255);
}

}  // namespace ah
