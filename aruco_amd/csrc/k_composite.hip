// Plane compositing: a texture blended onto the plane of every frame, in place, seen through the camera and its lens and hidden where a
// mask says so. The inverse direction of k_rectify.hip: it runs over frame pixels, needs the inverse lens model per pixel and leaves
// everything outside the texture's footprint untouched. No reference counterpart.
//
// The rule for frame pixel (u, v) of a frame with map N (row-major, double), in this order and in double, unfused (-ffp-contract=off):
//   valid[f] == 0, or mask byte 0: untouched
//   the ray: undistort_point (pnp_device.h) with dist; x = (u - cx) (1 / fx), y likewise, with K alone; x = u, y = v without a camera
//   S = (N0 x + N1 y) + N2, T = (N3 x + N4 y) + N5, Q = (N6 x + N7 y) + N8; !(Q > 0): untouched; s = S / Q, t = T / Q; not finite: untouched
//   is = rint_half_even(clamp(s * 32, -2^31, 2^31 - 1)), it likewise; painted iff 0 <= is <= 32 (tw - 1) and 0 <= it <= 32 (th - 1)
//   C_c = remap_bilinear at (is >> 5, it >> 5, is & 31, it & 31), A = the same sample of the alpha channel or 255, w = (A opacity + 127) / 255
//   w == 0: untouched; else out_c = (C_c w + frame_c (255 - w) + 127) / 255
// tests/composite_ref.py restates it in numpy.
#include "internal.h"
#include "plane_device.h"
#include "pnp_device.h"
#include "remap_device.h"

namespace ah {

// plane_warp_kernel's shape: a wave covers 64 x 4 frame pixels (16 lanes of 4 adjacent pixels by 4 rows), the four waves of a workgroup
// 64 x 16, so that a wave's texture footprint is a compact patch.
constexpr int PC_TILE_W = 64, PC_TILE_H = 16;

// The fixed-point texel position of frame pixel (u, v); false: the pixel is not painted. N and c are uniform (scalar registers).
template <bool DIST>
__device__ inline bool composite_position(const double* __restrict__ N, const PlaneComposite& c, int u, int v, int* is, int* it) {
    double x, y;
    if (DIST) {
        undistort_point((double)u, (double)v, c.K, c.k, &x, &y);
    } else {
        const double fx = c.K[0], fy = c.K[4], cx = c.K[2], cy = c.K[5];
        const double ifx = 1. / fx, ify = 1. / fy;
        x = ((double)u - cx) * ifx, y = ((double)v - cy) * ify;
    }
    const double S = (N[0] * x + N[1] * y) + N[2], T = (N[3] * x + N[4] * y) + N[5], Q = (N[6] * x + N[7] * y) + N[8];
    if (!(Q > 0)) return false;
    const double s = S / Q, t = T / Q;
    if (!isfinite(s) || !isfinite(t)) return false;
    const int a = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, s * 32)));
    const int b = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, t * 32)));
    *is = a, *it = b;
    // inside the box of texel centres: every tap with a non-zero weight is inside the texture
    return a >= 0 && a <= 32 * (c.tex_width - 1) && b >= 0 && b <= 32 * (c.tex_height - 1);
}

template <bool DIST, int CN, bool ALPHA>
__global__ __launch_bounds__(256) void plane_composite_kernel(PlaneComposite a) {
    const int f = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * PC_TILE_W + (lane & 15) * 4, y = blockIdx.y * PC_TILE_H + wave * 4 + (lane >> 4);
    if (x0 >= a.width || y >= a.height) return;
    if (a.valid && a.valid[f] == 0) return;   // uniform: an invalid frame reads nothing
    const int npx = min(4, a.width - x0);
    // bit i: pixel i of the lane is inside the row and not masked
    uint32_t live = (1u << npx) - 1;
    if (a.masks) {
        const uint8_t* m = a.masks + ((size_t)f * a.height + y) * a.width + x0;
        if (npx == 4 && ((uintptr_t)m & 3) == 0) {
            const uint32_t four = *(const uint32_t*)m;
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (((four >> (8 * i)) & 255) == 0) live &= ~(1u << i);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < npx && m[i] == 0) live &= ~(1u << i);
        }
    }
    if (!live) return;
    constexpr int TCN = CN + (ALPHA ? 1 : 0);
    const double* __restrict__ N = a.maps + (size_t)f * 9;
    const uint8_t* tex = a.tex + (size_t)f * a.tex_frame_stride;
    uint8_t* d = a.frames + (size_t)f * a.frame_stride + (size_t)y * a.row_stride + (size_t)x0 * CN;
    // the lane's 4 * CN bytes, packed as they lie in memory, and the pixels of them that are painted
    uint32_t word[CN], painted = 0;
#pragma unroll
    for (int k = 0; k < CN; k++) word[k] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int is, it;
        if (!((live >> i) & 1) || !composite_position<DIST>(N, a, x0 + i, y, &is, &it)) continue;
        const int sx = is >> 5, sy = it >> 5, ax = is & 31, ay = it & 31;
        const int A = ALPHA ? remap_bilinear(tex, a.tex_row_stride, a.tex_width, a.tex_height, TCN, sx, sy, ax, ay, CN) : 255;
        const int w = (A * a.opacity + 127) / 255;
        if (w == 0) continue;
        painted |= 1u << i;
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const int b = i * CN + c;
            int out = remap_bilinear(tex, a.tex_row_stride, a.tex_width, a.tex_height, TCN, sx, sy, ax, ay, c);
            if (w < 255) out = (out * w + (int)d[b] * (255 - w) + 127) / 255;
            word[b >> 2] |= (uint32_t)out << (8 * (b & 3));
        }
    }
    if (!painted) return;
    if (painted == 15 && ((uintptr_t)d & 3) == 0) {
#pragma unroll
        for (int k = 0; k < CN; k++) ((uint32_t*)d)[k] = word[k];
    } else {   // pixels that keep their value among the four, a row's tail, or an address that is not dword aligned
#pragma unroll
        for (int b = 0; b < 4 * CN; b++)
            if ((painted >> (b / CN)) & 1) d[b] = (uint8_t)(word[b >> 2] >> (8 * (b & 3)));
    }
}

// One lane per frame: M as plane_maps_kernel computes it (window pixel -> camera-frame point), then its adjugate (ray -> window pixel
// up to scale), signed so that Q > 0 holds exactly for rays that meet the plane in front of the camera. No pose, an entry of M that is not
// finite, or a determinant that is zero or not finite: valid = 0 and a zero map.
__global__ __launch_bounds__(64) void plane_inverse_maps_kernel(const arucohip_board_t* boards, int nframes, arucohip_rectify_t win, double* maps, int32_t* valid) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const arucohip_board_t b = boards[f];
    double M[9], N[9];
    bool ok = plane_map_of_board(b, win, M);
    N[0] = M[4] * M[8] - M[5] * M[7], N[1] = M[2] * M[7] - M[1] * M[8], N[2] = M[1] * M[5] - M[2] * M[4];
    N[3] = M[5] * M[6] - M[3] * M[8], N[4] = M[0] * M[8] - M[2] * M[6], N[5] = M[2] * M[3] - M[0] * M[5];
    N[6] = M[3] * M[7] - M[4] * M[6], N[7] = M[1] * M[6] - M[0] * M[7], N[8] = M[0] * M[4] - M[1] * M[3];
    const double det = (M[0] * N[0] + M[1] * N[3]) + M[2] * N[6];
    ok = ok && isfinite(det) && det != 0;
    for (int k = 0; k < 9; k++) maps[(size_t)f * 9 + k] = ok ? (det < 0 ? -N[k] : N[k]) : 0.0;
    valid[f] = ok ? 1 : 0;
}

template <bool DIST, int CN>
static auto composite_kernel_of(bool alpha) { return alpha ? plane_composite_kernel<DIST, CN, true> : plane_composite_kernel<DIST, CN, false>; }

void launch_plane_composite(hipStream_t s, const PlaneComposite& args, int cn, bool alpha, bool dist, int nframes) {
    auto kernel = cn == 3 ? (dist ? composite_kernel_of<true, 3>(alpha) : composite_kernel_of<false, 3>(alpha))
                          : (dist ? composite_kernel_of<true, 1>(alpha) : composite_kernel_of<false, 1>(alpha));
    const dim3 tiles((args.width + PC_TILE_W - 1) / PC_TILE_W, (args.height + PC_TILE_H - 1) / PC_TILE_H);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {   // the grid's z limit
        PlaneComposite a = args;
        a.frames += (size_t)f0 * a.frame_stride, a.tex += (size_t)f0 * a.tex_frame_stride, a.maps += (size_t)f0 * 9;
        if (a.valid) a.valid += f0;
        if (a.masks) a.masks += (size_t)f0 * a.height * a.width;
        hipLaunchKernelGGL(kernel, dim3(tiles.x, tiles.y, std::min(65535, nframes - f0)), dim3(256), 0, s, a);
    }
}

void launch_plane_inverse_maps(hipStream_t s, const arucohip_board_t* boards, int nframes, const arucohip_rectify_t& win, double* maps, int32_t* valid) {
    hipLaunchKernelGGL(plane_inverse_maps_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, boards, nframes, win, maps, valid);
}

}  // namespace ah
