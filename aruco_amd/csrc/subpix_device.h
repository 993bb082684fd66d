// cv::cornerSubPix on one 64-lane wavefront, shared by refine_pixels_kernel (k_refine.hip: the detector's SUBPIX corner method) and
// charuco_corners_kernel (k_charuco.hip): the patch in LDS, the five sums across the lanes in double.
// Reference: cv::cornerSubPix(grey, corners, Size(win, win), Size(-1, -1), {MAX_ITER | EPS, 8, 0.005}), src/markerdetector.cpp:402-405.
#pragma once
#include <float.h>

#include "internal.h"

namespace ah {

constexpr int SUBPIX_MAX_WIN = 15;                       // half window the LDS patch holds
constexpr int SUBPIX_PATCH = 2 * SUBPIX_MAX_WIN + 3;     // (2 win + 1) + 2 pixels a side

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// All 64 lanes of a one-wave workgroup call it with the same arguments. src: the W x H frame, rows st bytes apart; (cTx, cTy): the
// start; buf: SUBPIX_PATCH^2 floats of LDS. Every lane gets the refined corner; a corner that moved more than win is reset to the start.
__device__ __forceinline__ void subpix_refine_wave(const uint8_t* src, size_t st, int W, int H, float cTx, float cTy, int win, float* buf, int lane,
                                                   float* rx, float* ry) {
    const int ww = 2 * win + 1, pw = ww + 2;
    float cIx = cTx, cIy = cTy;
    int iter = 0;
    double err = 0;
    const double eps = 0.005 * 0.005;
    do {
        // getRectSubPix 8u -> 32f, (ww+2)^2 patch around cI
        float ox = cIx - (pw - 1) * 0.5f, oy = cIy - (pw - 1) * 0.5f;
        int ix = (int)floorf(ox), iy = (int)floorf(oy);
        float fa = ox - ix, fb = oy - iy;
        float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
        __syncthreads();
        for (int i = lane; i < pw * pw; i += WAVE) {
            int r = i / pw, c = i - r * pw;
            int y0 = clampi(iy + r, 0, H - 1), y1 = clampi(iy + r + 1, 0, H - 1);
            int x0 = clampi(ix + c, 0, W - 1), x1 = clampi(ix + c + 1, 0, W - 1);
            float s0 = src[y0 * st + x0] * a11 + src[y0 * st + x1] * a12 + src[y1 * st + x0] * a21 + src[y1 * st + x1] * a22;
            buf[i] = s0;
        }
        __syncthreads();
        double A = 0, B = 0, C = 0, bb1 = 0, bb2 = 0;
        for (int k = lane; k < ww * ww; k += WAVE) {
            int i = k / ww, j = k - i * ww;
            float y = (float)(i - win) / win, x = (float)(j - win) / win;
            float vy = expf(-y * y);
            double m = (double)(float)(vy * expf(-x * x));
            const float* sp = buf + (i + 1) * pw + (j + 1);
            double tgx = (double)sp[1] - (double)sp[-1];
            double tgy = (double)sp[pw] - (double)sp[-pw];
            double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            double px = j - win, py = i - win;
            A += gxx, B += gxy, C += gyy;
            bb1 += gxx * px + gxy * py;
            bb2 += gxy * px + gyy * py;
        }
        A = wave_sum(A), B = wave_sum(B), C = wave_sum(C), bb1 = wave_sum(bb1), bb2 = wave_sum(bb2);
        double det = A * C - B * B;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        double scale = 1.0 / det;
        float nx = (float)(cIx + C * scale * bb1 - B * scale * bb2);
        float ny = (float)(cIy - B * scale * bb1 + A * scale * bb2);
        err = (nx - cIx) * (nx - cIx) + (ny - cIy) * (ny - cIy);
        cIx = nx, cIy = ny;
        if (cIx < 0 || cIx >= W || cIy < 0 || cIy >= H) break;
    } while (++iter < 8 && err > eps);
    if (fabsf(cIx - cTx) > win || fabsf(cIy - cTy) > win) cIx = cTx, cIy = cTy;
    *rx = cIx, *ry = cIy;
}

}  // namespace ah
