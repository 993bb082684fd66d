// Chessboard-corner (ChArUco) boards: the inner corners of the chessboard from the detected markers (arucohip.h, DESIGN.md "ChArUco").
//
//   charuco_corners_kernel  one wavefront per (corner, frame): lanes 0 and 1 each look one neighbour marker up and solve its 4-point
//                           homography (8 x 8, double, LDS), the wave takes the mean projection as the start, sizes the window from the
//                           distance to the markers' corners and runs the SUBPIX iteration of refine_pixels_kernel (subpix_device.h)
//   charuco_gather_kernel   one wavefront per calibration view: the found corners, in corner order, as obj / img points
//   charuco_pose_kernel     one wavefront per frame: the found corners into LDS, solve_pnp_planar_wave<64>
// The board painter is fid_paint_kernel (k_fiducial.hip, FidLayout::sq).
#include "internal.h"
#include "decode_device.h"
#include "pnp_device.h"
#include "subpix_device.h"

namespace ah {

__device__ __forceinline__ int charuco_corners(const arucohip_charuco_t& L) { return (L.squares_x - 1) * (L.squares_y - 1); }

// the marker of white square (sx, sy): row-major order of the white squares. Even rows hold them at odd sx, odd rows at even sx
__device__ __forceinline__ int charuco_marker_index(const arucohip_charuco_t& L, int sx, int sy) {
    return (sy >> 1) * L.squares_x + ((sy & 1) ? L.squares_x / 2 : 0) + (sx >> 1);
}

__global__ __launch_bounds__(64) void charuco_corners_kernel(CharucoArgs a, const arucohip_marker_t* markers, const int32_t* nmarkers, int cap_markers,
                                                             arucohip_charuco_corner_t* out, int32_t* n_found) {
    latency_bound_priority();
    __shared__ float buf[SUBPIX_PATCH * SUBPIX_PATCH];
    __shared__ double sA[2][64], sb[2][8];
    const int c = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x;
    const int ncx = a.L.squares_x - 1, iy = c / ncx, ix = c - iy * ncx;
    arucohip_charuco_corner_t* rec = out + (size_t)frame * charuco_corners(a.L) + c;
    const arucohip_marker_t* M = markers + (size_t)frame * cap_markers;
    const int nm = min(nmarkers[frame], cap_markers);   // negative: the batch gave the frame up
    const double X = (double)((ix + 1) * a.L.square_px), Y = (double)((iy + 1) * a.L.square_px);
    // the two neighbours in marker order: the white square of the upper row, then that of the lower row
    double px = 0, py = 0;
    int used = 0, mi = -1;
    if (lane < 2) {
        const int odd = (ix + iy) & 1;
        const int sy = iy + lane, sx = ix + (lane == 0 ? 1 - odd : odd);
        const int id = a.ids[charuco_marker_index(a.L, sx, sy)];
        for (int i = 0; i < nm; i++)
            if (M[i].id == id) {
                mi = i;
                break;
            }
        if (mi >= 0) {
            const int m = (a.L.square_px - a.L.marker_px) / 2;
            const float x0 = (float)(sx * a.L.square_px + m), y0 = (float)(sy * a.L.square_px + m), x1 = x0 + (float)a.L.marker_px, y1 = y0 + (float)a.L.marker_px;
            const float bx[4] = {x0, x1, x1, x0}, by[4] = {y0, y0, y1, y1};
            double* A = sA[lane];
            double* b = sb[lane];
            for (int i = 0; i < 64; i++) A[i] = 0;
            for (int i = 0; i < 4; i++) {
                const double sxd = bx[i], syd = by[i], dx = M[mi].corners[2 * i], dy = M[mi].corners[2 * i + 1];
                double* r0 = A + i * 8;
                double* r1 = A + (i + 4) * 8;
                r0[0] = r1[3] = sxd, r0[1] = r1[4] = syd, r0[2] = r1[5] = 1;
                r0[6] = -sxd * dx, r0[7] = -syd * dx, r1[6] = -sxd * dy, r1[7] = -syd * dy;
                b[i] = dx, b[i + 4] = dy;
            }
            if (solve8(A, b)) {
                const double w = b[6] * X + b[7] * Y + 1.0;
                if (w > 0) px = (b[0] * X + b[1] * Y + b[2]) / w, py = (b[3] * X + b[4] * Y + b[5]) / w, used = 1;
            }
        }
    }
    const int u0 = __shfl(used, 0, 64), u1 = __shfl(used, 1, 64), nused = u0 + u1;
    const double px0 = __shfl(px, 0, 64), py0 = __shfl(py, 0, 64), px1 = __shfl(px, 1, 64), py1 = __shfl(py, 1, 64);
    double sxd = 0, syd = 0;
    if (nused == 2)
        sxd = (px0 + px1) / 2.0, syd = (py0 + py1) / 2.0;
    else if (nused == 1)
        sxd = u0 ? px0 : px1, syd = u0 ? py0 : py1;
    const float fx = (float)sxd, fy = (float)syd;
    int win = 0;
    bool found = nused >= a.min_markers && nused > 0;
    if (found) {
        double d = DBL_MAX;
        if (used)
            for (int i = 0; i < 4; i++) {
                const double ex = sxd - (double)M[mi].corners[2 * i], ey = syd - (double)M[mi].corners[2 * i + 1];
                d = fmin(d, sqrt(ex * ex + ey * ey));
            }
        d = fmin(__shfl(d, 0, 64), __shfl(d, 1, 64));
        const double wv = floor(d * 0.70710678118654752) - 1.0;
        win = wv > (double)a.max_win ? a.max_win : (int)wv;
        const double lim = (double)(win + 1);
        found = win >= 2 && !((double)fx - lim < 0 || (double)fx + lim > (double)(a.width - 1) || (double)fy - lim < 0 || (double)fy + lim > (double)(a.height - 1));
    }
    float rx = fx, ry = fy;
    if (found)   // uniform over the wave
        subpix_refine_wave(a.gray + (size_t)frame * a.frame_stride, a.row_stride, a.width, a.height, fx, fy, win, buf, lane, &rx, &ry);
    if (lane == 0) {
        rec->x = rx, rec->y = ry, rec->start_x = fx, rec->start_y = fy;
        rec->found = found ? 1 : 0, rec->win = win, rec->markers = nused, rec->pad_ = 0;
        if (found) atomicAdd(&n_found[frame], 1);
    }
}

void launch_charuco_corners(hipStream_t s, int nframes, const Buffers& b, const CharucoArgs& a, arucohip_charuco_corner_t* out, int32_t* n_found) {
    const int nc = (a.L.squares_x - 1) * (a.L.squares_y - 1);
    hipLaunchKernelGGL(charuco_corners_kernel, dim3(nc, nframes), dim3(64), 0, s, a, (const arucohip_marker_t*)b.markers, (const int32_t*)b.nmarkers,
                       b.cap_markers, out, n_found);
}

// the object point of corner c: its board pixel times `scale`, rounded to float as calib_gather_kernel rounds a board's points
__device__ __forceinline__ void charuco_obj(const arucohip_charuco_t& L, double scale, int c, float* o) {
    const int ncx = L.squares_x - 1, iy = c / ncx, ix = c - iy * ncx;
    o[0] = (float)((float)((ix + 1) * L.square_px) * scale), o[1] = (float)((float)((iy + 1) * L.square_px) * scale), o[2] = (float)(0.f * scale);
}

// All 64 lanes: the found corners of rec[0 .. nc) in corner order to obj / img; returns their number (on every lane)
__device__ __forceinline__ int charuco_compact(const arucohip_charuco_t& L, double scale, const arucohip_charuco_corner_t* rec, int nc, int lane, float* obj,
                                               float* img) {
    int n = 0;
    for (int base = 0; base < nc; base += 64) {
        const int c = base + lane;
        const bool keep = c < nc && rec[c].found != 0;
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int dst = n + __popcll(bal & ((1ull << lane) - 1ull));
            charuco_obj(L, scale, c, obj + 3 * dst);
            img[2 * dst] = rec[c].x, img[2 * dst + 1] = rec[c].y;
        }
        n += __popcll(bal);
    }
    return n;
}

__global__ __launch_bounds__(64) void charuco_gather_kernel(arucohip_charuco_t L, double scale, const arucohip_charuco_corner_t* rec, const int2* views,
                                                            int nviews, float* obj, float* img, int32_t* npt) {
    const int v = blockIdx.x, lane = threadIdx.x;
    if (v >= nviews) return;
    const int nc = charuco_corners(L), frame = views[v].x, off = views[v].y;
    const int n = charuco_compact(L, scale, rec + (size_t)frame * nc, nc, lane, obj + (size_t)off * 3, img + (size_t)off * 2);
    if (lane == 0) npt[v] = n;
}

void launch_charuco_gather(hipStream_t s, const arucohip_charuco_t& L, double scale, const arucohip_charuco_corner_t* rec, const int2* views, int nviews,
                           float* obj, float* img, int32_t* npt) {
    hipLaunchKernelGGL(charuco_gather_kernel, dim3(nviews), dim3(64), 0, s, L, scale, rec, views, nviews, obj, img, npt);
}

__global__ __launch_bounds__(64) void charuco_pose_kernel(arucohip_charuco_t L, double scale, const arucohip_charuco_corner_t* rec, int min_corners,
                                                          CamModel cam, arucohip_board_t* out) {
    latency_bound_priority();
    __shared__ float s_obj[CALIB_MAX_POINTS * 3], s_img[CALIB_MAX_POINTS * 2];
    const int frame = blockIdx.x, lane = threadIdx.x, nc = charuco_corners(L);   // nc <= CALIB_MAX_POINTS: checked by the host
    const int n = charuco_compact(L, scale, rec + (size_t)frame * nc, nc, lane, s_obj, s_img);
    __syncthreads();
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    bool ok = false;
    if (n >= min_corners && cam.has_K) {   // uniform over the wave
        ok = solve_pnp_planar_wave<64>(s_obj, s_img, n, cam, r, t, lane);
        if (ok && cam.y_perp) rotate_x_axis(r);
    }
    if (lane == 0) {
        arucohip_board_t* o = out + frame;
        o->n_markers = n, o->has_pose = ok ? 1 : 0;
        for (int k = 0; k < 3; k++) o->rvec[k] = ok ? r[k] : 0, o->tvec[k] = ok ? t[k] : 0;
    }
}

void launch_charuco_pose(hipStream_t s, const arucohip_charuco_t& L, double scale, const arucohip_charuco_corner_t* rec, int nframes, int min_corners,
                         const CamModel& cam, arucohip_board_t* out) {
    hipLaunchKernelGGL(charuco_pose_kernel, dim3(nframes), dim3(64), 0, s, L, scale, rec, min_corners, cam, out);
}

}  // namespace ah
