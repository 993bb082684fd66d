// BoardDetector::detect's pose of one frame on one 64-lane wavefront (boarddetector.cpp:157-198), shared by board_pose_kernel
// (k_finalize.hip) and the marker recovery (k_recover.hip): lane 0 filters the frame's markers by board id and lays out the 3-D / 2-D
// correspondences in LDS, then the 64 lanes share the points of solvePnP (any rigid point set: pnp3d_device.h); optional reprojection
// filter and second solve.
#pragma once
#include "internal.h"
#include "pnp3d_device.h"

namespace ah {

constexpr int MAX_BOARD_POINTS = 512;

// LDS of one frame's board solve. Each solve of a board out of z = 0 borrows the object points of the other one for its plane-frame points:
// obj2 is not filled before the first solve is over, obj is not read after the filter.
struct BoardLds {
    Pnp3dLds w3d;
    float obj[MAX_BOARD_POINTS * 3], img[MAX_BOARD_POINTS * 2], obj2[MAX_BOARD_POINTS * 3], img2[MAX_BOARD_POINTS * 2];
    int npts, nmark, n2;
};

// All 64 lanes call it. M[0 .. nm): the frame's markers. Returns BOARD_NOT_TRIED without K, without a member marker or on a PIX board
// without a marker size, else whether the solve gave a pose; r / t hold what the solver left, BEFORE rotateXAxis (on every lane),
// *nk_out the member markers found.
enum { BOARD_NOT_TRIED = 0, BOARD_NO_POSE = 1, BOARD_POSE = 2 };
__device__ __forceinline__ int board_solve_wave(const arucohip_marker_t* M, int nm, const BoardDef& bd, const CamModel& cam, uint32_t* counters,
                                                 BoardLds& s, int lane, double* r, double* t, int* nk_out) {
    if (lane == 0) {
        const double mpp = board_mpp(bd);
        int np = 0, nk = 0;
        for (int i = 0; i < nm; i++) {
            int slot = -1;
            for (int j = 0; j < bd.nboard; j++)
                if (bd.ids[j] == M[i].id) {
                    slot = j;
                    break;
                }
            if (slot < 0) continue;
            nk++;
            if (np + 4 > MAX_BOARD_POINTS) {   // more correspondences than the kernel holds: reported, never silent
                atomicOr(&counters[CNT_STATUS], (uint32_t)ST_MARKER_OVERFLOW);
                continue;
            }
            for (int p = 0; p < 4; p++, np++) {
                s.img[2 * np] = M[i].corners[2 * p], s.img[2 * np + 1] = M[i].corners[2 * p + 1];
                const float* q = bd.obj + ((size_t)slot * 4 + p) * 3;
                for (int c = 0; c < 3; c++) s.obj[3 * np + c] = (float)(q[c] * mpp);
            }
        }
        s.npts = np, s.nmark = nk;
    }
    __syncthreads();
    const int np = s.npts, nk = s.nmark;
    *nk_out = nk;
    for (int k = 0; k < 3; k++) r[k] = t[k] = 0;
    const bool enough = (bd.marker_size > 0 && bd.info_type == ARUCOHIP_BOARD_PIX) || bd.info_type == ARUCOHIP_BOARD_METERS;
    if (!(nk > 0 && cam.has_K && enough)) return BOARD_NOT_TRIED;
    bool ok = solve_pnp_wave3d(s.obj, s.img, np, cam, r, t, lane, s.obj2, s.w3d);
    if (bd.repj_thres > 0 && ok) {
        double R[9];
        rodrigues_vec2mat(r, R, nullptr);
        if (lane == 0) s.n2 = 0;
        __syncthreads();
        for (int base = 0; base < np; base += 64) {   // order-preserving compaction of the points that pass
            const int i = base + lane;
            bool keep = false;
            if (i < np) {
                double mx, my;
                project_point(s.obj[3 * i], s.obj[3 * i + 1], s.obj[3 * i + 2], R, nullptr, t, cam.K, cam.k, &mx, &my, nullptr, nullptr);
                const float ex = (float)mx - s.img[2 * i], ey = (float)my - s.img[2 * i + 1];
                keep = (float)sqrt((double)ex * ex + (double)ey * ey) < bd.repj_thres;
            }
            const unsigned long long bal = __ballot(keep);
            const int dst = s.n2 + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep) {
                for (int c = 0; c < 3; c++) s.obj2[3 * dst + c] = s.obj[3 * i + c];
                s.img2[2 * dst] = s.img[2 * i], s.img2[2 * dst + 1] = s.img[2 * i + 1];
            }
            __syncthreads();
            if (lane == 0) s.n2 += __popcll(bal);
            __syncthreads();
        }
        // fewer than 4 surviving points: the reference's second solvePnP would throw; keep the first pose, flag no pose
        ok = s.n2 >= 4 && solve_pnp_wave3d(s.obj2, s.img2, s.n2, cam, r, t, lane, s.obj, s.w3d);
    }
    return ok ? BOARD_POSE : BOARD_NO_POSE;
}

}  // namespace ah
