// The map of a window on a board's plane, written once: plane_maps_kernel (k_rectify.hip) stores it, plane_inverse_maps_kernel
// (k_composite.hip) inverts it.
#pragma once
#include "internal.h"
#include "pnp_device.h"

namespace ah {

// The columns of M are R (ux, uy, 0), R (vx, vy, 0) and R (x0, y0, 0) + t with R = Rodrigues(rvec), so that M (u, v, 1) is the camera-frame
// point of window pixel (u, v). False: no pose, or an entry that is not finite (M is then whatever the arithmetic gave).
__device__ inline bool plane_map_of_board(const arucohip_board_t& b, const arucohip_rectify_t& win, double* M) {
    double R[9];
    rodrigues_vec2mat(b.rvec, R, nullptr);
    const double ux = win.ux, uy = win.uy, vx = win.vx, vy = win.vy, x0 = win.x0, y0 = win.y0;
    bool ok = b.has_pose != 0;
    for (int i = 0; i < 3; i++) {
        M[3 * i] = R[3 * i] * ux + R[3 * i + 1] * uy;
        M[3 * i + 1] = R[3 * i] * vx + R[3 * i + 1] * vy;
        M[3 * i + 2] = (R[3 * i] * x0 + R[3 * i + 1] * y0) + b.tvec[i];
    }
    for (int k = 0; k < 9; k++) ok = ok && isfinite(M[k]);
    return ok;
}

}  // namespace ah
