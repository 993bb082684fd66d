// Camera calibration from planar views (cv::calibrateCamera, pinhole + k1 k2 p1 p2 k3), FP64 throughout. The same solver calibrates a
// fisheye lens (CalibState::model, arucohip_fisheye_calibrate*): another projection and another start, everything else as below.
//
// Views are given as points (obj xyz float, img xy float) at d.off[v], d.npt[v] points each. One wave per view does everything
// that touches the view's points; the few kernels that combine views run on one workgroup and add the views in view order, so
// the result does not depend on scheduling (no floating-point atomics).
//   init:   calib_homography_kernel (per view: DLT homography plane -> pixel, the two vanishing-point rows of initIntrinsicParams2D)
//           calib_focal_kernel      (one thread: least squares fx, fy over all views)
//           calib_pose_kernel       (per view: planar solvePnP with the start intrinsics)
//   LM:     calib_normal_kernel     (per view: Gram matrix of [J_intr | J_pose | r], elimination of the view's pose -> S_i, reduced rhs)
//           calib_solve_kernel      (sum of S_i in view order + damping, NI x NI solve on the free intrinsics)
//           calib_eval_kernel       (per view: pose back-substitution, candidate cost)
//           calib_update_kernel     (one thread: accept / reject, lambda, stopping rule: lm_decide of lm_device.h)
#include <float.h>

#include "fisheye_device.h"
#include "internal.h"
#include "pnp_device.h"

namespace ah {

// The camera model of a run (CalibState::model): the pinhole model of this file's header, or the fisheye model of fisheye_device.h, whose
// eight intrinsics fx fy cx cy k1..k4 take the first eight of the nine columns (the ninth is zero and never free).
__device__ inline void calib_project(int model, double X, double Y, double Z, const double* R, const double* dRdr, const double* t, const double* in,
                                     double* mx, double* my, double* di, double* dp) {
    if (model == CALIB_MODEL_FISHEYE)
        fisheye_project_point_d(X, Y, Z, R, dRdr, t, in, mx, my, di, dp);
    else
        project_point_d(X, Y, Z, R, dRdr, t, in, mx, my, di, dp);
}

// Jacobian rows of one point are 16 doubles: 9 intrinsic columns, 6 pose columns, the residual
constexpr int CJ = 16;
constexpr int CG = CJ * (CJ + 1) / 2;   // 136 entries of the upper triangle of the Gram matrix

// pivoted Gaussian elimination for a small run-time n (one thread, n <= 9)
__device__ inline bool solve_small(double* A, double* b, int n) {
    for (int c = 0; c < n; c++) {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (fabs(A[r * n + c]) > fabs(A[piv * n + c])) piv = r;
        if (A[piv * n + c] == 0) return false;
        if (piv != c) {
            for (int k = 0; k < n; k++) {
                const double t = A[c * n + k];
                A[c * n + k] = A[piv * n + k], A[piv * n + k] = t;
            }
            const double t = b[c];
            b[c] = b[piv], b[piv] = t;
        }
        for (int r = c + 1; r < n; r++) {
            const double f = A[r * n + c] / A[c * n + c];
            for (int k = c; k < n; k++) A[r * n + k] -= f * A[c * n + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; r--) {
        double s = b[r];
        for (int k = r + 1; k < n; k++) s -= A[r * n + k] * b[k];
        b[r] = s / A[r * n + r];
    }
    return true;
}

__device__ inline const double* view_pose(const CalibDev& d, int buf, int v) { return d.pose + ((size_t)buf * d.nviews + v) * 6; }

// ---- initialisation ---------------------------------------------------------------------------------------------------------------

// Homography plane (X, Y) -> pixel by the normalised DLT (h33 = 1, centroid / mean-absolute-deviation scaling), then the rows of
// OpenCV's initIntrinsicParams2D for this view with the principal point at st.intr[2..3]: init[v] = {A00, A01, A10, A11, b0, b1}.
__global__ __launch_bounds__(64) void calib_homography_kernel(CalibDev d) {
    const int v = blockIdx.x, lane = threadIdx.x, n = d.npt[v];
    const float* obj = d.obj + (size_t)3 * d.off[v];
    const float* img = d.img + (size_t)2 * d.off[v];
    double cM[2] = {0, 0}, cm[2] = {0, 0}, sM[2] = {0, 0}, sm[2] = {0, 0};
    for (int i = lane; i < n; i += 64) cM[0] += obj[3 * i], cM[1] += obj[3 * i + 1], cm[0] += img[2 * i], cm[1] += img[2 * i + 1];
    wave_sum_arr<64>(cM, 2), wave_sum_arr<64>(cm, 2);
    for (int k = 0; k < 2; k++) cM[k] /= n, cm[k] /= n;
    for (int i = lane; i < n; i += 64) {
        sM[0] += fabs(obj[3 * i] - cM[0]), sM[1] += fabs(obj[3 * i + 1] - cM[1]);
        sm[0] += fabs(img[2 * i] - cm[0]), sm[1] += fabs(img[2 * i + 1] - cm[1]);
    }
    wave_sum_arr<64>(sM, 2), wave_sum_arr<64>(sm, 2);
    bool ok = sM[0] > DBL_EPSILON && sM[1] > DBL_EPSILON && sm[0] > DBL_EPSILON && sm[1] > DBL_EPSILON;
    for (int k = 0; k < 2; k++) sM[k] = n / sM[k], sm[k] = n / sm[k];
    double A[64], b[8];
    for (int i = 0; i < 64; i++) A[i] = 0;
    for (int i = 0; i < 8; i++) b[i] = 0;
    for (int i = lane; i < n; i += 64) {
        const double X = (obj[3 * i] - cM[0]) * sM[0], Y = (obj[3 * i + 1] - cM[1]) * sM[1];
        const double x = (img[2 * i] - cm[0]) * sm[0], y = (img[2 * i + 1] - cm[1]) * sm[1];
        const double Lx[8] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y};
        const double Ly[8] = {0, 0, 0, X, Y, 1, -y * X, -y * Y};
        for (int j = 0; j < 8; j++) {
            for (int q = 0; q < 8; q++) A[j * 8 + q] += Lx[j] * Lx[q] + Ly[j] * Ly[q];
            b[j] += Lx[j] * x + Ly[j] * y;
        }
    }
    wave_sum_arr<64>(A, 64), wave_sum_arr<64>(b, 8);
    if (lane != 0) return;
    ok = ok && solve_spd<8>(A, b);
    double H[9];
    if (ok) {
        const double H0[9] = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], 1.0};
        const double invHnorm[9] = {1. / sm[0], 0, cm[0], 0, 1. / sm[1], cm[1], 0, 0, 1};
        const double Hnorm2[9] = {sM[0], 0, -cM[0] * sM[0], 0, sM[1], -cM[1] * sM[1], 0, 0, 1};
        double T[9];
        mat3_mul(invHnorm, H0, T);
        mat3_mul(T, Hnorm2, H);
        const double s = 1. / H[8];
        for (int i = 0; i < 9; i++) {
            H[i] *= s;
            if (!isfinite(H[i])) ok = false;
        }
    }
    double* out = d.init + (size_t)v * 6;
    if (!ok) {
        atomicOr(&d.st->lm.err, CALIB_ERR_DEGENERATE);
        for (int k = 0; k < 6; k++) out[k] = 0;
        return;
    }
    const double cx = d.st->intr[2], cy = d.st->intr[3];
    for (int j = 0; j < 3; j++) H[j] -= H[6 + j] * cx, H[3 + j] -= H[6 + j] * cy;
    double h[3], w[3], d1[3], d2[3], nn[4] = {0, 0, 0, 0};
    for (int j = 0; j < 3; j++) {
        const double t0 = H[j * 3], t1 = H[j * 3 + 1];
        h[j] = t0, w[j] = t1, d1[j] = (t0 + t1) * 0.5, d2[j] = (t0 - t1) * 0.5;
        nn[0] += t0 * t0, nn[1] += t1 * t1, nn[2] += d1[j] * d1[j], nn[3] += d2[j] * d2[j];
    }
    for (int j = 0; j < 4; j++) nn[j] = 1. / sqrt(nn[j]);
    for (int j = 0; j < 3; j++) h[j] *= nn[0], w[j] *= nn[1], d1[j] *= nn[2], d2[j] *= nn[3];
    out[0] = h[0] * w[0], out[1] = h[1] * w[1], out[2] = d1[0] * d2[0], out[3] = d1[1] * d2[1];
    out[4] = -h[2] * w[2], out[5] = -d1[2] * d2[2];
}

// least squares (1/fx^2, 1/fy^2) over the 2 rows of every view, normal equations summed in view order
__global__ void calib_focal_kernel(CalibDev d) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    CalibState* st = d.st;
    double N[4] = {0, 0, 0, 0}, r[2] = {0, 0};
    for (int v = 0; v < d.nviews; v++) {
        const double* a = d.init + (size_t)v * 6;
        for (int q = 0; q < 2; q++) {
            const double u0 = a[2 * q], u1 = a[2 * q + 1], bb = a[4 + q];
            N[0] += u0 * u0, N[1] += u0 * u1, N[3] += u1 * u1;
            r[0] += u0 * bb, r[1] += u1 * bb;
        }
    }
    N[2] = N[1];
    const double det = N[0] * N[3] - N[1] * N[2];
    const double f0 = (N[3] * r[0] - N[1] * r[1]) / det, f1 = (N[0] * r[1] - N[2] * r[0]) / det;
    double fx = sqrt(fabs(1. / f0)), fy = sqrt(fabs(1. / f1));
    if (st->flags & ARUCOHIP_CALIB_FIX_ASPECT_RATIO) {
        const double tf = (fx + fy) / (st->aspect + 1.);
        fx = st->aspect * tf, fy = tf;
    }
    if (!(det != 0 && isfinite(fx) && isfinite(fy) && fx > 0 && fy > 0)) {
        atomicOr(&st->lm.err, CALIB_ERR_DEGENERATE);
        return;
    }
    st->intr[0] = fx, st->intr[1] = fy;
}

// start pose of every view: the planar solvePnP of the detector (homography, decomposition, pose-only LM) with the start intrinsics.
// The board plane z = z0 is solved as z = 0 and moved back: t = t' - z0 * R e3.
__global__ __launch_bounds__(64) void calib_pose_kernel(CalibDev d) {
    __shared__ float s_obj[CALIB_MAX_POINTS * 3], s_img[CALIB_MAX_POINTS * 2];
    __shared__ int s_bad;
    const int v = blockIdx.x, lane = threadIdx.x, n = d.npt[v];
    const float* obj = d.obj + (size_t)3 * d.off[v];
    const float* img = d.img + (size_t)2 * d.off[v];
    const float z0 = obj[2];
    const double* in = d.st->intr;
    const bool fisheye = d.st->model == CALIB_MODEL_FISHEYE;
    if (lane == 0) s_bad = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        if (obj[3 * i + 2] != z0) s_bad = 1;
        s_obj[3 * i] = obj[3 * i], s_obj[3 * i + 1] = obj[3 * i + 1], s_obj[3 * i + 2] = 0.f;
        if (fisheye) {
            // the point undistorted with the start model, its angle clamped to 1.5 rad for this start only: normalised coordinates
            const double x = ((double)img[2 * i] - in[2]) / in[0], y = ((double)img[2 * i + 1] - in[3]) / in[1], thd = hypot(x, y);
            bool rising;
            const double th = fmin(fmax(fisheye_solve_theta(in + 4, thd, &rising), 0.0), 1.5);
            const double sc = thd > 0 ? tan(th) / thd : 1.0;
            s_img[2 * i] = (float)(x * sc), s_img[2 * i + 1] = (float)(y * sc);
        } else {
            s_img[2 * i] = img[2 * i], s_img[2 * i + 1] = img[2 * i + 1];
        }
    }
    __syncthreads();
    if (s_bad) {
        if (lane == 0) atomicOr(&d.st->lm.err, CALIB_ERR_NONPLANAR);
        return;
    }
    CamModel cam;
    cam.has_K = 1, cam.has_dist = 1, cam.marker_size = 0, cam.y_perp = 0;
    for (int i = 0; i < 9; i++) cam.K[i] = 0;
    cam.K[0] = (float)in[0], cam.K[4] = (float)in[1], cam.K[2] = (float)in[2], cam.K[5] = (float)in[3], cam.K[8] = 1.f;
    for (int i = 0; i < 8; i++) cam.k[i] = 0;
    for (int i = 0; i < 5; i++) cam.k[i] = in[4 + i];
    if (fisheye) {   // the points are normalised already: the identity camera
        cam.K[0] = cam.K[4] = 1.f, cam.K[2] = cam.K[5] = 0.f;
        for (int i = 0; i < 5; i++) cam.k[i] = 0;
    }
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    const bool ok = solve_pnp_planar_wave<64>(s_obj, s_img, n, cam, r, t, lane);
    if (lane != 0) return;
    if (!ok) atomicOr(&d.st->lm.err, CALIB_ERR_DEGENERATE);
    double R[9];
    rodrigues_vec2mat(r, R, nullptr);
    double* p = d.pose + (size_t)v * 6;   // buffer 0
    for (int k = 0; k < 3; k++) p[k] = r[k], p[3 + k] = t[k] - (double)z0 * R[k * 3 + 2];
}

// ---- Levenberg-Marquardt ----------------------------------------------------------------------------------------------------------

// Per view: the Gram matrix G = [J_c J_p r]^T [J_c J_p r] (J_c 2n x 9 intrinsics, J_p 2n x 6 pose) — 32 points at a time, their 64
// Jacobian rows in LDS, lane e accumulating entries e, e+64, e+128 over the rows in order. Then lane 0 eliminates the pose:
//   U~ = U with its diagonal times (1 + lambda), M = U~^-1 W^T, u = U~^-1 g_p
//   S_i = A - W M, rhs_i = g_c - W u
// red[v] = {S_i (81), diag A (9), rhs_i (9)}, bs[v] = {u (6), M (54)}.
__global__ __launch_bounds__(64) void calib_normal_kernel(CalibDev d) {
    __shared__ double s_j[64][CJ + 1];
    __shared__ double s_g[CG];
    const int v = blockIdx.x, lane = threadIdx.x, n = d.npt[v];
    const float* obj = d.obj + (size_t)3 * d.off[v];
    const float* img = d.img + (size_t)2 * d.off[v];
    const CalibState* st = d.st;
    double in[9];
    for (int k = 0; k < 9; k++) in[k] = st->intr[k];
    const bool fixar = st->flags & ARUCOHIP_CALIB_FIX_ASPECT_RATIO;
    const double aspect = st->aspect, lambda = lm_lambda(st->lm.lg);
    const double* p = view_pose(d, st->lm.cur, v);
    double R[9], dRdr[27];
    rodrigues_vec2mat(p, R, dRdr);
    int ea[3], eb[3];   // (row, column) of the Gram entries this lane sums
    for (int q = 0; q < 3; q++) {
        int e = lane + 64 * q, a = 0;
        ea[q] = eb[q] = -1;
        if (e >= CG) continue;
        while (e >= CJ - a) e -= CJ - a, a++;
        ea[q] = a, eb[q] = a + e;
    }
    double acc[3] = {0, 0, 0};
    for (int base = 0; base < n; base += 32) {
        const int i = base + (lane >> 1), row = lane & 1;
        double rowv[CJ];
        for (int c = 0; c < CJ; c++) rowv[c] = 0;
        if (i < n) {
            double mx, my, di[18], dp[12];
            calib_project(st->model, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], R, dRdr, p + 3, in, &mx, &my, di, dp);
            for (int c = 0; c < 9; c++) rowv[c] = di[row * 9 + c];
            if (fixar) rowv[1] += aspect * rowv[0], rowv[0] = 0;   // fx = aspect * fy: fy's column carries both
            for (int c = 0; c < 6; c++) rowv[9 + c] = dp[row * 6 + c];
            rowv[15] = row ? my - (double)img[2 * i + 1] : mx - (double)img[2 * i];
        }
        for (int c = 0; c < CJ; c++) s_j[lane][c] = rowv[c];
        __syncthreads();
        for (int q = 0; q < 3; q++)
            if (ea[q] >= 0)
                for (int r = 0; r < 64; r++) acc[q] += s_j[r][ea[q]] * s_j[r][eb[q]];
        __syncthreads();
    }
    for (int q = 0; q < 3; q++)
        if (ea[q] >= 0) s_g[lane + 64 * q] = acc[q];
    __syncthreads();
    if (lane != 0) return;
    auto G = [&](int a, int b) -> double {
        if (a > b) { const int t = a; a = b, b = t; }
        return s_g[a * CJ - a * (a - 1) / 2 + (b - a)];
    };
    double U[36], X[60];   // X: 10 right-hand sides (9 columns of W^T, g_p), solved one at a time
    for (int c = 0; c < 10; c++) {
        double Uc[36], bc[6];
        for (int a = 0; a < 6; a++) {
            for (int b = 0; b < 6; b++) Uc[a * 6 + b] = G(9 + a, 9 + b);
            Uc[a * 7] *= 1. + lambda;
            bc[a] = c < 9 ? G(c, 9 + a) : G(9 + a, 15);
        }
        if (!solve_static<6>(Uc, bc))
            for (int a = 0; a < 6; a++) bc[a] = 0;
        for (int a = 0; a < 6; a++) X[c * 6 + a] = bc[a];
    }
    double* red = d.red + (size_t)v * CALIB_RED;
    double* bs = d.bs + (size_t)v * CALIB_BS;
    for (int i = 0; i < 9; i++) {
        for (int j = 0; j < 9; j++) {
            double s = G(i, j);
            for (int a = 0; a < 6; a++) s -= G(i, 9 + a) * X[j * 6 + a];
            red[i * 9 + j] = s;
        }
        red[81 + i] = G(i, i);
        double r = G(i, 15);
        for (int a = 0; a < 6; a++) r -= G(i, 9 + a) * X[54 + a];
        red[90 + i] = r;
    }
    for (int a = 0; a < 6; a++) bs[a] = X[54 + a];
    for (int j = 0; j < 9; j++)
        for (int a = 0; a < 6; a++) bs[6 + a * 9 + j] = X[j * 6 + a];
}

// Sum of the views' reduced systems in view order (thread e owns entry e), damping of the intrinsic block by its own diagonal,
// solve on the free intrinsics. st->delta = the intrinsic step, st->cand = intr - delta.
__global__ __launch_bounds__(128) void calib_solve_kernel(CalibDev d) {
    __shared__ double s_sum[CALIB_RED];
    const int e = threadIdx.x;
    if (e < 99) {
        double s = 0;
        for (int v = 0; v < d.nviews; v++) s += d.red[(size_t)v * CALIB_RED + e];
        s_sum[e] = s;
    }
    __syncthreads();
    if (e != 0) return;
    CalibState* st = d.st;
    const double lambda = lm_lambda(st->lm.lg);
    int fr[9], nf = 0;
    for (int i = 0; i < 9; i++)
        if (st->free_mask & (1 << i)) fr[nf++] = i;
    double A[81], b[9], delta[9];
    for (int a = 0; a < nf; a++) {
        for (int c = 0; c < nf; c++) A[a * nf + c] = s_sum[fr[a] * 9 + fr[c]];
        A[a * nf + a] += lambda * s_sum[81 + fr[a]];
        b[a] = s_sum[90 + fr[a]];
    }
    if (nf > 0 && !solve_small(A, b, nf))
        for (int a = 0; a < nf; a++) b[a] = 0;
    for (int i = 0; i < 9; i++) delta[i] = 0;
    for (int a = 0; a < nf; a++) delta[fr[a]] = b[a];
    for (int i = 0; i < 9; i++) st->delta[i] = delta[i], st->cand[i] = st->intr[i] - delta[i];
    if (st->flags & ARUCOHIP_CALIB_FIX_ASPECT_RATIO) st->cand[0] = st->aspect * st->cand[1];
}

// Per view: step = 0 evaluates the cost at the current parameters into vcost[cur]; step = 1 back-substitutes the pose step
// dp = u - M delta, writes the candidate pose to the other buffer, its cost to vcost[other] and |dp|^2, |p|^2 to vchg.
__global__ __launch_bounds__(64) void calib_eval_kernel(CalibDev d, int step) {
    const int v = blockIdx.x, lane = threadIdx.x, n = d.npt[v];
    const float* obj = d.obj + (size_t)3 * d.off[v];
    const float* img = d.img + (size_t)2 * d.off[v];
    const CalibState* st = d.st;
    const int cur = st->lm.cur, dst = step ? 1 - cur : cur;
    const double* p0 = view_pose(d, cur, v);
    double in[9], p[6], dn = 0, pn = 0;
    for (int k = 0; k < 9; k++) in[k] = step ? st->cand[k] : st->intr[k];
    for (int k = 0; k < 6; k++) p[k] = p0[k];
    if (step) {
        const double* bs = d.bs + (size_t)v * CALIB_BS;
        for (int a = 0; a < 6; a++) {
            double s = bs[a];
            for (int j = 0; j < 9; j++) s -= bs[6 + a * 9 + j] * st->delta[j];
            dn += s * s, pn += p[a] * p[a];
            p[a] -= s;
        }
    }
    double R[9];
    rodrigues_vec2mat(p, R, nullptr);
    double e2 = 0;
    for (int i = lane; i < n; i += 64) {
        double mx, my;
        calib_project(st->model, obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], R, nullptr, p + 3, in, &mx, &my, nullptr, nullptr);
        const double ex = mx - (double)img[2 * i], ey = my - (double)img[2 * i + 1];
        e2 += ex * ex + ey * ey;
    }
    e2 = wave_sum_d<64>(e2);
    if (lane != 0) return;
    d.vcost[(size_t)dst * d.nviews + v] = e2;
    if (step) {
        double* q = d.pose + ((size_t)dst * d.nviews + v) * 6;
        for (int k = 0; k < 6; k++) q[k] = p[k];
        d.vchg[2 * v] = dn, d.vchg[2 * v + 1] = pn;
    }
}

// One thread: the cost over the views in view order; step 0 records the start, a step decides by lm_decide, and an accepted
// candidate's intrinsics become the current ones. The step norms add the views, then the intrinsics.
__global__ void calib_update_kernel(CalibDev d, int step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    CalibState* st = d.st;
    const int other = step ? 1 - st->lm.cur : st->lm.cur;
    double c = 0;
    for (int v = 0; v < d.nviews; v++) c += d.vcost[(size_t)other * d.nviews + v];
    if (!step) {
        st->lm.cost = c;
        if (!isfinite(c)) st->lm.err |= CALIB_ERR_DEGENERATE;
        return;
    }
    double dn = 0, pn = 0;
    if (lm_takes(st->lm, c)) {
        for (int v = 0; v < d.nviews; v++) dn += d.vchg[2 * v], pn += d.vchg[2 * v + 1];
        for (int i = 0; i < 9; i++) {
            const double dd = st->cand[i] - st->intr[i];
            dn += dd * dd, pn += st->intr[i] * st->intr[i];
        }
    }
    if (lm_decide(st->lm, c, dn, pn))
        for (int i = 0; i < 9; i++) st->intr[i] = st->cand[i];
}

void launch_calib_init(hipStream_t s, const CalibDev& d, bool guess) {
    if (!guess) {
        hipLaunchKernelGGL(calib_homography_kernel, dim3(d.nviews), dim3(64), 0, s, d);
        hipLaunchKernelGGL(calib_focal_kernel, dim3(1), dim3(64), 0, s, d);
    }
    hipLaunchKernelGGL(calib_pose_kernel, dim3(d.nviews), dim3(64), 0, s, d);
    hipLaunchKernelGGL(calib_eval_kernel, dim3(d.nviews), dim3(64), 0, s, d, 0);
    hipLaunchKernelGGL(calib_update_kernel, dim3(1), dim3(64), 0, s, d, 0);
}

void launch_calib_iteration(hipStream_t s, const CalibDev& d) {
    hipLaunchKernelGGL(calib_normal_kernel, dim3(d.nviews), dim3(64), 0, s, d);
    hipLaunchKernelGGL(calib_solve_kernel, dim3(1), dim3(128), 0, s, d);
    hipLaunchKernelGGL(calib_eval_kernel, dim3(d.nviews), dim3(64), 0, s, d, 1);
    hipLaunchKernelGGL(calib_update_kernel, dim3(1), dim3(64), 0, s, d, 1);
}

// ---- correspondences of a batch's board detections ------------------------------------------------------------------------------

// One wave per frame of the worker's last batch, the id matching and PIX scaling of board_pose_kernel: the board corners of the
// frame's board markers go to obj / img + (first + frame) * CALIB_MAX_POINTS, the counts to npt / nmark. A frame with more points
// than a slot holds gets npt = -1.
__global__ __launch_bounds__(64) void calib_gather_kernel(const arucohip_marker_t* markers, const int32_t* nmarkers, int cap_markers,
                                                          const int32_t* ids, const float* bobj, int nboard, double mpp, int first,
                                                          float* obj, float* img, int32_t* npt, int32_t* nmark) {
    const int frame = blockIdx.x;
    if (threadIdx.x != 0) return;
    const arucohip_marker_t* M = markers + (size_t)frame * cap_markers;
    const int nm = min(nmarkers[frame], cap_markers), slot0 = first + frame;
    float* o = obj + (size_t)slot0 * CALIB_MAX_POINTS * 3;
    float* q = img + (size_t)slot0 * CALIB_MAX_POINTS * 2;
    int np = 0, nk = 0;
    bool over = false;
    for (int i = 0; i < nm; i++) {
        int slot = -1;
        for (int j = 0; j < nboard; j++)
            if (ids[j] == M[i].id) {
                slot = j;
                break;
            }
        if (slot < 0) continue;
        nk++;
        if (np + 4 > CALIB_MAX_POINTS) {
            over = true;
            continue;
        }
        for (int c = 0; c < 4; c++, np++) {
            q[2 * np] = M[i].corners[2 * c], q[2 * np + 1] = M[i].corners[2 * c + 1];
            const float* b = bobj + ((size_t)slot * 4 + c) * 3;
            for (int k = 0; k < 3; k++) o[3 * np + k] = (float)(b[k] * mpp);
        }
    }
    npt[slot0] = over ? -1 : np;
    nmark[slot0] = nk;
}

void launch_calib_gather(hipStream_t s, int nframes, const Buffers& b, const BoardDef& bd, double mpp, int first, float* obj, float* img,
                         int32_t* npt, int32_t* nmark) {
    hipLaunchKernelGGL(calib_gather_kernel, dim3(nframes), dim3(64), 0, s, b.markers, b.nmarkers, b.cap_markers, bd.ids, bd.obj, bd.nboard, mpp,
                       first, obj, img, npt, nmark);
}

}  // namespace ah
