// Camera rigs: where ncams cameras with fixed intrinsics stand relative to each other (camera 0 is the rig frame: identity, no
// variable), and the pose of a board in the rig frame from every camera that sees part of it at one instant. FP64 throughout, with
// the Schur-complement Levenberg-Marquardt of k_calib.hip (lm_device.h); the composition is the one of k_map.hip with the roles
// swapped: the shared block is the outer transform (the camera), the eliminated block the inner one (the board at an instant).
//
// Corner k of board marker m seen by camera c at instant t projects R_c (R_t X_mk + t_t) + t_c through project_point_d with camera c's
// intrinsics. View v = t * ncams + c. One wave does everything that touches a view's points; whatever combines views adds them in
// camera order and instants in instant order, so the result does not depend on scheduling (no floating-point atomics).
//   views:  rig_view_kernel           (per view: the board's markers it shows -> a 512-point slot in HBM, the single-camera start pose)
//   start:  rig_edge_kernel           (per camera pair: the eligible instant with the largest min(n_a, n_b) where both views count)
//           rig_tree_kernel           (one workgroup: spanning tree from camera 0 by edge score, camera transforms composed along it)
//           rig_instant_kernel        (per instant: used or not, its pose from the counted calibrated view with the most markers)
//   LM:     rig_gram_kernel           (per view: the 13 x 13 Gram [J_c | J_p | r] of its points, accumulated in registers)
//           rig_instant_solve_kernel  (per instant: U, g_p over its views in camera order, Y_c = W_c U~^-1, u, g_c - W_c u)
//           rig_assemble_kernel       (per entry of the reduced system: sum over the instants in order of d_ab V_a - Y_a W_b^T, damping)
//           rig_solve_kernel          (one workgroup: Cholesky of the reduced system, the camera step, candidate camera transforms)
//           rig_eval_kernel           (per view: pose back-substitution, candidate cost)
//           rig_update_kernel         (one thread: accept / reject, lambda, stopping rule)
//   pose:   rig_pose_kernel           (per instant one workgroup, one wave per camera: start pose and the whole LM loop on the 6 pose unknowns)
#include <float.h>

#include "board_device.h"
#include "chol_device.h"
#include "internal.h"

namespace ah {

constexpr int RIG_SOLVE_THREADS = 256;

__host__ __device__ inline int rg_index(int a, int b) {   // a <= b
    return a * RIG_J - a * (a - 1) / 2 + (b - a);
}

// ---- the composed projection, written once -------------------------------------------------------------------------------------------

// Board point X at board pose (R_t, t_t) seen through camera transform (R_c, t_c) and intrinsics `in`: the two Jacobian rows
// [d / d(r_c, t_c) | d / d(r_t, t_t) | residual]. d pixel / d(r_c, t_c) is project_point_d's own pose derivative at the rig-frame point
// P = R_t X + t_t; with A = d pixel / d P = (d pixel / d t_c) R_c the inner pose gets d / d t_t = A and d / d r_t[j] = A (dR_t / dr_j) X.
__device__ __forceinline__ void rig_rows(const float* X3, const float* x2, const double* Rt, const double* dRt, const double* tt, const double* Rc,
                                         const double* dRc, const double* tc, const double* in, double (*row)[RIG_J]) {
    const double X = X3[0], Y = X3[1], Z = X3[2];
    const double Px = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + tt[0], Py = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + tt[1],
                 Pz = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + tt[2];
    double mx, my, di[18], dp[12];
    project_point_d(Px, Py, Pz, Rc, dRc, tc, in, &mx, &my, di, dp);
    const double res[2] = {mx - (double)x2[0], my - (double)x2[1]};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        double A[3];
#pragma unroll
        for (int c = 0; c < 3; c++) A[c] = dp[r * 6 + 3] * Rc[c] + dp[r * 6 + 4] * Rc[3 + c] + dp[r * 6 + 5] * Rc[6 + c];
#pragma unroll
        for (int j = 0; j < 6; j++) row[r][j] = dp[r * 6 + j];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double* dm = dRt + j * 9;
            row[r][6 + j] = A[0] * (dm[0] * X + dm[1] * Y + dm[2] * Z) + A[1] * (dm[3] * X + dm[4] * Y + dm[5] * Z) +
                            A[2] * (dm[6] * X + dm[7] * Y + dm[8] * Z);
            row[r][9 + j] = A[j];
        }
        row[r][12] = res[r];
    }
}

// squared pixel residual of the same point
__device__ __forceinline__ double rig_residual2(const float* X3, const float* x2, const double* Rt, const double* tt, const double* Rc, const double* tc,
                                                const double* in) {
    const double X = X3[0], Y = X3[1], Z = X3[2];
    const double Px = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + tt[0], Py = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + tt[1],
                 Pz = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + tt[2];
    double mx, my;
    project_point_d(Px, Py, Pz, Rc, nullptr, tc, in, &mx, &my, nullptr, nullptr);
    const double ex = mx - (double)x2[0], ey = my - (double)x2[1];
    return ex * ex + ey * ey;
}

// ---- views ---------------------------------------------------------------------------------------------------------------------------

// Per view. The view's observations of board ids in detection order, the first of a repeated id; their corners and object points (scaled
// to metres as board_solve_wave scales them) go to the view's slot; the start pose is solve_pnp_wave3d's, as arucohip_board_detect_batch
// solves it without the reprojection filter. The view counts with >= min_markers member markers and a pose. A batch's view reads its
// own slot of gathered markers; observations given as arrays come in any order, so the wave reads every view index and keeps its own
// (views x nobs loads: fine for a calibration's views, quadratic for thousands of them, where the batch forms are the way).
__global__ __launch_bounds__(64) void rig_view_kernel(RigDev d) {
    __shared__ int s_m[RIG_MAX_BOARD], s_o[RIG_MAX_BOARD];
    __shared__ float s_obj[RIG_VIEW_POINTS * 3], s_img[RIG_VIEW_POINTS * 2], s_flat[RIG_VIEW_POINTS * 3];
    __shared__ Pnp3dLds s_w;
    const int v = blockIdx.x, lane = threadIdx.x, c = v % d.ncams;
    int lo = 0, hi = d.nobs;
    if (!d.obs_view) lo = v * d.obs_stride, hi = lo + max(min(d.obs_cnt[v], d.obs_stride), 0);
    const int n = listed_scan(d.obs_view, v, d.obs_id, lo, hi, d.bd.ids, d.bd.nboard, lane, s_m, s_o);   // n <= nboard <= RIG_MAX_BOARD
    __syncthreads();
    const double mpp = board_mpp(d.bd);
    float* pobj = d.pobj + (size_t)v * RIG_VIEW_POINTS * 3;
    float* pimg = d.pimg + (size_t)v * RIG_VIEW_POINTS * 2;
    for (int e = lane; e < n * 4; e += 64) {
        const int i = e >> 2, p = e & 3;
        const float* cn = d.obs_corners + (size_t)s_o[i] * 8;
        const float* q = d.bd.obj + ((size_t)s_m[i] * 4 + p) * 3;
        s_img[2 * e] = cn[2 * p], s_img[2 * e + 1] = cn[2 * p + 1];
        pimg[2 * e] = cn[2 * p], pimg[2 * e + 1] = cn[2 * p + 1];
        for (int k = 0; k < 3; k++) {
            const float o = (float)(q[k] * mpp);
            s_obj[3 * e + k] = o, pobj[3 * e + k] = o;
        }
    }
    __syncthreads();
    double r[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    bool ok = false;
    if (n >= 1) ok = solve_pnp_wave3d(s_obj, s_img, n * 4, d.cams[c].cam, r, t, lane, s_flat, s_w);   // n is the same on every lane
    if (lane == 0) {
        double R[9];
        rodrigues_vec2mat(r, R, nullptr);
        double* T = d.vT + (size_t)v * 12;
        for (int k = 0; k < 9; k++) T[k] = R[k];
        for (int k = 0; k < 3; k++) T[9 + k] = t[k];
        d.vn[v] = n;
        d.vok[v] = (ok && n >= d.min_markers) ? 1 : 0;
        d.vact[v] = 0;
    }
}

// ---- start values of the calibration ---------------------------------------------------------------------------------------------------

// an instant is eligible when at least two of its views count
__device__ inline bool rig_eligible(const RigDev& d, int t) {
    int cnt = 0;
    for (int c = 0; c < d.ncams; c++) cnt += d.vok[(size_t)t * d.ncams + c];
    return cnt >= 2;
}

// Per ordered camera pair (a, b): the eligible instant where both views count with the largest min(n_a, n_b); an equal score keeps
// the lower instant.
__global__ __launch_bounds__(64) void rig_edge_kernel(RigDev d) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= RIG_MAX_CAMERAS * RIG_MAX_CAMERAS) return;
    const int a = e / RIG_MAX_CAMERAS, b = e % RIG_MAX_CAMERAS;
    int bt = -1, bq = -1;
    if (a != b && a < d.ncams && b < d.ncams)
        for (int t = 0; t < d.ninstants; t++) {
            const size_t va = (size_t)t * d.ncams + a, vb = (size_t)t * d.ncams + b;
            if (!d.vok[va] || !d.vok[vb]) continue;   // two counted views: the instant is eligible
            const int q = min(d.vn[va], d.vn[vb]);
            if (bt < 0 || q > bq) bt = t, bq = q;
        }
    d.edge_t[e] = bt, d.edge_q[e] = bq;
}

// One workgroup, thread b = camera b. Prim's rule on the edge scores: every step reaches the camera whose best edge into the reached set
// scores highest (an equal score: the lower camera; among a camera's edges: the lower reached camera), its transform composed along
// that edge: T_b = V_tb V_ta^-1 T_a.
__global__ __launch_bounds__(64) void rig_tree_kernel(RigDev d) {
    __shared__ int s_reached[RIG_MAX_CAMERAS], s_from[RIG_MAX_CAMERAS], s_best[RIG_MAX_CAMERAS], s_stop;
    __shared__ double s_T[RIG_MAX_CAMERAS][12];
    const int b = threadIdx.x, nc = d.ncams;
    if (b < RIG_MAX_CAMERAS) {
        s_reached[b] = b == 0;
        s_from[b] = -1, s_best[b] = -1;
        for (int c = 0; c < 12; c++) s_T[b][c] = (c == 0 || c == 4 || c == 8) ? 1. : 0.;
    }
    if (b == 0) s_stop = 0;
    int seen = 0;   // camera 0 in an eligible instant
    for (int t = b; t < d.ninstants; t += 64) seen |= d.vok[(size_t)t * nc] && rig_eligible(d, t);
    seen = __syncthreads_or(seen);
    for (int it = 1; it < nc && seen; it++) {
        int best = -1, from = -1;
        if (b < nc && !s_reached[b])
            for (int a = 0; a < nc; a++) {
                if (!s_reached[a] || d.edge_t[a * RIG_MAX_CAMERAS + b] < 0) continue;
                const int q = d.edge_q[a * RIG_MAX_CAMERAS + b];
                if (from < 0 || q > best) best = q, from = a;
            }
        if (b < RIG_MAX_CAMERAS) s_best[b] = best, s_from[b] = from;
        __syncthreads();
        if (b == 0) {
            int w = -1;
            for (int k = 0; k < nc; k++)
                if (s_from[k] >= 0 && (w < 0 || s_best[k] > s_best[w])) w = k;
            if (w < 0) {
                s_stop = 1;
            } else {
                const int a = s_from[w], t = d.edge_t[a * RIG_MAX_CAMERAS + w];
                const double* Va = d.vT + ((size_t)t * nc + a) * 12;
                const double* Vb = d.vT + ((size_t)t * nc + w) * 12;
                double M[9];   // R_Vb R_Va^T
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) M[i * 3 + j] = Vb[i * 3] * Va[j * 3] + Vb[i * 3 + 1] * Va[j * 3 + 1] + Vb[i * 3 + 2] * Va[j * 3 + 2];
                const double* A = s_T[a];
                double Rw[9];
                mat3_mul(M, A, Rw);
                const double dt[3] = {A[9] - Va[9], A[10] - Va[10], A[11] - Va[11]};
                for (int i = 0; i < 9; i++) s_T[w][i] = Rw[i];
                for (int i = 0; i < 3; i++) s_T[w][9 + i] = M[i * 3] * dt[0] + M[i * 3 + 1] * dt[1] + M[i * 3 + 2] * dt[2] + Vb[9 + i];
                s_reached[w] = 1;
            }
        }
        __syncthreads();
        if (s_stop) break;
    }
    __syncthreads();
    if (b < nc) {
        double p[6] = {0, 0, 0, 0, 0, 0};
        if (s_reached[b] && b > 0 && seen) {
            rodrigues_mat2vec(s_T[b], p);
            for (int i = 0; i < 3; i++) p[3 + i] = s_T[b][9 + i];
        }
        for (int i = 0; i < 6; i++) d.cpose[(size_t)b * 6 + i] = p[i], d.cpose[((size_t)nc + b) * 6 + i] = p[i];
        d.calibrated[b] = (s_reached[b] && seen) ? 1 : 0;
    }
    if (b == 0) {
        int nr = 0;
        for (int k = 0; k < nc; k++) nr += s_reached[k];
        d.st->ncal = seen ? nr : 0;
        if (!seen)
            d.st->lm.err |= RIG_ERR_NO_REFERENCE;
        else if (nr < 2)
            d.st->lm.err |= RIG_ERR_TOO_FEW;
    }
}

// The views of instant t that count and belong to calibrated cameras: their number, *first the lowest such camera, p the instant's
// start pose T_c^-1 V_tc from the one with the most member markers (an equal number: the lower camera); zeros without such a view.
__device__ inline int rig_instant_start(const RigDev& d, int t, double* p, int* first) {
    const int nc = d.ncams;
    int cnt = 0, bc = -1;
    *first = -1;
    for (int c = 0; c < nc; c++) {
        const size_t v = (size_t)t * nc + c;
        if (!d.vok[v] || !d.calibrated[c]) continue;
        cnt++;
        if (*first < 0) *first = c;
        if (bc < 0 || d.vn[v] > d.vn[(size_t)t * nc + bc]) bc = c;
    }
    for (int i = 0; i < 6; i++) p[i] = 0;
    if (bc >= 0) {
        const double* V = d.vT + ((size_t)t * nc + bc) * 12;
        const double* cp = d.cpose + (size_t)bc * 6;
        double Rc[9], R[9];
        rodrigues_vec2mat(cp, Rc, nullptr);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i * 3 + j] = Rc[i] * V[j] + Rc[3 + i] * V[3 + j] + Rc[6 + i] * V[6 + j];   // R_c^T R_V
        rodrigues_mat2vec(R, p);
        for (int i = 0; i < 3; i++) p[3 + i] = Rc[i] * (V[9] - cp[3]) + Rc[3 + i] * (V[10] - cp[4]) + Rc[6 + i] * (V[11] - cp[5]);
    }
    return cnt;
}

// Per instant of the calibration: used with at least two such views, which then take part in the solve.
__global__ __launch_bounds__(64) void rig_instant_kernel(RigDev d) {
    const int t = blockIdx.x * 64 + threadIdx.x, nc = d.ncams;
    if (t >= d.ninstants) return;
    double p[6];
    int first;
    const int used = rig_instant_start(d, t, p, &first) >= 2;
    for (int c = 0; c < nc; c++) d.vact[(size_t)t * nc + c] = (used && d.vok[(size_t)t * nc + c] && d.calibrated[c]) ? 1 : 0;
    d.used[t] = used, d.lead[t] = used ? first : -1;
    for (int i = 0; i < 6; i++) {
        const double q = used ? p[i] : 0.;
        d.ipose[(size_t)t * 6 + i] = q, d.ipose[((size_t)d.ninstants + t) * 6 + i] = q;
    }
}

// ---- Levenberg-Marquardt of the calibration ----------------------------------------------------------------------------------------------

// Per view that takes part, the lanes stride over its points. Each point gives two rows of 13 numbers; a lane keeps the 91 entries of
// the upper triangle of their Gram matrix in registers, a fixed butterfly adds the lanes. Camera 0's columns are zero.
__global__ __launch_bounds__(64) void rig_gram_kernel(RigDev d) {
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!d.vact[v]) return;
    const int nc = d.ncams, t = v / nc, c = v % nc, cur = d.st->lm.cur, np = d.vn[v] * 4;
    const double* cp = d.cpose + ((size_t)cur * nc + c) * 6;
    const double* ip = d.ipose + ((size_t)cur * d.ninstants + t) * 6;
    double in[9], Rc[9], dRc[27], Rt[9], dRt[27];
    for (int i = 0; i < 9; i++) in[i] = d.cams[c].in[i];
    rodrigues_vec2mat<true>(cp, Rc, dRc);
    rodrigues_vec2mat<true>(ip, Rt, dRt);
    const float* pobj = d.pobj + (size_t)v * RIG_VIEW_POINTS * 3;
    const float* pimg = d.pimg + (size_t)v * RIG_VIEW_POINTS * 2;
    double G[RIG_G];
#pragma unroll
    for (int e = 0; e < RIG_G; e++) G[e] = 0;
    for (int i = lane; i < np; i += 64) {
        double row[2][RIG_J];
        rig_rows(pobj + 3 * i, pimg + 2 * i, Rt, dRt, ip + 3, Rc, dRc, cp + 3, in, row);
#pragma unroll
        for (int r = 0; r < 2; r++) {
#pragma unroll
            for (int j = 0; j < 6; j++) row[r][j] = c ? row[r][j] : 0.;
#pragma unroll
            for (int a = 0; a < RIG_J; a++)
#pragma unroll
                for (int b = a; b < RIG_J; b++) G[a * RIG_J - a * (a - 1) / 2 + (b - a)] += row[r][a] * row[r][b];
        }
    }
#pragma unroll
    for (int e = 0; e < RIG_G; e++) G[e] = wave_sum_d<64>(G[e]);
    if (lane == 0) {
        double* g = d.gram + (size_t)v * RIG_G;
#pragma unroll
        for (int e = 0; e < RIG_G; e++) g[e] = G[e];
    }
}

// Per used instant. U = sum_c J_p^T J_p and g_p = sum_c J_p^T r over its views in camera order, U~ = U with its diagonal times
// (1 + lambda); u = U~^-1 g_p, and per view of a camera c > 0: Y_c = W_c U~^-1 with W_c = J_c^T J_p, rec = {Y_c, g_c - W_c u} (one 6 x 6
// solve per row of W_c and one for g_p, a lane each: solve_damped6).
__global__ __launch_bounds__(64) void rig_instant_solve_kernel(RigDev d) {
    __shared__ double s_u[6];
    const int t = blockIdx.x, lane = threadIdx.x, nc = d.ncams;
    if (!d.used[t]) return;
    const double lambda = lm_lambda(d.st->lm.lg);
    double U[36], gp[6];
#pragma unroll
    for (int a = 0; a < 36; a++) U[a] = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) gp[a] = 0;
    for (int c = 0; c < nc; c++) {
        if (!d.vact[(size_t)t * nc + c]) continue;
        const double* g = d.gram + ((size_t)t * nc + c) * RIG_G;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = 0; b < 6; b++) U[a * 6 + b] += g[rg_index(6 + min(a, b), 6 + max(a, b))];
            gp[a] += g[rg_index(6 + a, 12)];
        }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) U[a * 7] *= 1. + lambda;
    for (int e = lane; e < nc * 6 + 1; e += 64) {
        const int c = e / 6, j = e % 6;
        if (c < nc && (c == 0 || !d.vact[(size_t)t * nc + c])) continue;
        const double* g = d.gram + ((size_t)t * nc + min(c, nc - 1)) * RIG_G;
        double bc[6];
#pragma unroll
        for (int a = 0; a < 6; a++) bc[a] = c < nc ? g[rg_index(j, 6 + a)] : gp[a];
        solve_damped6(U, bc, &d.st->lm.solve_failed);   // a failure: the instant's pose cannot be eliminated
        if (c < nc) {
            double* Y = d.rec + ((size_t)t * nc + c) * RIG_REC + j * 6;
#pragma unroll
            for (int a = 0; a < 6; a++) Y[a] = bc[a];
        } else {
#pragma unroll
            for (int a = 0; a < 6; a++) s_u[a] = bc[a], d.fu[(size_t)t * 6 + a] = bc[a];
        }
    }
    __syncthreads();
    for (int e = lane; e < nc * 6; e += 64) {
        const int c = e / 6, i = e % 6;
        if (c == 0 || !d.vact[(size_t)t * nc + c]) continue;
        const double* g = d.gram + ((size_t)t * nc + c) * RIG_G;
        double val = g[rg_index(i, 12)];
        for (int a = 0; a < 6; a++) val -= g[rg_index(i, 6 + a)] * s_u[a];
        d.rec[((size_t)t * nc + c) * RIG_REC + 36 + i] = val;
    }
}

// One thread per entry (i, j <= i) of the reduced system and per entry of its right-hand side, N = 6 (ncams - 1), camera a = i / 6 + 1:
// the sum over the used instants, in instant order, of d_ab V_a - Y_a W_b^T where both cameras' views take part, and of g_a - W_a u.
// The diagonal is damped by lambda times the block's own diagonal sum of V. A camera that is not calibrated gets an identity row and
// a zero right-hand side.
__global__ __launch_bounds__(256) void rig_assemble_kernel(RigDev d) {
    const int nc = d.ncams, N = 6 * (nc - 1);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * (N + 1)) return;
    const int i = e / (N + 1), j = e % (N + 1);
    if (j > i && j < N) return;
    const int a = i / 6 + 1, ia = i % 6;
    if (j == N) {
        double g = 0;
        if (d.calibrated[a])
            for (int t = 0; t < d.ninstants; t++)
                if (d.vact[(size_t)t * nc + a]) g += d.rec[((size_t)t * nc + a) * RIG_REC + 36 + ia];
        d.delta[i] = g;
        return;
    }
    const int b = j / 6 + 1, jb = j % 6;
    if (!d.calibrated[a] || !d.calibrated[b]) {
        d.S[(size_t)i * N + j] = i == j ? 1. : 0.;
        return;
    }
    const double lambda = lm_lambda(d.st->lm.lg);
    double sum = 0, diag = 0;
    for (int t = 0; t < d.ninstants; t++) {
        const size_t va = (size_t)t * nc + a, vb = (size_t)t * nc + b;
        if (!d.vact[va] || !d.vact[vb]) continue;
        const double* ga = d.gram + va * RIG_G;
        const double* gb = d.gram + vb * RIG_G;
        const double* Y = d.rec + va * RIG_REC + ia * 6;
        double c = a == b ? ga[rg_index(min(ia, jb), max(ia, jb))] : 0.;
        for (int k = 0; k < 6; k++) c -= Y[k] * gb[rg_index(jb, 6 + k)];
        sum += c;
        if (i == j) diag += ga[rg_index(ia, ia)];
    }
    d.S[(size_t)i * N + j] = i == j ? sum + lambda * diag : sum;
}

// One workgroup: the camera step from the reduced system and the candidate camera transforms cpose[other] (reduced_step_block).
__global__ __launch_bounds__(RIG_SOLVE_THREADS) void rig_solve_kernel(RigDev d) {
    __shared__ double s_col[RIG_MAX_N], s_b[RIG_MAX_N], s_piv;
    __shared__ int s_fail;
    reduced_step_block<RIG_SOLVE_THREADS>(d.S, d.delta, d.cpose, d.ncams - 1, &d.st->lm, s_col, s_b, &s_piv, &s_fail);
}

// Per view that takes part: step = 0 evaluates the cost at the current parameters into vcost[cur]; step = 1 back-substitutes the
// instant's pose step dp = u - sum_c Y_c^T delta_c (every view of the instant computes the same), evaluates the candidate pose with the
// candidate camera transforms into vcost[other]; the instant's leading view writes the candidate pose and |dp|^2, |p|^2 to vchg.
__global__ __launch_bounds__(64) void rig_eval_kernel(RigDev d, int step) {
    const int v = blockIdx.x, lane = threadIdx.x;
    if (!d.vact[v]) return;
    const int nc = d.ncams, t = v / nc, c = v % nc, cur = d.st->lm.cur, dst = step ? 1 - cur : cur, np = d.vn[v] * 4;
    const double* p0 = d.ipose + ((size_t)cur * d.ninstants + t) * 6;
    const double* cp = d.cpose + ((size_t)dst * nc + c) * 6;
    double in[9], p[6], dn = 0, pn = 0;
    for (int i = 0; i < 9; i++) in[i] = d.cams[c].in[i];
    for (int i = 0; i < 6; i++) p[i] = p0[i];
    if (step) {
        double dp[6];
        for (int a = 0; a < 6; a++) dp[a] = d.fu[(size_t)t * 6 + a];
        for (int k = 1; k < nc; k++) {
            if (!d.vact[(size_t)t * nc + k]) continue;
            const double* Y = d.rec + ((size_t)t * nc + k) * RIG_REC;
            const double* dc = d.delta + (size_t)(k - 1) * 6;
            for (int a = 0; a < 6; a++)
                for (int j = 0; j < 6; j++) dp[a] -= Y[j * 6 + a] * dc[j];
        }
        for (int a = 0; a < 6; a++) dn += dp[a] * dp[a], pn += p[a] * p[a], p[a] -= dp[a];
    }
    double Rt[9], Rc[9], e2 = 0;
    rodrigues_vec2mat(p, Rt, nullptr);
    rodrigues_vec2mat(cp, Rc, nullptr);
    const float* pobj = d.pobj + (size_t)v * RIG_VIEW_POINTS * 3;
    const float* pimg = d.pimg + (size_t)v * RIG_VIEW_POINTS * 2;
    for (int i = lane; i < np; i += 64) e2 += rig_residual2(pobj + 3 * i, pimg + 2 * i, Rt, p + 3, Rc, cp + 3, in);
    e2 = wave_sum_d<64>(e2);
    if (lane != 0) return;
    d.vcost[(size_t)dst * d.ninstants * nc + v] = e2;
    if (step && c == d.lead[t]) {
        double* q = d.ipose + ((size_t)dst * d.ninstants + t) * 6;
        for (int i = 0; i < 6; i++) q[i] = p[i];
        d.vchg[2 * t] = dn, d.vchg[2 * t + 1] = pn;
    }
}

// One thread: the cost over the views that take part, in view order (instants in order, cameras in order); step 0 records the
// start, a step decides by lm_decide.
__global__ void rig_update_kernel(RigDev d, int step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RigState* st = d.st;
    const int other = step ? 1 - st->lm.cur : st->lm.cur, V = d.ninstants * d.ncams;
    double c = 0;
    int np = 0, nu = 0;
    for (int v = 0; v < V; v++)
        if (d.vact[v]) c += d.vcost[(size_t)other * V + v], np += d.vn[v] * 4;
    for (int t = 0; t < d.ninstants; t++) nu += d.used[t];
    if (!step) {
        st->lm.cost = c, st->nused = nu, st->npts = np;
        if (!isfinite(c) || nu < 1) st->lm.err |= RIG_ERR_DEGENERATE;
        return;
    }
    double dn = st->lm.sdn, pn = st->lm.spn;
    if (lm_takes(st->lm, c))
        for (int t = 0; t < d.ninstants; t++)
            if (d.used[t]) dn += d.vchg[2 * t], pn += d.vchg[2 * t + 1];
    lm_decide(st->lm, c, dn, pn);
}

// ---- rig pose --------------------------------------------------------------------------------------------------------------------------

// One workgroup per instant, wave c = camera c. An instant has a pose when at least one of its views counts and belongs to a calibrated
// camera; the start is rig_instant_start's. NW: the waves the launch bound allows (the block itself has ncams waves). Every wave
// adds the pose columns' Gram (21 + 6 numbers) or the cost of its view's points, lane 0 leaves the wave's sum in LDS, and every thread
// adds the waves in camera order and runs the same 6 x 6 damped solve and the same accept / stop rule as the calibration, so the whole
// workgroup walks through the loop together.
template <int NW>
__global__ __launch_bounds__(NW * 64) void rig_pose_kernel(RigDev d) {
    __shared__ double s_acc[NW][28];
    __shared__ int s_act[NW];
    const int t = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63, nc = d.ncams;
    const int v = t * nc + c;
    double p[6];
    int first;
    if (rig_instant_start(d, t, p, &first) < 1) {   // the same on every thread
        if (threadIdx.x == 0) {
            arucohip_board_t o{};
            d.boards[t] = o;
            d.views_used[t] = 0;
        }
        return;
    }
    const bool act = d.vok[v] && d.calibrated[c];
    const int np = act ? d.vn[v] * 4 : 0;
    if (lane == 0) s_act[c] = act ? d.vn[v] : 0;
    const double* cp = d.cpose + (size_t)c * 6;
    double in[9], Rc[9], dRc[27];
    for (int i = 0; i < 9; i++) in[i] = d.cams[c].in[i];
    rodrigues_vec2mat<true>(cp, Rc, dRc);
    const float* pobj = d.pobj + (size_t)v * RIG_VIEW_POINTS * 3;
    const float* pimg = d.pimg + (size_t)v * RIG_VIEW_POINTS * 2;

    // the cost at pose q, on every thread
    auto cost_at = [&](const double* q) {
        double Rt[9], e2 = 0;
        rodrigues_vec2mat(q, Rt, nullptr);
        for (int i = lane; i < np; i += 64) e2 += rig_residual2(pobj + 3 * i, pimg + 2 * i, Rt, q + 3, Rc, cp + 3, in);
        e2 = wave_sum_d<64>(e2);
        if (lane == 0) s_acc[c][27] = e2;
        __syncthreads();
        double sum = 0;
        for (int k = 0; k < nc; k++) sum += s_acc[k][27];
        __syncthreads();
        return sum;
    };

    double cost = cost_at(p), U[21], g[6];
    bool good = isfinite(cost), fresh = true;
    int lg = -3, iters = 0;
    for (int attempt = 0; attempt < 256 && good; attempt++) {
        if (fresh) {
            double Rt[9], dRt[27], acc[27];
            rodrigues_vec2mat<true>(p, Rt, dRt);
#pragma unroll
            for (int e = 0; e < 27; e++) acc[e] = 0;
            for (int i = lane; i < np; i += 64) {
                double row[2][RIG_J];
                rig_rows(pobj + 3 * i, pimg + 2 * i, Rt, dRt, p + 3, Rc, dRc, cp + 3, in, row);
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int a = 0; a < 6; a++) {
#pragma unroll
                        for (int b = a; b < 6; b++) acc[a * 6 - a * (a - 1) / 2 + (b - a)] += row[r][6 + a] * row[r][6 + b];
                        acc[21 + a] += row[r][6 + a] * row[r][12];
                    }
            }
#pragma unroll
            for (int e = 0; e < 27; e++) acc[e] = wave_sum_d<64>(acc[e]);
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < 27; e++) s_acc[c][e] = acc[e];
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 21; e++) U[e] = 0;
#pragma unroll
            for (int e = 0; e < 6; e++) g[e] = 0;
            for (int k = 0; k < nc; k++) {
#pragma unroll
                for (int e = 0; e < 21; e++) U[e] += s_acc[k][e];
#pragma unroll
                for (int e = 0; e < 6; e++) g[e] += s_acc[k][21 + e];
            }
            __syncthreads();
            fresh = false;
        }
        const double lambda = lm_lambda(lg);
        double A[36], b[6], cand[6], dn = 0, pn = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int k = 0; k < 6; k++) A[a * 6 + k] = a <= k ? U[a * 6 - a * (a - 1) / 2 + (k - a)] : U[k * 6 - k * (k - 1) / 2 + (a - k)];
            b[a] = g[a];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) A[a * 7] *= 1. + lambda;
        const bool ok = solve_spd<6>(A, b);
#pragma unroll
        for (int a = 0; a < 6; a++) cand[a] = p[a] - b[a], dn += b[a] * b[a], pn += p[a] * p[a];
        const double c2 = cost_at(cand);   // every thread holds the same numbers: the branches below are uniform
        if (ok && isfinite(c2) && c2 <= cost) {
#pragma unroll
            for (int a = 0; a < 6; a++) p[a] = cand[a];
            cost = c2, fresh = true;
            lg = max(lg - 1, -16);
            if (++iters >= 30 || sqrt(dn) < DBL_EPSILON * sqrt(pn)) break;
        } else if (++lg > 16) {
            break;
        }
    }
    if (threadIdx.x == 0) {
        arucohip_board_t o{};
        int nm = 0, nv = 0;
        for (int k = 0; k < nc; k++) nm += s_act[k], nv += s_act[k] > 0;
        o.n_markers = nm, o.has_pose = good ? 1 : 0;
        for (int i = 0; i < 3; i++) o.rvec[i] = good ? p[i] : 0., o.tvec[i] = good ? p[3 + i] : 0.;
        d.boards[t] = o;
        d.views_used[t] = nv;
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------

void launch_rig_views(hipStream_t s, const RigDev& d) {
    hipLaunchKernelGGL(rig_view_kernel, dim3(d.ninstants * d.ncams), dim3(64), 0, s, d);
}

void launch_rig_calib_init(hipStream_t s, const RigDev& d) {
    hipLaunchKernelGGL(rig_edge_kernel, dim3(RIG_MAX_CAMERAS * RIG_MAX_CAMERAS / 64), dim3(64), 0, s, d);
    hipLaunchKernelGGL(rig_tree_kernel, dim3(1), dim3(64), 0, s, d);
    hipLaunchKernelGGL(rig_instant_kernel, dim3((d.ninstants + 63) / 64), dim3(64), 0, s, d);
    hipLaunchKernelGGL(rig_eval_kernel, dim3(d.ninstants * d.ncams), dim3(64), 0, s, d, 0);
    hipLaunchKernelGGL(rig_update_kernel, dim3(1), dim3(64), 0, s, d, 0);
}

void launch_rig_calib_iteration(hipStream_t s, const RigDev& d) {
    const int V = d.ninstants * d.ncams, N = 6 * (d.ncams - 1), entries = N * (N + 1);
    hipLaunchKernelGGL(rig_gram_kernel, dim3(V), dim3(64), 0, s, d);
    hipLaunchKernelGGL(rig_instant_solve_kernel, dim3(d.ninstants), dim3(64), 0, s, d);
    hipLaunchKernelGGL(rig_assemble_kernel, dim3((entries + 255) / 256), dim3(256), 0, s, d);
    hipLaunchKernelGGL(rig_solve_kernel, dim3(1), dim3(RIG_SOLVE_THREADS), 0, s, d);
    hipLaunchKernelGGL(rig_eval_kernel, dim3(V), dim3(64), 0, s, d, 1);
    hipLaunchKernelGGL(rig_update_kernel, dim3(1), dim3(64), 0, s, d, 1);
}

// the views' costs at the accepted parameters (the last evaluation may have been a rejected candidate's)
void launch_rig_calib_finish(hipStream_t s, const RigDev& d) {
    hipLaunchKernelGGL(rig_eval_kernel, dim3(d.ninstants * d.ncams), dim3(64), 0, s, d, 0);
}

// behind launch_rig_views, with d.calibrated and d.cpose[0] from the caller uploaded before the view kernel: no host round trip in between
void launch_rig_pose(hipStream_t s, const RigDev& d) {
    if (d.ncams <= 4)
        hipLaunchKernelGGL(rig_pose_kernel<4>, dim3(d.ninstants), dim3(d.ncams * 64), 0, s, d);
    else if (d.ncams <= 8)
        hipLaunchKernelGGL(rig_pose_kernel<8>, dim3(d.ninstants), dim3(d.ncams * 64), 0, s, d);
    else
        hipLaunchKernelGGL(rig_pose_kernel<16>, dim3(d.ninstants), dim3(d.ncams * 64), 0, s, d);
}

}  // namespace ah
