// Marker mapping: the rigid placement of every listed marker in the frame of the first one, and the board pose of every frame,
// from frames that show several of the markers. Bundle adjustment with fixed intrinsics, FP64 throughout, with the
// Schur-complement Levenberg-Marquardt of k_calib.hip (lm_device.h): there the shared unknowns are 9 intrinsics, here 6 numbers per marker.
//
// A corner k of marker m in frame f projects R_f (R_m c_k + t_m) + t_f through project_point_d. Marker 0 is the gauge (identity, no
// variable). One wave per frame does everything that touches the frame's corners (4 lanes per marker slot, 16 slots); whatever
// combines frames adds them in frame order, so the result does not depend on scheduling (no floating-point atomics).
//   start:  map_build_kernel    (per frame: the listed markers it shows -> slots; both planar solutions of each, solution 0 and q = rms1 / rms0)
//           map_edge_kernel     (per marker pair: the frame with the largest min(q_a, q_b) that shows both)
//           map_tree_kernel     (one workgroup: spanning tree from marker 0 by edge score, marker poses composed along it)
//           map_frame_kernel    (per frame: pose from its highest-q mapped marker)
//   LM:     map_normal_kernel   (per frame: a 13 x 13 Gram [J_m | J_p | r] per slot, elimination of the frame's pose)
//           map_assemble_kernel (per entry of the reduced system: sum over the frames in order of d_ab V_a - Y_a W_b^T, damping)
//           map_solve_kernel    (one workgroup: Cholesky of the reduced system in HBM, the marker step, candidate marker poses)
//           map_eval_kernel     (per frame: pose back-substitution, candidate cost)
//           map_update_kernel   (one thread: accept / reject, lambda, stopping rule)
#include <float.h>

#include "chol_device.h"
#include "internal.h"
#include "planar_device.h"

namespace ah {

constexpr int MJ = 13;                  // a Jacobian row of one slot: 6 marker columns, 6 frame-pose columns, the residual
constexpr int MG = MJ * (MJ + 1) / 2;   // 91 entries of the upper triangle of its Gram matrix
constexpr int MAP_SOLVE_THREADS = 1024;
constexpr int MAP_MAX_N = 6 * (MAP_MAX_MARKERS - 1);

__device__ inline int mg_index(int a, int b) {
    if (a > b) { const int t = a; a = b, b = t; }
    return a * MJ - a * (a - 1) / 2 + (b - a);
}

// corner k of Marker::getObjectPoints: (-,-), (-,+), (+,+), (+,-)
__device__ inline void map_corner(float half, int k, double* cx, double* cy) {
    *cx = (k < 2) ? -(double)half : (double)half;
    *cy = (k == 1 || k == 2) ? (double)half : -(double)half;
}

// ---- observations of a batch ----------------------------------------------------------------------------------------------------

// One workgroup per frame of a worker's last batch: ids and corners of its markers to the slots of frame first + frame.
__global__ __launch_bounds__(64) void map_gather_kernel(const arucohip_marker_t* markers, const int32_t* nmarkers, int cap_markers, int first,
                                                        int stride, int32_t* obs_id, float* obs_corners, int32_t* obs_cnt) {
    const int frame = blockIdx.x, g = first + frame;
    const arucohip_marker_t* M = markers + (size_t)frame * cap_markers;
    const int nm = max(min(min(nmarkers[frame], cap_markers), stride), 0);
    for (int i = threadIdx.x; i < nm; i += 64) {
        const size_t o = (size_t)g * stride + i;
        obs_id[o] = M[i].id;
        for (int c = 0; c < 8; c++) obs_corners[o * 8 + c] = M[i].corners[c];
    }
    if (threadIdx.x == 0) obs_cnt[g] = nm;
}

void launch_map_gather(hipStream_t s, int nframes, const Buffers& b, int first, int stride, int32_t* obs_id, float* obs_corners, int32_t* obs_cnt) {
    hipLaunchKernelGGL(map_gather_kernel, dim3(nframes), dim3(64), 0, s, (const arucohip_marker_t*)b.markers, (const int32_t*)b.nmarkers, b.cap_markers,
                       first, stride, obs_id, obs_corners, obs_cnt);
}

// ---- start values ------------------------------------------------------------------------------------------------------------------

// Per frame. The frame's observations of listed ids in detection order, the first of a repeated id; more than MAP_SLOTS keep the
// MAP_SLOTS with the largest quad perimeter (an equal perimeter: the earlier one), still in detection order. Each kept marker gets
// both planar solutions (no refinement); one the method cannot solve is dropped. used[f]: the frame lists >= max(min_markers, 2)
// markers and at least two are kept.
__global__ __launch_bounds__(64) void map_build_kernel(MapDev d, CamModel cam) {
    __shared__ int s_m[64], s_o[64], s_keep[MAP_SLOTS];
    __shared__ double s_per[64];
    __shared__ float s_obj[MAP_SLOTS][12], s_img[MAP_SLOTS][8];
    const int f = blockIdx.x, lane = threadIdx.x;
    int lo = 0, hi = d.nobs;
    if (!d.obs_frame) lo = f * d.obs_stride, hi = lo + max(min(d.obs_cnt[f], d.obs_stride), 0);
    const int n = listed_scan(d.obs_frame, f, d.obs_id, lo, hi, d.ids, d.nboard, lane, s_m, s_o);   // n <= nboard <= 64
    d.slot[(size_t)f * MAP_MAX_MARKERS + lane] = -1;
    __syncthreads();
    if (lane < n) {
        const float* c = d.obs_corners + (size_t)s_o[lane] * 8;
        double per = 0;
        for (int k = 0; k < 4; k++) {
            const double dx = (double)c[2 * k] - (double)c[2 * ((k + 1) & 3)], dy = (double)c[2 * k + 1] - (double)c[2 * ((k + 1) & 3) + 1];
            per += sqrt(dx * dx + dy * dy);
        }
        s_per[lane] = per;
    }
    __syncthreads();
    bool keep = lane < n;
    if (keep && n > MAP_SLOTS) {
        int rank = 0;
        for (int k = 0; k < n; k++) rank += (s_per[k] > s_per[lane] || (s_per[k] == s_per[lane] && k < lane)) ? 1 : 0;
        keep = rank < MAP_SLOTS;
    }
    const unsigned long long kmask = __ballot(keep);
    const int nk = __popcll(kmask);   // <= MAP_SLOTS
    if (keep) s_keep[__popcll(kmask & ((1ull << lane) - 1))] = lane;
    __syncthreads();
    const int grp = lane >> 2, sub = lane & 3;
    if (grp < nk) {
        const float* c = d.obs_corners + (size_t)s_o[s_keep[grp]] * 8;
        double cx, cy;
        map_corner(d.half, sub, &cx, &cy);
        s_obj[grp][3 * sub] = (float)cx, s_obj[grp][3 * sub + 1] = (float)cy, s_obj[grp][3 * sub + 2] = 0.f;
        s_img[grp][2 * sub] = c[2 * sub], s_img[grp][2 * sub + 1] = c[2 * sub + 1];
    }
    __syncthreads();
    double r0[3] = {0, 0, 0}, t0[3] = {0, 0, 0}, r1[3] = {0, 0, 0}, t1[3] = {0, 0, 0}, rms[2] = {0, 0};
    int ns = 0;
    if (grp < nk) ns = planar_poses_wave<4>(s_obj[grp], s_img[grp], 4, cam, sub, false, r0, t0, r1, t1, rms);   // uniform in the group of four
    const unsigned long long vmask = __ballot(ns == 2 && sub == 0);
    const int nv = __popcll(vmask);
    if (ns == 2 && sub == 0) {
        const int s = __popcll(vmask & ((1ull << lane) - 1)), b = s_m[s_keep[grp]];
        const size_t fs = (size_t)f * MAP_SLOTS + s;
        d.fm[fs] = (int8_t)b;
        d.slot[(size_t)f * MAP_MAX_MARKERS + b] = (int8_t)s;
        for (int c = 0; c < 8; c++) d.fc[fs * 8 + c] = s_img[grp][c];
        double R[9];
        rodrigues_vec2mat(r0, R, nullptr);
        for (int c = 0; c < 9; c++) d.fT[fs * 12 + c] = R[c];
        for (int c = 0; c < 3; c++) d.fT[fs * 12 + 9 + c] = t0[c];
        d.fq[fs] = rms[1] / fmax(rms[0], DBL_MIN);
    }
    if (lane == 0) {
        d.fn[f] = nv;
        d.used[f] = (n >= max(d.min_markers, 2) && nv >= 2) ? 1 : 0;
    }
}

// Per ordered marker pair (a, b): the used frame that shows both with the largest min(q_a, q_b); an equal score keeps the lower frame.
__global__ __launch_bounds__(64) void map_edge_kernel(MapDev d) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= MAP_MAX_MARKERS * MAP_MAX_MARKERS) return;
    const int a = e / MAP_MAX_MARKERS, b = e % MAP_MAX_MARKERS;
    int bf = -1;
    double bq = -1;
    if (a != b && a < d.nboard && b < d.nboard)
        for (int f = 0; f < d.nframes; f++) {
            if (!d.used[f]) continue;
            const int sa = d.slot[(size_t)f * MAP_MAX_MARKERS + a], sb = d.slot[(size_t)f * MAP_MAX_MARKERS + b];
            if (sa < 0 || sb < 0) continue;
            const double q = fmin(d.fq[(size_t)f * MAP_SLOTS + sa], d.fq[(size_t)f * MAP_SLOTS + sb]);
            if (bf < 0 || q > bq) bf = f, bq = q;
        }
    d.edge_f[e] = bf, d.edge_q[e] = bq;
}

// One workgroup, thread b = marker b. Prim's rule on the edge scores: every step maps the marker whose best edge into the mapped set
// scores highest (an equal score: the lower marker; among a marker's edges: the lower mapped marker), its pose composed along that edge:
// T_b = T_a (T_a^f)^-1 T_b^f.
__global__ __launch_bounds__(64) void map_tree_kernel(MapDev d) {
    __shared__ int s_mapped[MAP_MAX_MARKERS], s_from[MAP_MAX_MARKERS], s_stop;
    __shared__ double s_best[MAP_MAX_MARKERS], s_T[MAP_MAX_MARKERS][12];
    const int b = threadIdx.x, nb = d.nboard;
    s_mapped[b] = b == 0;
    for (int c = 0; c < 12; c++) s_T[b][c] = (c == 0 || c == 4 || c == 8) ? 1. : 0.;
    if (b == 0) s_stop = 0;
    int seen = 0;   // marker 0 in a used frame
    for (int f = b; f < d.nframes; f += 64) seen |= d.used[f] && d.slot[(size_t)f * MAP_MAX_MARKERS] >= 0;
    seen = __syncthreads_or(seen);
    for (int it = 1; it < nb && seen; it++) {
        double best = -1;
        int from = -1;
        if (b < nb && !s_mapped[b])
            for (int a = 0; a < nb; a++) {
                if (!s_mapped[a] || d.edge_f[a * MAP_MAX_MARKERS + b] < 0) continue;
                const double q = d.edge_q[a * MAP_MAX_MARKERS + b];
                if (from < 0 || q > best) best = q, from = a;
            }
        s_best[b] = best, s_from[b] = from;
        __syncthreads();
        if (b == 0) {
            int w = -1;
            for (int k = 0; k < nb; k++)
                if (s_from[k] >= 0 && (w < 0 || s_best[k] > s_best[w])) w = k;
            if (w < 0) {
                s_stop = 1;
            } else {
                const int a = s_from[w], f = d.edge_f[a * MAP_MAX_MARKERS + w];
                const double* Ta = d.fT + ((size_t)f * MAP_SLOTS + d.slot[(size_t)f * MAP_MAX_MARKERS + a]) * 12;
                const double* Tb = d.fT + ((size_t)f * MAP_SLOTS + d.slot[(size_t)f * MAP_MAX_MARKERS + w]) * 12;
                double Rr[9], tr[3];   // (T_a^f)^-1 T_b^f = [Ra^T Rb | Ra^T (tb - ta)]
                for (int i = 0; i < 3; i++) {
                    for (int j = 0; j < 3; j++) Rr[i * 3 + j] = Ta[i] * Tb[j] + Ta[3 + i] * Tb[3 + j] + Ta[6 + i] * Tb[6 + j];
                    tr[i] = Ta[i] * (Tb[9] - Ta[9]) + Ta[3 + i] * (Tb[10] - Ta[10]) + Ta[6 + i] * (Tb[11] - Ta[11]);
                }
                const double* A = s_T[a];
                double Rw[9];
                mat3_mul(A, Rr, Rw);
                for (int i = 0; i < 9; i++) s_T[w][i] = Rw[i];
                for (int i = 0; i < 3; i++) s_T[w][9 + i] = A[i * 3] * tr[0] + A[i * 3 + 1] * tr[1] + A[i * 3 + 2] * tr[2] + A[9 + i];
                s_mapped[w] = 1;
            }
        }
        __syncthreads();
        if (s_stop) break;
    }
    __syncthreads();
    if (b < nb) {
        double p[6] = {0, 0, 0, 0, 0, 0};
        if (s_mapped[b] && b > 0 && seen) {
            rodrigues_mat2vec(s_T[b], p);
            for (int i = 0; i < 3; i++) p[3 + i] = s_T[b][9 + i];
        }
        for (int i = 0; i < 6; i++) d.mpose[(size_t)b * 6 + i] = p[i], d.mpose[((size_t)nb + b) * 6 + i] = p[i];
        d.mapped[b] = (s_mapped[b] && seen) ? 1 : 0;
    }
    if (b == 0) {
        int nm = 0;
        for (int k = 0; k < nb; k++) nm += s_mapped[k];
        d.st->nmapped = seen ? nm : 0;
        if (!seen)
            d.st->lm.err |= MAP_ERR_NO_REFERENCE;
        else if (nm < 2)
            d.st->lm.err |= MAP_ERR_TOO_FEW;
    }
}

// Per frame: T_f = T_m^f T_m^-1 from its mapped marker with the highest q (an equal q: the lower slot). A frame of markers that are not
// connected to marker 0 is not used.
__global__ __launch_bounds__(64) void map_frame_kernel(MapDev d) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= d.nframes) return;
    double p[6] = {0, 0, 0, 0, 0, 0};
    if (d.used[f]) {
        int bs = -1;
        const int ns = d.fn[f];
        for (int s = 0; s < ns; s++)
            if (d.mapped[d.fm[(size_t)f * MAP_SLOTS + s]] && (bs < 0 || d.fq[(size_t)f * MAP_SLOTS + s] > d.fq[(size_t)f * MAP_SLOTS + bs])) bs = s;
        if (bs < 0) {
            d.used[f] = 0;
        } else {
            const double* T = d.fT + ((size_t)f * MAP_SLOTS + bs) * 12;
            const double* mp = d.mpose + (size_t)d.fm[(size_t)f * MAP_SLOTS + bs] * 6;
            double Rm[9], Rf[9];
            rodrigues_vec2mat(mp, Rm, nullptr);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Rf[i * 3 + j] = T[i * 3] * Rm[j * 3] + T[i * 3 + 1] * Rm[j * 3 + 1] + T[i * 3 + 2] * Rm[j * 3 + 2];   // R_mf R_m^T
            rodrigues_mat2vec(Rf, p);
            for (int i = 0; i < 3; i++) p[3 + i] = T[9 + i] - (Rf[i * 3] * mp[3] + Rf[i * 3 + 1] * mp[4] + Rf[i * 3 + 2] * mp[5]);
        }
    }
    for (int i = 0; i < 6; i++) d.fpose[(size_t)f * 6 + i] = p[i], d.fpose[((size_t)d.nframes + f) * 6 + i] = p[i];
}

// ---- Levenberg-Marquardt ----------------------------------------------------------------------------------------------------------

// Per used frame, lane = 4 * slot + corner. A row of the Jacobian touches its own marker's 6 columns, the frame's 6 pose columns and the
// residual, so every slot has its own 13 x 13 Gram G_s = [J_m J_p r]^T [J_m J_p r] over its 8 rows (rows in LDS, the 91 entries of a
// slot spread over the lanes, each summed over the rows in order). With U = sum_s J_p^T J_p and g_p = sum_s J_p^T r in slot order,
// U~ = U with its diagonal times (1 + lambda):
//   u = U~^-1 g_p, and per slot V = J_m^T J_m, W = J_m^T J_p, Y = W U~^-1, rec = {V, W, Y, g_m - W u}
// (one 6 x 6 solve per row of W and one for g_p, a lane each: solve_damped6). Marker 0's columns are zero.
__global__ __launch_bounds__(64) void map_normal_kernel(MapDev d) {
    __shared__ double s_j[8 * MAP_SLOTS][MJ];
    __shared__ double s_g[MAP_SLOTS][MG];
    __shared__ double s_u[6];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (!d.used[f]) return;
    const MapState* st = d.st;
    const int cur = st->lm.cur, ns = d.fn[f], s = lane >> 2, k = lane & 3;
    const double lambda = lm_lambda(st->lm.lg);
    double in[9];
    for (int i = 0; i < 9; i++) in[i] = st->intr[i];
    const double* p = d.fpose + ((size_t)cur * d.nframes + f) * 6;
    double Rf[9], dRf[27];
    rodrigues_vec2mat(p, Rf, dRf);
    if (s < ns) {
        const size_t fs = (size_t)f * MAP_SLOTS + s;
        const int m = d.fm[fs];
        const double* mp = d.mpose + ((size_t)cur * d.nboard + m) * 6;
        double Rm[9], dRm[27], cx, cy;
        rodrigues_vec2mat(mp, Rm, dRm);
        map_corner(d.half, k, &cx, &cy);
        const double X = Rm[0] * cx + Rm[1] * cy + mp[3], Y = Rm[3] * cx + Rm[4] * cy + mp[4], Z = Rm[6] * cx + Rm[7] * cy + mp[5];
        double mx, my, di[18], dp[12];
        project_point_d(X, Y, Z, Rf, dRf, p + 3, in, &mx, &my, di, dp);
        const double res[2] = {mx - (double)d.fc[fs * 8 + 2 * k], my - (double)d.fc[fs * 8 + 2 * k + 1]};
#pragma unroll
        for (int r = 0; r < 2; r++) {
            double* row = s_j[lane * 2 + r];
            double A[3];   // d pixel / d X = (d pixel / d t_f) R_f
#pragma unroll
            for (int c = 0; c < 3; c++) A[c] = dp[r * 6 + 3] * Rf[c] + dp[r * 6 + 4] * Rf[3 + c] + dp[r * 6 + 5] * Rf[6 + c];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double* dm = dRm + j * 9;
                const double v = A[0] * (dm[0] * cx + dm[1] * cy) + A[1] * (dm[3] * cx + dm[4] * cy) + A[2] * (dm[6] * cx + dm[7] * cy);
                row[j] = m ? v : 0., row[3 + j] = m ? A[j] : 0.;
            }
#pragma unroll
            for (int j = 0; j < 6; j++) row[6 + j] = dp[r * 6 + j];
            row[12] = res[r];
        }
    }
    __syncthreads();
    for (int e = lane; e < ns * MG; e += 64) {
        const int sl = e / MG;
        int q = e % MG, a = 0;
        while (q >= MJ - a) q -= MJ - a, a++;
        const int b = a + q;
        double acc = 0;
        for (int r = 0; r < 8; r++) acc += s_j[sl * 8 + r][a] * s_j[sl * 8 + r][b];
        s_g[sl][e % MG] = acc;
    }
    __syncthreads();
    double U[36], gp[6];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double v = 0;
            for (int sl = 0; sl < ns; sl++) v += s_g[sl][mg_index(6 + a, 6 + b)];
            U[a * 6 + b] = v;
        }
        double v = 0;
        for (int sl = 0; sl < ns; sl++) v += s_g[sl][mg_index(6 + a, 12)];
        gp[a] = v;
        U[a * 7] *= 1. + lambda;
    }
    for (int c = lane; c < ns * 6 + 1; c += 64) {
        const int sl = c / 6, j = c % 6;
        double bc[6];
#pragma unroll
        for (int a = 0; a < 6; a++) bc[a] = sl < ns ? s_g[sl][mg_index(j, 6 + a)] : gp[a];
        solve_damped6(U, bc, &d.st->lm.solve_failed);   // a failure: the frame's pose cannot be eliminated
        if (sl < ns) {
            double* Yrow = d.rec + ((size_t)f * MAP_SLOTS + sl) * MAP_REC + 72 + j * 6;
#pragma unroll
            for (int a = 0; a < 6; a++) Yrow[a] = bc[a];
        } else {
#pragma unroll
            for (int a = 0; a < 6; a++) s_u[a] = bc[a], d.fu[(size_t)f * 6 + a] = bc[a];
        }
    }
    __syncthreads();
    for (int e = lane; e < ns * 78; e += 64) {
        const int sl = e / 78, q = e % 78;
        double* rec = d.rec + ((size_t)f * MAP_SLOTS + sl) * MAP_REC;
        if (q < 36) {
            rec[q] = s_g[sl][mg_index(q / 6, q % 6)];
        } else if (q < 72) {
            rec[q] = s_g[sl][mg_index((q - 36) / 6, 6 + (q - 36) % 6)];
        } else {
            const int i = q - 72;
            double v = s_g[sl][mg_index(i, 12)];
            for (int a = 0; a < 6; a++) v -= s_g[sl][mg_index(i, 6 + a)] * s_u[a];
            rec[108 + i] = v;
        }
    }
}

// One thread per entry (i, j <= i) of the reduced system and per entry of its right-hand side, N = 6 (nboard - 1), marker block a =
// i / 6 + 1: the sum over the used frames, in frame order, of d_ab V_a - Y_a W_b^T where the frame shows both markers (the slot
// table says so), and of g_a - W_a u. The diagonal is damped by lambda times the block's own diagonal sum of V. A marker that is not
// mapped gets an identity row and a zero right-hand side.
__global__ __launch_bounds__(256) void map_assemble_kernel(MapDev d) {
    const int N = 6 * (d.nboard - 1);
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * (N + 1)) return;
    const int i = (int)(e / (N + 1)), j = (int)(e % (N + 1));
    if (j > i && j < N) return;
    const int a = i / 6 + 1, ia = i % 6;
    if (j == N) {
        double g = 0;
        if (d.mapped[a])
            for (int f = 0; f < d.nframes; f++) {
                if (!d.used[f]) continue;
                const int sa = d.slot[(size_t)f * MAP_MAX_MARKERS + a];
                if (sa >= 0) g += d.rec[((size_t)f * MAP_SLOTS + sa) * MAP_REC + 108 + ia];
            }
        d.delta[i] = g;
        return;
    }
    const int b = j / 6 + 1, jb = j % 6;
    if (!d.mapped[a] || !d.mapped[b]) {
        d.S[(size_t)i * N + j] = i == j ? 1. : 0.;
        return;
    }
    const double lambda = lm_lambda(d.st->lm.lg);
    double sum = 0, diag = 0;
    for (int f = 0; f < d.nframes; f++) {
        if (!d.used[f]) continue;
        const int sa = d.slot[(size_t)f * MAP_MAX_MARKERS + a], sb = d.slot[(size_t)f * MAP_MAX_MARKERS + b];
        if (sa < 0 || sb < 0) continue;
        const double* ra = d.rec + ((size_t)f * MAP_SLOTS + sa) * MAP_REC;
        const double* rb = d.rec + ((size_t)f * MAP_SLOTS + sb) * MAP_REC;
        double c = a == b ? ra[ia * 6 + jb] : 0.;
        for (int k = 0; k < 6; k++) c -= ra[72 + ia * 6 + k] * rb[36 + jb * 6 + k];
        sum += c;
        if (i == j) diag += ra[ia * 6 + ia];
    }
    d.S[(size_t)i * N + j] = i == j ? sum + lambda * diag : sum;
}

// One workgroup: the marker step from the reduced system and the candidate marker poses mpose[other] (reduced_step_block).
__global__ __launch_bounds__(MAP_SOLVE_THREADS) void map_solve_kernel(MapDev d) {
    __shared__ double s_col[MAP_MAX_N], s_b[MAP_MAX_N], s_piv;
    __shared__ int s_fail;
    reduced_step_block<MAP_SOLVE_THREADS>(d.S, d.delta, d.mpose, d.nboard - 1, &d.st->lm, s_col, s_b, &s_piv, &s_fail);
}

// Per used frame: step = 0 evaluates the cost at the current parameters into vcost[cur]; step = 1 back-substitutes the pose step
// dp = u - sum_s Y_s^T delta_m(s), writes the candidate pose to the other buffer, its cost with the candidate marker poses to
// vcost[other] and |dp|^2, |p|^2 to vchg. scost gets every slot's share of the cost.
__global__ __launch_bounds__(64) void map_eval_kernel(MapDev d, int step) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (!d.used[f]) return;
    const MapState* st = d.st;
    const int cur = st->lm.cur, dst = step ? 1 - cur : cur, ns = d.fn[f], s = lane >> 2, k = lane & 3;
    const double* p0 = d.fpose + ((size_t)cur * d.nframes + f) * 6;
    double in[9], p[6], dn = 0, pn = 0;
    for (int i = 0; i < 9; i++) in[i] = st->intr[i];
    for (int i = 0; i < 6; i++) p[i] = p0[i];
    if (step) {
        double dp[6];
        for (int a = 0; a < 6; a++) dp[a] = d.fu[(size_t)f * 6 + a];
        for (int sl = 0; sl < ns; sl++) {
            const int m = d.fm[(size_t)f * MAP_SLOTS + sl];
            if (!m) continue;
            const double* Y = d.rec + ((size_t)f * MAP_SLOTS + sl) * MAP_REC + 72;
            const double* dm = d.delta + (size_t)(m - 1) * 6;
            for (int a = 0; a < 6; a++)
                for (int j = 0; j < 6; j++) dp[a] -= Y[j * 6 + a] * dm[j];
        }
        for (int a = 0; a < 6; a++) dn += dp[a] * dp[a], pn += p[a] * p[a], p[a] -= dp[a];
    }
    double Rf[9], e2 = 0;
    rodrigues_vec2mat(p, Rf, nullptr);
    if (s < ns) {
        const size_t fs = (size_t)f * MAP_SLOTS + s;
        const double* mp = d.mpose + ((size_t)dst * d.nboard + d.fm[fs]) * 6;
        double Rm[9], cx, cy, mx, my;
        rodrigues_vec2mat(mp, Rm, nullptr);
        map_corner(d.half, k, &cx, &cy);
        const double X = Rm[0] * cx + Rm[1] * cy + mp[3], Y = Rm[3] * cx + Rm[4] * cy + mp[4], Z = Rm[6] * cx + Rm[7] * cy + mp[5];
        project_point_d(X, Y, Z, Rf, nullptr, p + 3, in, &mx, &my, nullptr, nullptr);
        const double ex = mx - (double)d.fc[fs * 8 + 2 * k], ey = my - (double)d.fc[fs * 8 + 2 * k + 1];
        e2 = ex * ex + ey * ey;
    }
    const double es = wave_sum_d<4>(e2);
    if (s < ns && k == 0) d.scost[(size_t)f * MAP_SLOTS + s] = es;
    e2 = wave_sum_d<64>(e2);
    if (lane != 0) return;
    d.vcost[(size_t)dst * d.nframes + f] = e2;
    if (step) {
        double* q = d.fpose + ((size_t)dst * d.nframes + f) * 6;
        for (int i = 0; i < 6; i++) q[i] = p[i];
        d.vchg[2 * f] = dn, d.vchg[2 * f + 1] = pn;
    }
}

// One thread: the cost over the used frames in frame order; step 0 records the start, a step decides by lm_decide.
__global__ void map_update_kernel(MapDev d, int step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    MapState* st = d.st;
    const int other = step ? 1 - st->lm.cur : st->lm.cur;
    double c = 0;
    int nu = 0, no = 0;
    for (int f = 0; f < d.nframes; f++)
        if (d.used[f]) c += d.vcost[(size_t)other * d.nframes + f], nu++, no += d.fn[f];
    if (!step) {
        st->lm.cost = c, st->nused = nu, st->nobs = no;
        if (!isfinite(c)) st->lm.err |= MAP_ERR_DEGENERATE;
        return;
    }
    double dn = st->lm.sdn, pn = st->lm.spn;
    if (lm_takes(st->lm, c))
        for (int f = 0; f < d.nframes; f++)
            if (d.used[f]) dn += d.vchg[2 * f], pn += d.vchg[2 * f + 1];
    lm_decide(st->lm, c, dn, pn);
}

// The corners of every marker in the frame of marker 0, rounded once to float; zeros for a marker that is not mapped.
__global__ __launch_bounds__(64) void map_obj_kernel(MapDev d) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= d.nboard * 4) return;
    const int m = e >> 2, k = e & 3;
    float* o = d.obj + (size_t)e * 3;
    if (!d.mapped[m]) {
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const double* mp = d.mpose + ((size_t)d.st->lm.cur * d.nboard + m) * 6;
    double Rm[9], cx, cy;
    rodrigues_vec2mat(mp, Rm, nullptr);
    map_corner(d.half, k, &cx, &cy);
    for (int c = 0; c < 3; c++) o[c] = (float)(Rm[c * 3] * cx + Rm[c * 3 + 1] * cy + mp[3 + c]);
}

void launch_map_init(hipStream_t s, const MapDev& d, const CamModel& cam) {
    hipLaunchKernelGGL(map_build_kernel, dim3(d.nframes), dim3(64), 0, s, d, cam);
    hipLaunchKernelGGL(map_edge_kernel, dim3(MAP_MAX_MARKERS * MAP_MAX_MARKERS / 64), dim3(64), 0, s, d);
    hipLaunchKernelGGL(map_tree_kernel, dim3(1), dim3(64), 0, s, d);
    hipLaunchKernelGGL(map_frame_kernel, dim3((d.nframes + 63) / 64), dim3(64), 0, s, d);
    hipLaunchKernelGGL(map_eval_kernel, dim3(d.nframes), dim3(64), 0, s, d, 0);
    hipLaunchKernelGGL(map_update_kernel, dim3(1), dim3(64), 0, s, d, 0);
}

void launch_map_iteration(hipStream_t s, const MapDev& d) {
    const long long N = 6 * (d.nboard - 1), entries = N * (N + 1);
    hipLaunchKernelGGL(map_normal_kernel, dim3(d.nframes), dim3(64), 0, s, d);
    hipLaunchKernelGGL(map_assemble_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, d);
    hipLaunchKernelGGL(map_solve_kernel, dim3(1), dim3(MAP_SOLVE_THREADS), 0, s, d);
    hipLaunchKernelGGL(map_eval_kernel, dim3(d.nframes), dim3(64), 0, s, d, 1);
    hipLaunchKernelGGL(map_update_kernel, dim3(1), dim3(64), 0, s, d, 1);
}

// the slots' costs at the accepted parameters (the last evaluation may have been a rejected candidate's) and the object points
void launch_map_finish(hipStream_t s, const MapDev& d) {
    hipLaunchKernelGGL(map_eval_kernel, dim3(d.nframes), dim3(64), 0, s, d, 0);
    hipLaunchKernelGGL(map_obj_kernel, dim3((d.nboard * 4 + 63) / 64), dim3(64), 0, s, d);
}

}  // namespace ah
