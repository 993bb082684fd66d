// The general start of cv::solvePnP(ITERATIVE) on one 64-lane wavefront: object points that are not all in z = 0 (a marker cube, markers
// on two walls, a printed board whose configuration is written in world coordinates). BoardDetector::detect hands such points to
// cv::solvePnP as they are (the reference's src/boarddetector.cpp:139-157), and solvePnP chooses its start from their spread:
//   a. every z == 0            : solve_pnp_planar_wave<64> as before, bit for bit (pnp_device.h).
//   b. Mc = mean(M), MM = sum (M - Mc)(M - Mc)^T, eigenvalues w0 >= w1 >= w2 with eigenvectors v0, v1, v2.
//   c. w2 / w1 < 1e-3           : planar in another frame. R_tr = rows v0, v1, v2 (negated when det < 0), T_tr = -R_tr Mc; homography of the
//                                 points R_tr M + T_tr (third coordinate dropped), its (R_h, t_h); start R = R_h R_tr, t = R_h T_tr + t_h.
//   d. else, n >= 6             : direct linear transform. Rows [P, 0, -x P], [0, P, -y P] with P = (X, Y, Z, 1) and (x, y) the undistorted
//                                 normalised image point; the unit eigenvector of the smallest eigenvalue of their 12 x 12 normal matrix is
//                                 [RR | tt] (negated when det RR < 0); R = polar factor of RR, t = tt sqrt(3) / |RR|_F.
//      else                     : no pose.
// The Levenberg-Marquardt loop then runs on the original 3-D points from that start (solve_pnp_planar_wave<64, true>), never on the
// flattened ones: at the threshold the points are still 3 % out of their plane. A start that is not finite gives no pose.
//
// Only the board pose goes through here (board_solve_wave, pnp_points_kernel). Left planar-only, exactly as they were: the per-marker pose
// (G = 4), the two planar solutions (planar_device.h), calibration (non-planar views give CALIB_ERR_NONPLANAR), the ChromaticMask board
// rectangle and ChArUco. Nothing here reasons about self-occlusion: a face turned away from the camera is simply not detected.
#pragma once
#include "pnp_device.h"

namespace ah {

// LDS of the 12 x 12 eigen-solve: the normal matrix, the eigenvector accumulator and the round's six rotations. They are never per-lane
// arrays: the pose kernels sit at the 256-register limit and a run-time indexed private array would live in scratch memory.
struct Pnp3dLds {
    double A[144], V[144], cs[24];
};

// One Jacobi rotation angle: c, s of the rotation in the (p, q) plane that annihilates apq (Rutishauser's stable form)
__device__ inline void jacobi_cs(double app, double aqq, double apq, double* c, double* s) {
    *c = 1.0, *s = 0.0;
    if (apq != 0.0 && isfinite(apq)) {
        const double theta = (aqq - app) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        if (!isfinite(theta)) t = 0.0;   // apq is negligible beside the diagonal's difference
        *c = 1.0 / sqrt(t * t + 1.0);
        *s = t * *c;
    }
}

// Rotation (P, Q) of the cyclic Jacobi on a symmetric 3 x 3 held as a full matrix in registers: a <- J^T a J, v <- v J. P, Q are template
// parameters so that every index is static.
template <int P, int Q>
__device__ inline void jacobi3_rotate(double* a, double* v) {
    double c, s;
    jacobi_cs(a[P * 3 + P], a[Q * 3 + Q], a[P * 3 + Q], &c, &s);
    constexpr int O = 3 - P - Q;   // the third index
    const double app = a[P * 3 + P], aqq = a[Q * 3 + Q], apq = a[P * 3 + Q], aop = a[O * 3 + P], aoq = a[O * 3 + Q];
    a[P * 3 + P] = c * c * app - 2.0 * s * c * apq + s * s * aqq;
    a[Q * 3 + Q] = s * s * app + 2.0 * s * c * apq + c * c * aqq;
    a[P * 3 + Q] = a[Q * 3 + P] = 0.0;
    a[O * 3 + P] = a[P * 3 + O] = c * aop - s * aoq;
    a[O * 3 + Q] = a[Q * 3 + O] = s * aop + c * aoq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = v[k * 3 + P], vq = v[k * 3 + Q];
        v[k * 3 + P] = c * vp - s * vq;
        v[k * 3 + Q] = s * vp + c * vq;
    }
}

// Eigen-decomposition of a symmetric 3 x 3 (m: xx xy xz yy yz zz) on every lane redundantly: w[0] >= w[1] >= w[2], the unit eigenvectors
// are the ROWS of E. Cyclic Jacobi, at most 12 sweeps, stops when the off-diagonal part is below 1e-30 of the diagonal's squares; all
// lanes hold the same input, so the test is wave-uniform.
__device__ inline void sym3_eigen(const double* m, double* w, double* E) {
    double a[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
    double v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5], dia = a[0] * a[0] + a[4] * a[4] + a[8] * a[8];
        if (!(off > 1e-30 * dia)) break;
        jacobi3_rotate<0, 1>(a, v);
        jacobi3_rotate<0, 2>(a, v);
        jacobi3_rotate<1, 2>(a, v);
    }
    double d[3] = {a[0], a[4], a[8]};
    // descending order by three compare-exchanges on (value, column)
#define AH_SYM3_CX(I, J)                                                    \
    if (d[I] < d[J]) {                                                      \
        const double td = d[I];                                             \
        d[I] = d[J], d[J] = td;                                             \
        for (int k = 0; k < 3; k++) {                                       \
            const double tv = v[k * 3 + I];                                 \
            v[k * 3 + I] = v[k * 3 + J], v[k * 3 + J] = tv;                 \
        }                                                                   \
    }
    AH_SYM3_CX(0, 1)
    AH_SYM3_CX(1, 2)
    AH_SYM3_CX(0, 1)
#undef AH_SYM3_CX
    for (int i = 0; i < 3; i++) {
        w[i] = d[i];
        for (int k = 0; k < 3; k++) E[i * 3 + k] = v[k * 3 + i];
    }
}

// Round r (0 .. 10) of the round-robin order on 12 indices: six disjoint pairs, index 11 stays and the other eleven turn.
__device__ inline int jacobi12_partner(int i, int r) {
    if (i == 11) return r;
    if (i == r) return 11;
    int p = 2 * r - i;
    p += p < 0 ? 11 : 0;
    p -= p >= 11 ? 11 : 0;
    return p;
}

// Eigen-decomposition of the symmetric 12 x 12 in w.A by cyclic Jacobi, the six disjoint rotations of a round spread over the lanes:
// lanes 0 .. 5 work out the round's (c, s), then every lane updates its share of the upper triangle of A <- J^T A J (78 entries, written to
// both halves) and of V <- V J (144). Order and sweep cap (12) are fixed and every sum is taken in a fixed order, so the same input gives the
// same bits on every run. On return w.A's diagonal holds the eigenvalues and w.V's columns the eigenvectors. One wavefront per workgroup:
// __syncthreads orders the LDS traffic of its lanes. False: the matrix holds a value that is not finite (the test is wave-uniform).
__device__ inline bool jacobi12_wave(Pnp3dLds& w, int lane) {
    for (int e = lane; e < 144; e += 64) w.V[e] = (e / 12 == e % 12) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 12; sweep++) {
        double off = 0, dia = 0;
        for (int e = lane; e < 144; e += 64) {
            const double x = w.A[e];
            if (e / 12 == e % 12)
                dia += x * x;
            else
                off += x * x;
        }
        off = wave_sum_d<64>(off), dia = wave_sum_d<64>(dia);
        if (!isfinite(off) || !isfinite(dia)) return false;
        if (!(off > 1e-30 * dia)) break;
        for (int r = 0; r < 11; r++) {
            if (lane < 6) {
                // pair k of round r: (11, r) for k = 0, else (r + k, r - k) mod 11; p < q
                int a = lane == 0 ? 11 : r + lane, b = lane == 0 ? r : r - lane;
                a -= (a >= 11 && lane != 0) ? 11 : 0;
                b += b < 0 ? 11 : 0;
                const int p = min(a, b), q = max(a, b);
                double c, s;
                jacobi_cs(w.A[p * 12 + p], w.A[q * 12 + q], w.A[p * 12 + q], &c, &s);
                w.cs[2 * p] = c, w.cs[2 * p + 1] = -s;   // column p of J: c at p, -s at q
                w.cs[2 * q] = c, w.cs[2 * q + 1] = s;    // column q of J: c at q, +s at p
            }
            __syncthreads();
            // entry (i, j = i + d mod 12), d = 0 .. 6 (d = 6 only for i < 6): every unordered pair once
            double na[2], nv[3];
            for (int trip = 0; trip < 2; trip++) {
                const int e = lane + 64 * trip, d = e / 12, i = e - d * 12;
                na[trip] = 0;
                if (e < 84 && (d < 6 || i < 6)) {
                    int j = i + d;
                    j -= j >= 12 ? 12 : 0;
                    const int pi = jacobi12_partner(i, r), pj = jacobi12_partner(j, r);
                    const double ai = w.cs[2 * i], bi = w.cs[2 * i + 1], aj = w.cs[2 * j], bj = w.cs[2 * j + 1];
                    const double v = ai * (aj * w.A[i * 12 + j] + bj * w.A[i * 12 + pj]) + bi * (aj * w.A[pi * 12 + j] + bj * w.A[pi * 12 + pj]);
                    na[trip] = j == pi ? 0.0 : v;   // the annihilated entry is exactly zero
                }
            }
            for (int trip = 0; trip < 3; trip++) {
                const int e = lane + 64 * trip;
                nv[trip] = 0;
                if (e < 144) {
                    const int i = e / 12, j = e - i * 12, pj = jacobi12_partner(j, r);
                    nv[trip] = w.cs[2 * j] * w.V[i * 12 + j] + w.cs[2 * j + 1] * w.V[i * 12 + pj];
                }
            }
            __syncthreads();
            for (int trip = 0; trip < 2; trip++) {
                const int e = lane + 64 * trip, d = e / 12, i = e - d * 12;
                if (e < 84 && (d < 6 || i < 6)) {
                    int j = i + d;
                    j -= j >= 12 ? 12 : 0;
                    w.A[i * 12 + j] = na[trip], w.A[j * 12 + i] = na[trip];
                }
            }
            for (int trip = 0; trip < 3; trip++) {
                const int e = lane + 64 * trip;
                if (e < 144) w.V[e] = nv[trip];
            }
            __syncthreads();
        }
    }
    return true;
}

// The decomposition of a plane-to-image homography into a pose, as solve_pnp_planar_wave does it (pnp_device.h:537-549) with Mc = 0. The
// twelve lines are repeated here and not shared: taking them out of that function changes the register allocation of the pose kernels
// that do not come through this header (see the comment there).
__device__ inline void homography_pose(const double* H, double* R, double* t) {
    double h1n = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]);
    double h2n = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
    double s1 = 1. / fmax(h1n, DBL_EPSILON), s2 = 1. / fmax(h2n, DBL_EPSILON), st = 2. / fmax(h1n + h2n, DBL_EPSILON);
    double h1[3] = {H[0] * s1, H[3] * s1, H[6] * s1}, h2[3] = {H[1] * s2, H[4] * s2, H[7] * s2};
    t[0] = H[2] * st, t[1] = H[5] * st, t[2] = H[8] * st;
    double h3[3] = {h1[1] * h2[2] - h1[2] * h2[1], h1[2] * h2[0] - h1[0] * h2[2], h1[0] * h2[1] - h1[1] * h2[0]};
    double R0[9] = {h1[0], h2[0], h3[0], h1[1], h2[1], h3[1], h1[2], h2[2], h3[2]};
    double r[3];
    rodrigues_mat2vec(R0, r);
    rodrigues_vec2mat(r, R, nullptr);
}

// solvePnP(ITERATIVE) for any rigid point set. All 64 lanes of the workgroup's one wavefront call it; obj / img: n points in LDS or global
// memory; flat: 3 n floats of LDS the caller lends (the plane-frame points of branch c), w: the LDS of branch d. rvec / tvec on every lane.
__device__ __forceinline__ bool solve_pnp_wave3d(const float* obj, const float* img, int n, const CamModel& cam, double* rvec, double* tvec, int lane,
                                        float* flat, Pnp3dLds& w) {
    if (n < 4) return false;
    // a. the planar function makes the wave-uniform z test itself and returns false only for points out of z = 0
    if (solve_pnp_planar_wave<64>(obj, img, n, cam, rvec, tvec, lane)) return true;
    // b. spread of the points
    double Mc[3] = {0, 0, 0}, mm[6] = {0, 0, 0, 0, 0, 0};
    for (int i = lane; i < n; i += 64)
        for (int c = 0; c < 3; c++) Mc[c] += (double)obj[3 * i + c];
    wave_sum_arr<64>(Mc, 3);
    for (int c = 0; c < 3; c++) Mc[c] /= n;
    for (int i = lane; i < n; i += 64) {
        const double X = (double)obj[3 * i] - Mc[0], Y = (double)obj[3 * i + 1] - Mc[1], Z = (double)obj[3 * i + 2] - Mc[2];
        mm[0] += X * X, mm[1] += X * Y, mm[2] += X * Z, mm[3] += Y * Y, mm[4] += Y * Z, mm[5] += Z * Z;
    }
    wave_sum_arr<64>(mm, 6);
    double ev[3], E[9];
    sym3_eigen(mm, ev, E);
    double R[9], t[3];
    if (ev[2] / ev[1] < 1e-3) {
        // c. planar in the frame of the eigenvectors
        if (mat3_det(E) < 0)
            for (int k = 0; k < 9; k++) E[k] = -E[k];
        double Tt[3];
        for (int i = 0; i < 3; i++) Tt[i] = -(E[i * 3] * Mc[0] + E[i * 3 + 1] * Mc[1] + E[i * 3 + 2] * Mc[2]);
        for (int i = lane; i < n; i += 64) {
            const double X = obj[3 * i], Y = obj[3 * i + 1], Z = obj[3 * i + 2];
            for (int c = 0; c < 3; c++) flat[3 * i + c] = (float)(E[c * 3] * X + E[c * 3 + 1] * Y + E[c * 3 + 2] * Z + Tt[c]);
        }
        __syncthreads();
        const double zero[2] = {0, 0};
        double H[9];
        const bool hok = planar_homography_wave<64, true>(flat, img, n, cam, lane, zero, H);
        __syncthreads();   // flat may be the caller's next input
        if (!hok) return false;
        double Rh[9], th[3];
        homography_pose(H, Rh, th);
        mat3_mul(Rh, E, R);
        for (int i = 0; i < 3; i++) t[i] = Rh[i * 3] * Tt[0] + Rh[i * 3 + 1] * Tt[1] + Rh[i * 3 + 2] * Tt[2] + th[i];
    } else {
        // d. direct linear transform on the points centred on Mc and scaled to a unit mean square radius (conditioning; mapped back below)
        if (n < 6) return false;
        const double sc = 1.0 / sqrt((mm[0] + mm[3] + mm[5]) / n);
        double S[40];
        for (int k = 0; k < 40; k++) S[k] = 0;
        for (int i = lane; i < n; i += 64) {
            double x, y;
            undistort_point(img[2 * i], img[2 * i + 1], cam.K, cam.k, &x, &y);
            const double P[4] = {((double)obj[3 * i] - Mc[0]) * sc, ((double)obj[3 * i + 1] - Mc[1]) * sc, ((double)obj[3 * i + 2] - Mc[2]) * sc, 1.0};
            const double q = x * x + y * y;
            int k = 0;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = a; b < 4; b++, k++) {
                    const double pp = P[a] * P[b];
                    S[k] += pp, S[10 + k] += x * pp, S[20 + k] += y * pp, S[30 + k] += q * pp;
                }
        }
        wave_sum_arr<64>(S, 40);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 40; k++) w.V[k] = S[k];
        }
        __syncthreads();
        // normal matrix [[A, 0, -Ax], [0, A, -Ay], [-Ax, -Ay, Axx+yy]] from the 4 x 10 sums
        for (int e = lane; e < 144; e += 64) {
            const int i = e / 12, j = e - i * 12, bi = i >> 2, bj = j >> 2, a = min(i & 3, j & 3), b = max(i & 3, j & 3);
            const int k = a * 4 - a * (a - 1) / 2 + (b - a);   // index of (a, b), a <= b, in the packed upper triangle
            double v = 0;
            if (bi == bj) v = w.V[(bi == 2 ? 30 : 0) + k];
            else if (bi == 2 || bj == 2) v = -w.V[(min(bi, bj) == 0 ? 10 : 20) + k];
            w.A[e] = v;
        }
        __syncthreads();
        if (!jacobi12_wave(w, lane)) return false;   // a corner or an object point that is not a number
        int jm = 0;
        double best = w.A[0];
        for (int j = 1; j < 12; j++) {
            const double dj = w.A[j * 13];
            if (dj < best) best = dj, jm = j;
        }
        double RR[9], tt[3];
        for (int i = 0; i < 3; i++) {
            for (int c = 0; c < 3; c++) RR[i * 3 + c] = w.V[(i * 4 + c) * 12 + jm];
            tt[i] = w.V[(i * 4 + 3) * 12 + jm];
        }
        __syncthreads();   // w is free for the caller's next solve
        double sgn = mat3_det(RR) < 0 ? -1.0 : 1.0, fro = 0;
        for (int k = 0; k < 9; k++) RR[k] *= sgn, fro += RR[k] * RR[k];
        // [RR | tt] = lambda [R / sc | R Mc + t] for the centred, scaled points: lambda = |RR|_F sc / sqrt(3)
        const double lam = sqrt(fro) * sc / sqrt(3.0);
        for (int k = 0; k < 9; k++) R[k] = RR[k] * (sqrt(3.0) / sqrt(fro));   // singular values about 1: the Newton iteration starts close
        orthonormalise(R);                                                      // the polar factor U V^T
        for (int i = 0; i < 3; i++) t[i] = sgn * tt[i] / lam - (R[i * 3] * Mc[0] + R[i * 3 + 1] * Mc[1] + R[i * 3 + 2] * Mc[2]);
    }
    double r[3];
    rodrigues_mat2vec(R, r);
    bool fin = true;
    for (int i = 0; i < 3; i++) fin = fin && isfinite(r[i]) && isfinite(t[i]);
    if (!fin) return false;
    for (int i = 0; i < 3; i++) rvec[i] = r[i], tvec[i] = t[i];
    solve_pnp_planar_wave<64, true>(obj, img, n, cam, rvec, tvec, lane);
    for (int i = 0; i < 3; i++) fin = fin && isfinite(rvec[i]) && isfinite(tvec[i]);
    return fin;
}

}  // namespace ah
