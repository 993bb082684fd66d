// Both pose solutions of a planar target: infinitesimal plane-based pose estimation (Collins and Bartoli, "Infinitesimal plane-based
// pose estimation", IJCV 2014). A plane seen under weak perspective has two poses that explain its image almost equally well; the
// homography's first-order behaviour at the plane's origin gives both in closed form. solvePnP(ITERATIVE) (pnp_device.h) lands in one
// of them, whichever basin its homography start lies in; this code reports the two, each optionally refined by the same
// Levenberg-Marquardt loop, each with its reprojection error, the smaller error first. Everything is double precision.
#pragma once
#include "pnp_device.h"

namespace ah {

// obj: centred planar points (z = 0), img: their pixels; the G lanes of a group share the points as in solve_pnp_planar_wave and
// all hold the same results. Returns the number of solutions, 2 or 0 (degenerate input; nothing is written then):
// r0 / t0 / rms[0] the solution with the smaller reprojection error (root mean square over the points, pixels, full camera model).
template <int G>
__device__ inline int planar_poses_wave(const float* obj, const float* img, int n, const CamModel& cam, int lane, bool refine, double* r0,
                                        double* t0, double* r1, double* t1, double* rms) {
    if (n < 4) return 0;
    const float* K = cam.K;
    const double* k = cam.k;
    // ---- homography plane -> normalised image (H22 = 1), inputs kept in double
    const double Mc[2] = {0, 0};
    double H[9];
    if (!planar_homography_wave<G, false>(obj, img, n, cam, lane, Mc, H)) return 0;
    // Image points on one line (a quadrilateral folded onto a segment included) leave the homography's system singular without a
    // zero spread along x or y, and rounding can keep the elimination's pivots just above 0. The points' scatter matrix says so:
    // det / (sxx syy) = 1 - rho^2 is a few DBL_EPSILON for collinear input (each product is rounded once), and 1e-12 stands for a
    // point cloud a million times longer than wide, far beyond any view a pose can be taken from.
    double su[3] = {0, 0, 0};   // sums of u, v and u^2 + v^2: the translation's normal equations below take them too
    for (int i = lane; i < n; i += G) {
        double u, v;
        undistort_point(img[2 * i], img[2 * i + 1], K, k, &u, &v);
        su[0] += u, su[1] += v, su[2] += u * u + v * v;
    }
    wave_sum_arr<G>(su, 3);
    {
        double m[3] = {0, 0, 0};
        for (int i = lane; i < n; i += G) {
            double u, v;
            undistort_point(img[2 * i], img[2 * i + 1], K, k, &u, &v);
            u -= su[0] / n, v -= su[1] / n;
            m[0] += u * u, m[1] += v * v, m[2] += u * v;
        }
        wave_sum_arr<G>(m, 3);
        if (!(m[0] * m[1] - m[2] * m[2] > 1e-12 * m[0] * m[1])) return 0;
    }
    // ---- the image of the plane's origin and the homography's Jacobian there
    const double p = H[2], q = H[5];
    const double J00 = H[0] - H[6] * p, J01 = H[1] - H[7] * p, J10 = H[3] - H[6] * q, J11 = H[4] - H[7] * q;
    // ---- Rv takes the ray (p, q, 1) onto the z axis: axis (q, -p, 0) / hypot(p, q), angle acos(1 / s)
    const double hpq = sqrt(p * p + q * q), s = sqrt(p * p + q * q + 1.);
    double Rv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (hpq > 0) {
        const double kx = q / hpq, ky = -p / hpq, c = 1. / s, sn = hpq / s, c1 = 1. - c;
        Rv[0] = c + c1 * kx * kx, Rv[1] = c1 * kx * ky, Rv[2] = sn * ky;
        Rv[3] = c1 * kx * ky, Rv[4] = c + c1 * ky * ky, Rv[5] = -sn * kx;
        Rv[6] = -sn * ky, Rv[7] = sn * kx, Rv[8] = c;
    }
    // ---- B = left 2x2 of [[1, 0, -p], [0, 1, -q]] Rv^T, A = B^-1 J, gamma = the larger singular value of A, R22 = A / gamma
    const double B00 = Rv[0] - p * Rv[2], B01 = Rv[3] - p * Rv[5], B10 = Rv[1] - q * Rv[2], B11 = Rv[4] - q * Rv[5];
    const double idet = 1. / (B00 * B11 - B01 * B10);
    const double A00 = (B11 * J00 - B01 * J10) * idet, A01 = (B11 * J01 - B01 * J11) * idet;
    const double A10 = (B00 * J10 - B10 * J00) * idet, A11 = (B00 * J11 - B10 * J01) * idet;
    const double S1 = A00 * A00 + A01 * A01 + A10 * A10 + A11 * A11;
    const double d1 = A00 * A00 + A01 * A01 - A10 * A10 - A11 * A11, d2 = A00 * A10 + A01 * A11;
    const double gamma = sqrt(0.5 * (S1 + sqrt(d1 * d1 + 4. * d2 * d2)));
    if (!(gamma > 0) || !isfinite(gamma)) return 0;
    const double ig = 1. / gamma;
    const double Q00 = A00 * ig, Q01 = A01 * ig, Q10 = A10 * ig, Q11 = A11 * ig;
    // ---- third row of the first two columns: c c^T = I - R22^T R22
    const double b00 = 1. - (Q00 * Q00 + Q10 * Q10), b11 = 1. - (Q01 * Q01 + Q11 * Q11), b01 = -(Q00 * Q01 + Q10 * Q11);
    const double c0 = sqrt(fmax(b00, 0.));
    const double c1 = b01 < 0 ? -sqrt(fmax(b11, 0.)) : sqrt(fmax(b11, 0.));
    // ---- the translation's normal equations: rows [1 0 -u], [0 1 -v] per point, the same matrix for both rotations
    bool bad = false;
    double e[2] = {0, 0};
    // one pass per sign; not unrolled, so that the refinement's code exists once and its registers are shared
#pragma nounroll
    for (int pass = 0; pass < 2; pass++) {
        const double sg = pass ? -1. : 1.;
        const double a0 = Q00, a1 = Q10, a2 = sg * c0, b0 = Q01, b1 = Q11, b2 = sg * c1;
        const double M[9] = {a0, b0, a1 * b2 - a2 * b1, a1, b1, a2 * b0 - a0 * b2, a2, b2, a0 * b1 - a1 * b0};
        double R[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[i * 3 + j] = Rv[i] * M[j] + Rv[3 + i] * M[3 + j] + Rv[6 + i] * M[6 + j];   // Rv^T M
        double rhs[3] = {0, 0, 0};
        for (int i = lane; i < n; i += G) {
            double u, v;
            undistort_point(img[2 * i], img[2 * i + 1], K, k, &u, &v);
            const double X = obj[3 * i], Y = obj[3 * i + 1];
            const double px = R[0] * X + R[1] * Y, py = R[3] * X + R[4] * Y, pz = R[6] * X + R[7] * Y;
            const double ex = u * pz - px, ey = v * pz - py;
            rhs[0] += ex, rhs[1] += ey, rhs[2] += -u * ex - v * ey;
        }
        wave_sum_arr<G>(rhs, 3);
        double N[9] = {(double)n, 0, -su[0], 0, (double)n, -su[1], -su[0], -su[1], su[2]};
        if (!solve_spd<3>(N, rhs)) bad = true;
        if (!(rhs[2] > 0) || !isfinite(rhs[0]) || !isfinite(rhs[1]) || !isfinite(rhs[2])) bad = true;
        double r[3], t[3] = {rhs[0], rhs[1], rhs[2]};
        rodrigues_mat2vec(R, r);
        if (refine && !bad) {
            double rr[3] = {r[0], r[1], r[2]}, tt[3] = {t[0], t[1], t[2]};
            solve_pnp_planar_wave<G, true>(obj, img, n, cam, rr, tt, lane);
            bool fin = true;
#pragma unroll
            for (int i = 0; i < 3; i++) fin = fin && isfinite(rr[i]) && isfinite(tt[i]);
            // a refinement that left the numbers' range keeps the analytic solution
#pragma unroll
            for (int i = 0; i < 3; i++) r[i] = fin ? rr[i] : r[i], t[i] = fin ? tt[i] : t[i];
        }
        rodrigues_vec2mat(r, R, nullptr);
        double e2 = 0;
        for (int i = lane; i < n; i += G) {
            double mx, my;
            project_point(obj[3 * i], obj[3 * i + 1], obj[3 * i + 2], R, nullptr, t, K, k, &mx, &my, nullptr, nullptr);
            const double ex = mx - (double)img[2 * i], ey = my - (double)img[2 * i + 1];
            e2 += ex * ex + ey * ey;
        }
        e2 = sqrt(wave_sum_d<G>(e2) / n);
        if (!isfinite(e2)) bad = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r0[i] = pass ? r0[i] : r[i], t0[i] = pass ? t0[i] : t[i];
            r1[i] = pass ? r[i] : r1[i], t1[i] = pass ? t[i] : t1[i];
        }
        e[0] = pass ? e[0] : e2, e[1] = pass ? e2 : e[1];
    }
    if (bad) return 0;
    const bool sw = e[1] < e[0];   // equal errors keep the sigma = +1 solution first
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double ra = r0[i], rb = r1[i], ta = t0[i], tb = t1[i];
        r0[i] = sw ? rb : ra, r1[i] = sw ? ra : rb, t0[i] = sw ? tb : ta, t1[i] = sw ? ta : tb;
    }
    rms[0] = sw ? e[1] : e[0], rms[1] = sw ? e[0] : e[1];
    return 2;
}

}  // namespace ah
