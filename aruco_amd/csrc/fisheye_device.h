// The equidistant fisheye model as cv::fisheye writes it, in double precision: the one copy the point kernels, the marker kernel and
// the map kernel of k_fisheye.hip use.
//   forward: r = hypot(X, Y), theta = atan2(r, Z), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
//            pixel = (fx X theta_d / r + cx, fy Y theta_d / r + cy), the principal point when r = 0. No skew.
//   inverse: x = (u - cx) / fx, y = (v - cy) / fy, theta_d = hypot(x, y); 10 Newton steps on theta P(theta) - theta_d from
//            theta = theta_d; the ideal normalised point is (x, y) tan(theta) / theta_d, and (x, y) itself when theta_d = 0.
//   A pixel is valid when the residual after the last step is at most 1e-12 max(theta_d, 1), the derivative stayed positive and
//   theta <= max_angle. The residual bound is loose on purpose (a converged iteration sits near 1e-16): it catches coefficients
//   for which theta_d(theta) is not monotone up to the pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace ah {

constexpr int FISHEYE_NEWTON_STEPS = 10;
constexpr double FISHEYE_RESIDUAL = 1e-12;
constexpr double FISHEYE_DEFAULT_MAX_ANGLE = 1.4;   // radians; what a max_angle <= 0 selects

// one lens and the ideal pinhole camera its pixels are mapped to (row-major Knew and its inverse)
struct FisheyeCam {
    double fx, fy, cx, cy, k[4];
    double Knew[9], iKnew[9];
    double max_angle;
};

// theta_d = theta P(theta)
__host__ __device__ inline double fisheye_theta_d(const double k[4], double th) {
    const double t2 = th * th;
    return th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}
// d theta_d / d theta
__host__ __device__ inline double fisheye_dtheta_d(const double k[4], double th) {
    const double t2 = th * th;
    return 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])));
}

// The projection and its analytic Jacobian, written once. in = fx fy cx cy k1 k2 k3 k4; (X, Y, Z) is a camera-frame point.
// J (may be NULL): d(u, v) / d(X, Y, Z), rows u then v. dk (with J): d u / d k1..k4, then d v / d k1..k4. *m: the point (X s, Y s)
// with s = theta_d / r, so that d u / d fx = m[0], d v / d fy = m[1]. On the axis (r = 0) the pixel is the principal point and the
// derivatives are the limit's: those of (X / Z, Y / Z).
__host__ __device__ inline void fisheye_project_jac(const double* in, double X, double Y, double Z, double* u, double* v, double* theta, double* m,
                                                    double* J, double* dk) {
    const double fx = in[0], fy = in[1], cx = in[2], cy = in[3];
    const double* k = in + 4;
    const double r = hypot(X, Y), th = atan2(r, Z);
    const double thd = fisheye_theta_d(k, th);
    const double s = r > 0 ? thd / r : 0.0;
    m[0] = X * s, m[1] = Y * s;
    *u = fx * m[0] + cx, *v = fy * m[1] + cy, *theta = th;
    if (!J) return;
    if (!(r > 0)) {
        const double iz = Z != 0 ? 1. / Z : 0.0;
        J[0] = fx * iz, J[1] = 0, J[2] = 0, J[3] = 0, J[4] = fy * iz, J[5] = 0;
        for (int j = 0; j < 8; j++) dk[j] = 0;
        return;
    }
    const double ir = 1. / r, d2 = r * r + Z * Z, dthd = fisheye_dtheta_d(k, th);
    // d theta / d(X, Y, Z) and d r / d(X, Y, Z)
    const double dth[3] = {Z / d2 * (X * ir), Z / d2 * (Y * ir), -r / d2};
    const double dr[3] = {X * ir, Y * ir, 0};
    for (int q = 0; q < 3; q++) {
        const double ds = (dthd * dth[q]) * ir - thd * dr[q] * (ir * ir);
        J[q] = fx * ((q == 0 ? s : 0.0) + X * ds);
        J[3 + q] = fy * ((q == 1 ? s : 0.0) + Y * ds);
    }
    const double t2 = th * th;
    double tp = th * t2;   // theta^3, ^5, ^7, ^9
    for (int j = 0; j < 4; j++, tp *= t2) dk[j] = fx * X * (tp * ir), dk[4 + j] = fy * Y * (tp * ir);
}

// camera-frame point (X, Y, Z) -> fisheye pixel; *theta: the field angle
__host__ __device__ inline void fisheye_project(const FisheyeCam& c, double X, double Y, double Z, double* u, double* v, double* theta) {
    const double in[8] = {c.fx, c.fy, c.cx, c.cy, c.k[0], c.k[1], c.k[2], c.k[3]};
    double m[2];
    fisheye_project_jac(in, X, Y, Z, u, v, theta, m, nullptr, nullptr);
}

// The solver's form of the projection (the signature of pnp_device.h's project_point_d): a board point through the pose (R, t) and the
// intrinsics in[0..7] (in[8] is not used: its column is zero); optional rows d / d(intrinsics) (2 x 9) and d / d(rvec, tvec) (2 x 6).
__host__ __device__ inline void fisheye_project_point_d(double X, double Y, double Z, const double* R, const double* dRdr, const double* t,
                                                        const double* in, double* mx, double* my, double* di, double* dp) {
    const double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    const double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    double th, m[2], J[6], dk[8];
    fisheye_project_jac(in, x, y, z, mx, my, &th, m, di ? J : nullptr, dk);
    if (!di) return;
    const double dx[9] = {m[0], 0, 1, 0, dk[0], dk[1], dk[2], dk[3], 0};
    const double dy[9] = {0, m[1], 0, 1, dk[4], dk[5], dk[6], dk[7], 0};
    for (int j = 0; j < 9; j++) di[j] = dx[j], di[9 + j] = dy[j];
    for (int j = 0; j < 6; j++) {
        double d[3];   // d(x, y, z) / d pose_j
        if (j < 3) {
            const double* D = dRdr + j * 9;
            d[0] = X * D[0] + Y * D[1] + Z * D[2], d[1] = X * D[3] + Y * D[4] + Z * D[5], d[2] = X * D[6] + Y * D[7] + Z * D[8];
        } else {
            d[0] = j == 3, d[1] = j == 4, d[2] = j == 5;
        }
        dp[j] = J[0] * d[0] + J[1] * d[1] + J[2] * d[2];
        dp[6 + j] = J[3] * d[0] + J[4] * d[1] + J[5] * d[2];
    }
}

// theta with theta P(theta) = theta_d: 10 Newton steps from theta_d; *rising = false when the derivative did not stay positive
__host__ __device__ inline double fisheye_solve_theta(const double k[4], double thd, bool* rising) {
    double th = thd;
    *rising = true;
    for (int it = 0; it < FISHEYE_NEWTON_STEPS; it++) {
        const double d = fisheye_dtheta_d(k, th);
        if (!(d > 0)) {
            *rising = false;
            break;
        }
        th -= (fisheye_theta_d(k, th) - thd) / d;
    }
    return th;
}

// fisheye pixel -> ideal normalised point; false: the pixel is not valid (xn, yn are then unspecified)
__host__ __device__ inline bool fisheye_unproject(const FisheyeCam& c, double u, double v, double* xn, double* yn) {
    const double x = (u - c.cx) / c.fx, y = (v - c.cy) / c.fy, thd = hypot(x, y);
    if (thd == 0) return *xn = x, *yn = y, true;
    bool rising;
    const double th = fisheye_solve_theta(c.k, thd, &rising);
    if (!rising) return false;
    const double res = fabs(fisheye_theta_d(c.k, th) - thd);
    if (!(res <= FISHEYE_RESIDUAL * fmax(thd, 1.0)) || !(th <= c.max_angle)) return false;
    const double s = tan(th) / thd;
    return *xn = x * s, *yn = y * s, true;
}

// ideal pixel under Knew -> the ray Knew^-1 (u, v, 1)
__host__ __device__ inline void fisheye_ideal_ray(const FisheyeCam& c, double u, double v, double* X, double* Y, double* Z) {
    *X = c.iKnew[0] * u + c.iKnew[1] * v + c.iKnew[2];
    *Y = c.iKnew[3] * u + c.iKnew[4] * v + c.iKnew[5];
    *Z = c.iKnew[6] * u + c.iKnew[7] * v + c.iKnew[8];
}

// ideal normalised point -> its pixel under Knew
__host__ __device__ inline void fisheye_ideal_pixel(const FisheyeCam& c, double xn, double yn, double* u, double* v) {
    const double w = c.Knew[6] * xn + c.Knew[7] * yn + c.Knew[8];
    *u = (c.Knew[0] * xn + c.Knew[1] * yn + c.Knew[2]) / w;
    *v = (c.Knew[3] * xn + c.Knew[4] * yn + c.Knew[5]) / w;
}

}  // namespace ah
