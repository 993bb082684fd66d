// cv::calibrateCamera through the shim (no OpenCV) on correspondences generated here, then CameraParameters::saveToFile and
// readFromXMLFile. Usage: shim_calib <out.yml>. Prints: rms, K (9), dist (5) from the calibration; K (9), dist (5), w h of the
// in-memory CameraParameters; K (9), dist (5), w h read back from the file.
#include <cmath>
#include <cstdio>

#include "aruco_hip_shim.hpp"

static void project(const double K[9], const double d[5], const double r[3], const double t[3], const cv::Point3f& P, cv::Point2f* out) {
    const double th = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0) {
        const double k[3] = {r[0] / th, r[1] / th, r[2] / th}, c = std::cos(th), s = std::sin(th);
        const double X[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
        for (int i = 0; i < 9; i++) R[i] = c * (i % 4 == 0) + (1 - c) * k[i / 3] * k[i % 3] + s * X[i];
    }
    const double X = R[0] * P.x + R[1] * P.y + R[2] * P.z + t[0], Y = R[3] * P.x + R[4] * P.y + R[5] * P.z + t[1],
                 Z = R[6] * P.x + R[7] * P.y + R[8] * P.z + t[2];
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y, cd = 1 + d[0] * r2 + d[1] * r2 * r2 + d[4] * r2 * r2 * r2;
    const double xd = x * cd + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x), yd = y * cd + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y;
    *out = cv::Point2f((float)(K[0] * xd + K[2]), (float)(K[4] * yd + K[5]));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const double K[9] = {1400, 0, 965, 0, 1390, 535, 0, 0, 1}, d[5] = {-0.12, 0.05, 1e-3, -8e-4, 0.01};
    std::vector<std::vector<cv::Point3f> > objV;
    std::vector<std::vector<cv::Point2f> > imgV;
    for (int v = 0; v < 20; v++) {
        const double r[3] = {0.4 * std::sin(v * 1.3), 0.4 * std::cos(v * 0.7), 0.12 * std::sin(v * 2.1)};
        const double t[3] = {-0.1 + 0.02 * (v % 3), -0.14 + 0.015 * (v % 4), 0.55 + 0.05 * (v % 5)};
        std::vector<cv::Point3f> o;
        std::vector<cv::Point2f> m;
        for (int j = 0; j < 12; j++)
            for (int i = 0; i < 8; i++) {
                o.push_back(cv::Point3f(0.025f * i, 0.025f * j, 0.f));
                cv::Point2f p;
                project(K, d, r, t, o.back(), &p);
                m.push_back(p);
            }
        objV.push_back(o), imgV.push_back(m);
    }
    cv::Mat Km, Dm;
    std::vector<cv::Mat> rvecs, tvecs;
    double rms;
    try {
        rms = cv::calibrateCamera(objV, imgV, cv::Size(1920, 1080), Km, Dm, rvecs, tvecs, 0);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    if (rvecs.size() != objV.size() || tvecs.size() != objV.size()) return 3;
    std::printf("%.17g\n", rms);
    for (int i = 0; i < 9; i++) std::printf("%.17g%c", Km.at<double>(i / 3, i % 3), i == 8 ? '\n' : ' ');
    for (int i = 0; i < 5; i++) std::printf("%.17g%c", Dm.at<double>(0, i), i == 4 ? '\n' : ' ');
    float Kf[9], Df[5];
    for (int i = 0; i < 9; i++) Kf[i] = (float)Km.at<double>(i / 3, i % 3);
    for (int i = 0; i < 5; i++) Df[i] = (float)Dm.at<double>(0, i);
    aruco::CameraParameters cp(Kf, Df, 5, cv::Size(1920, 1080)), back;
    cp.saveToFile(argv[1]);
    back.readFromXMLFile(argv[1]);
    for (const aruco::CameraParameters* c : {&cp, &back}) {
        for (int i = 0; i < 9; i++) std::printf("%.17g ", (double)c->CameraMatrix(i / 3, i % 3));
        for (int i = 0; i < 5; i++) std::printf("%.17g ", (double)c->Distorsion(i));
        std::printf("%d %d\n", c->CamSize.width, c->CamSize.height);
    }
    return 0;
}
