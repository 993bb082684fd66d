// The shim's drawing names. Compiled twice by tests/test_gpu_overlay_shim.py:
//   with -DARUCOHIP_SHIM_DEFINE_DRAWING  Marker::draw, Board::draw and CvDrawingUtils::draw3dAxis / draw3dCube come from the shim (the
//                                        device overlay); each result is compared with the bytes of the C call on a handle of its own;
//   without it                           the header defines neither Marker::draw nor CvDrawingUtils: this file defines both itself, which
//                                        would not compile or link otherwise.
// Prints one "<what> equal" or "<what> DIFFER" line per check.
#include <cstdio>
#include <cstring>
#include <vector>

#include "aruco_hip_shim.hpp"

#ifndef ARUCOHIP_SHIM_DEFINE_DRAWING
namespace aruco {
static int own_calls = 0;
void Marker::draw(cv::Mat&, cv::Scalar, int, bool) const { own_calls++; }
class CvDrawingUtils {
public:
    static void draw3dCube(cv::Mat&, Marker&, const CameraParameters&, bool = false) { own_calls += 10; }
};
}  // namespace aruco
#endif

static cv::Mat textured(int rows, int cols, int type) {
    cv::Mat m(rows, cols, type);
    for (int r = 0; r < rows; r++)
        for (size_t c = 0; c < (size_t)cols * m.elemSize(); c++) m.data[(size_t)r * (size_t)m.step + c] = (unsigned char)((r * 7 + c * 3) % 200);
    return m;
}

static void report(const char* what, const cv::Mat& a, const cv::Mat& b, const cv::Mat& before) {
    const size_t bytes = (size_t)a.rows * (size_t)a.step;
    const bool same = std::memcmp(a.data, b.data, bytes) == 0, changed = std::memcmp(a.data, before.data, bytes) != 0;
    std::printf("%s %s\n", what, same && changed ? "equal" : "DIFFER");
}

int main() {
    try {
        const int W = 70, H = 50;
        const float Kf[9] = {85.5f, 0, 35.25f, 0, 84.25f, 24.5f, 0, 0, 1}, Df[5] = {0.08f, -0.12f, 0.0011f, -0.0017f, 0.03f};
        aruco::CameraParameters cp(Kf, Df, 5, cv::Size(W, H));
        std::vector<cv::Point2f> corners;
        corners.push_back(cv::Point2f(14.3f, 9.8f)), corners.push_back(cv::Point2f(41.6f, 12.1f));
        corners.push_back(cv::Point2f(39.2f, 36.7f)), corners.push_back(cv::Point2f(12.9f, 33.4f));
        aruco::Marker m(corners, 219);
        m.ssize = 0.05f;
        m.Rvec = cv::Mat_<double>(3, 1), m.Tvec = cv::Mat_<double>(3, 1);
        const double r[3] = {0.31, -0.52, 0.2}, t[3] = {0.03, -0.02, 0.5137};
        for (int k = 0; k < 3; k++) m.Rvec(k) = r[k], m.Tvec(k) = t[k];
#ifndef ARUCOHIP_SHIM_DEFINE_DRAWING
        cv::Mat img = textured(H, W, CV_8UC3);
        m.draw(img, cv::Scalar(0, 0, 255), 2, true);
        aruco::CvDrawingUtils::draw3dCube(img, m, cp);
        std::printf("own definitions %d\n", aruco::own_calls);
        return 0;
#else
        arucohip_handle* h = nullptr;
        if (arucohip_create(nullptr, 0, 640, 480, 1, &h)) return 2;
        arucohip_marker_t am;
        m.to_abi(&am);
        const int32_t one = 1;
        for (int type : {CV_8UC3, CV_8UC1}) {
            const int ch = type == CV_8UC3 ? 3 : 1;
            const cv::Mat before = textured(H, W, type);
            // Marker::draw
            cv::Mat a = before.clone(), b = before.clone();
            m.draw(a, cv::Scalar(30, 200, 90), 2, true);
            const arucohip_overlay_t st = {ARUCOHIP_DRAW_OUTLINE | ARUCOHIP_DRAW_IDS, 2, {30, 200, 90, 0}};
            if (arucohip_draw_markers_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &am, 1, &one, 0, nullptr, nullptr, 0, &st)) return 3;
            report(ch == 3 ? "marker_draw_bgr" : "marker_draw_gray", a, b, before);
            // CvDrawingUtils::draw3dCube, both forms, and draw3dAxis
            for (int yp = 0; yp < 2; yp++) {
                a = before.clone(), b = before.clone();
                aruco::CvDrawingUtils::draw3dCube(a, m, cp, yp != 0);
                const arucohip_overlay_t sc = {ARUCOHIP_DRAW_CUBE | (yp ? ARUCOHIP_DRAW_Y_PERPENDICULAR : 0), 1, {0, 0, 255, 0}};
                if (arucohip_draw_markers_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &am, 1, &one, 0, Kf, Df, 5, &sc)) return 4;
                report(yp ? "cube_yperp" : "cube", a, b, before);
            }
            a = before.clone(), b = before.clone();
            aruco::CvDrawingUtils::draw3dAxis(a, m, cp);
            const arucohip_overlay_t sa = {ARUCOHIP_DRAW_AXIS, 1, {0, 0, 255, 0}};
            if (arucohip_draw_markers_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &am, 1, &one, 0, Kf, Df, 5, &sa)) return 5;
            report("axis", a, b, before);
            // a board: Board::draw = its markers, then the board's axis and cube
            aruco::Board B;
            B.push_back(m);
            B.Rvec = m.Rvec, B.Tvec = m.Tvec;
            a = before.clone(), b = before.clone();
            B.draw(a, cv::Scalar(255, 0, 0), 1, true);
            aruco::CvDrawingUtils::draw3dAxis(a, B, cp);
            aruco::CvDrawingUtils::draw3dCube(a, B, cp, true);
            const arucohip_overlay_t sb = {ARUCOHIP_DRAW_OUTLINE | ARUCOHIP_DRAW_IDS, 1, {255, 0, 0, 0}};
            arucohip_board_t ab;
            std::memset(&ab, 0, sizeof(ab));
            ab.n_markers = 1, ab.has_pose = 1;
            for (int k = 0; k < 3; k++) ab.rvec[k] = r[k], ab.tvec[k] = t[k];
            int rc = arucohip_draw_markers_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &am, 1, &one, 0, nullptr, nullptr, 0, &sb);
            rc |= arucohip_draw_boards_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &ab, 0, m.ssize, Kf, Df, 5, ARUCOHIP_DRAW_AXIS);
            rc |= arucohip_draw_boards_batch(h, b.data, 1, W, H, ch, (size_t)b.step, (size_t)b.step * H, 0, &ab, 0, m.ssize, Kf, Df, 5,
                                             ARUCOHIP_DRAW_CUBE | ARUCOHIP_DRAW_Y_PERPENDICULAR);
            if (rc) return 6;
            report("board", a, b, before);
        }
        arucohip_destroy(h);
        return 0;
#endif
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
