// aruco::BoardRectifier (include/aruco_hip_shim.hpp) on mock cv::Mat frames: every result is compared with the bytes of the C call with the
// same arguments on a handle of its own. Prints one "<what> equal" or "<what> DIFFER" line per check (tests/test_gpu_rectify_shim.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "aruco_hip_shim.hpp"

static cv::Mat textured(int rows, int cols, int type) {
    cv::Mat m(rows, cols, type);
    for (int r = 0; r < rows; r++)
        for (size_t c = 0; c < (size_t)cols * m.elemSize(); c++) m.data[(size_t)r * (size_t)m.step + c] = (unsigned char)(20 + (r * 7 + c * 3) % 200);
    return m;
}

// equal, and not the trivial all-zero image
static void report(const char* what, const cv::Mat& a, const std::vector<unsigned char>& b) {
    bool same = (size_t)a.rows * a.cols * a.elemSize() == b.size(), any = false;
    const size_t row = (size_t)a.cols * a.elemSize();
    for (int r = 0; same && r < a.rows; r++) {
        same = std::memcmp(a.data + (size_t)r * (size_t)a.step, b.data() + (size_t)r * row, row) == 0;
        for (size_t c = 0; c < row; c++) any = any || b[(size_t)r * row + c] != 0;
    }
    std::printf("%s %s\n", what, same && any ? "equal" : "DIFFER");
}

int main() {
    try {
        const int W = 96, H = 64;
        const float Kf[9] = {85.5f, 0, 47.25f, 0, 84.25f, 31.5f, 0, 0, 1}, Df[5] = {0.08f, -0.12f, 0.0011f, -0.0017f, 0.03f};
        aruco::CameraParameters cp(Kf, Df, 5, cv::Size(W, H));
        // a METERS board of two markers: x -0.07 .. 0.07, y -0.05 .. 0.05; 500 px per metre: a 70 x 50 window
        aruco::BoardConfiguration bc;
        bc.mInfoType = aruco::BoardConfiguration::METERS;
        const float boxes[2][4] = {{-0.07f, -0.05f, -0.03f, -0.01f}, {0.03f, 0.01f, 0.07f, 0.05f}};
        std::vector<float> obj;
        for (int k = 0; k < 2; k++) {
            const float* b = boxes[k];
            const float c[12] = {b[0], b[1], 0, b[2], b[1], 0, b[2], b[3], 0, b[0], b[3], 0};
            std::vector<cv::Point3f> pts;
            for (int j = 0; j < 4; j++) pts.push_back(cv::Point3f(c[3 * j], c[3 * j + 1], c[3 * j + 2]));
            bc.ids.push_back(10 + k), bc.objPoints.push_back(pts);
            obj.insert(obj.end(), c, c + 12);
        }
        aruco::BoardRectifier rect;
        rect.setWindow(bc, -1.f, 500.f, 0.f);
        arucohip_rectify_t win;
        if (arucohip_rectify_board_window(obj.data(), 2, ARUCOHIP_BOARD_METERS, -1.f, 500.f, 0.f, 0, &win)) return 2;
        std::printf("window %s\n", std::memcmp(&win, &rect.getWindow(), sizeof(win)) == 0 && win.out_width == 70 && win.out_height == 50 ? "equal" : "DIFFER");

        aruco::Board B;
        B.conf = bc;
        B.Rvec = cv::Mat_<double>(3, 1), B.Tvec = cv::Mat_<double>(3, 1);
        const double r[3] = {0.9, -0.2, 0.15}, t[3] = {0.004, -0.003, 0.22};
        for (int k = 0; k < 3; k++) B.Rvec(k) = r[k], B.Tvec(k) = t[k];
        arucohip_board_t ab;
        std::memset(&ab, 0, sizeof(ab));
        ab.has_pose = 1;
        for (int k = 0; k < 3; k++) ab.rvec[k] = r[k], ab.tvec[k] = t[k];
        const double M[9] = {0.9, 0.1, 4.0, -0.05, 1.1, 1.5, -1 / 400.0, -1 / 900.0, 1.0};
        cv::Mat Mm(3, 3, CV_64FC1);
        for (int i = 0; i < 9; i++) Mm.at<double>(i / 3, i % 3) = M[i];

        arucohip_handle* h = nullptr;
        if (arucohip_create(nullptr, 0, 640, 480, 1, &h)) return 3;
        for (int type : {CV_8UC3, CV_8UC1}) {
            const int ch = type == CV_8UC3 ? 3 : 1;
            const cv::Mat frame = textured(H, W, type);
            std::vector<unsigned char> want((size_t)70 * 50 * ch);
            if (arucohip_board_rectify_batch(h, frame.data, 1, W, H, ch, (size_t)frame.step, (size_t)frame.step * H, 0, &ab, 0, Kf, Df, 5, &win, want.data(),
                                             (size_t)70 * ch, (size_t)70 * 50 * ch, 0, nullptr, nullptr))
                return 4;
            report(ch == 3 ? "rectify_bgr" : "rectify_gray", rect.rectify(frame, B, cp), want);
            const std::vector<cv::Mat> both = rect.rectify(std::vector<cv::Mat>(2, frame), std::vector<aruco::Board>(2, B), cp);
            report(ch == 3 ? "rectify_vector_bgr" : "rectify_vector_gray", both.size() == 2 ? both[1] : cv::Mat(), want);
            // a board without a pose: all zero
            aruco::Board none;
            const cv::Mat z = rect.rectify(frame, none, cp);
            bool zero = z.rows == 50 && z.cols == 70;
            for (int y = 0; zero && y < z.rows; y++)
                for (size_t c = 0; c < (size_t)z.cols * z.elemSize(); c++) zero = zero && z.data[(size_t)y * (size_t)z.step + c] == 0;
            std::printf("%s %s\n", ch == 3 ? "no_pose_bgr" : "no_pose_gray", zero ? "equal" : "DIFFER");
            std::vector<unsigned char> wantw((size_t)33 * 21 * ch);
            if (arucohip_warp_plane_batch(h, frame.data, 1, W, H, ch, (size_t)frame.step, (size_t)frame.step * H, 0, M, nullptr, 0, nullptr, nullptr, 0,
                                          wantw.data(), 33, 21, (size_t)33 * ch, (size_t)33 * 21 * ch, 0))
                return 5;
            report(ch == 3 ? "warp_bgr" : "warp_gray", aruco::BoardRectifier::warpPerspectiveInverse(frame, Mm, cv::Size(33, 21)), wantw);
        }
        arucohip_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
