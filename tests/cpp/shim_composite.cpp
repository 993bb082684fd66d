// aruco::BoardCompositor (include/aruco_hip_shim.hpp) on mock cv::Mat frames: every result is compared with the bytes of the C call with
// the same arguments on a handle of its own. Prints one "<what> equal" or "<what> DIFFER" line per check (tests/test_gpu_composite_shim.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "aruco_hip_shim.hpp"

static cv::Mat textured(int rows, int cols, int type, int seed) {
    cv::Mat m(rows, cols, type);
    for (int r = 0; r < rows; r++)
        for (size_t c = 0; c < (size_t)cols * m.elemSize(); c++) m.data[(size_t)r * (size_t)m.step + c] = (unsigned char)(20 + (r * 7 + c * 3 + seed) % 200);
    return m;
}

// the rows of a, tightly packed
static std::vector<unsigned char> bytes_of(const cv::Mat& a) {
    std::vector<unsigned char> b;
    const size_t row = (size_t)a.cols * a.elemSize();
    for (int r = 0; r < a.rows; r++) b.insert(b.end(), a.data + (size_t)r * (size_t)a.step, a.data + (size_t)r * (size_t)a.step + row);
    return b;
}

// a equals want; with `changed`, want is not simply the frame as it was
static void report(const char* what, const cv::Mat& a, const std::vector<unsigned char>& want, const std::vector<unsigned char>& before, bool changed) {
    std::printf("%s %s\n", what, bytes_of(a) == want && (want != before) == changed ? "equal" : "DIFFER");
}

int main() {
    try {
        const int W = 96, H = 64, TW = 70, TH = 50;
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
        aruco::BoardCompositor comp;
        comp.setWindow(bc, -1.f, 500.f, 0.f);
        arucohip_rectify_t win;
        if (arucohip_rectify_board_window(obj.data(), 2, ARUCOHIP_BOARD_METERS, -1.f, 500.f, 0.f, 0, &win)) return 2;
        std::printf("window %s\n", std::memcmp(&win, &comp.getWindow(), sizeof(win)) == 0 && win.out_width == TW && win.out_height == TH ? "equal" : "DIFFER");

        aruco::Board B;
        B.conf = bc;
        B.Rvec = cv::Mat_<double>(3, 1), B.Tvec = cv::Mat_<double>(3, 1);
        const double r[3] = {0.9, -0.2, 0.15}, t[3] = {0.004, -0.003, 0.22};
        for (int k = 0; k < 3; k++) B.Rvec(k) = r[k], B.Tvec(k) = t[k];
        arucohip_board_t ab;
        std::memset(&ab, 0, sizeof(ab));
        ab.has_pose = 1;
        for (int k = 0; k < 3; k++) ab.rvec[k] = r[k], ab.tvec[k] = t[k];
        cv::Mat mask(H, W, CV_8UC1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) mask.data[(size_t)y * (size_t)mask.step + x] = (unsigned char)(((x >> 2) + (y >> 1)) & 1);
        const std::vector<unsigned char> mask_bytes = bytes_of(mask);

        arucohip_handle* h = nullptr;
        if (arucohip_create(nullptr, 0, 640, 480, 1, &h)) return 3;
        for (int type : {CV_8UC3, CV_8UC1}) {
            const int ch = type == CV_8UC3 ? 3 : 1;
            const cv::Mat frame = textured(H, W, type, 0);
            const std::vector<unsigned char> before = bytes_of(frame);
            // a texture with an alpha channel (its last channel runs over 20 .. 219) at opacity 200, and one without at 255
            const cv::Mat alpha = textured(TH, TW, CV_MAKETYPE(CV_8U, ch + 1), 91), solid = textured(TH, TW, type, 55);
            struct { const char* name; const cv::Mat* tex; int opacity; bool masked; } cases[3] = {
                {"paint", &solid, 255, false}, {"paint_alpha", &alpha, 200, false}, {"paint_mask", &solid, 255, true}};
            for (const auto& c : cases) {
                const arucohip_texture_t tex = {c.tex->data, TW, TH, c.tex->channels(), 0, (size_t)c.tex->step, 0, c.opacity, 0};
                std::vector<unsigned char> want = before;
                if (arucohip_board_composite_batch(h, want.data(), 1, W, H, ch, (size_t)W * ch, (size_t)W * H * ch, 0, &ab, 0, Kf, Df, 5, &win, &tex,
                                                   c.masked ? mask_bytes.data() : nullptr, 0, nullptr, nullptr))
                    return 4;
                cv::Mat got = frame.clone();
                comp.paint(got, B, cp, *c.tex, c.opacity, c.masked ? mask : cv::Mat());
                char what[64];
                std::snprintf(what, sizeof(what), "%s_%s", c.name, ch == 3 ? "bgr" : "gray");
                report(what, got, want, before, true);
            }
            std::vector<cv::Mat> both;
            both.push_back(frame.clone()), both.push_back(frame.clone());
            std::vector<unsigned char> want = before;
            const arucohip_texture_t tex = {solid.data, TW, TH, ch, 0, (size_t)solid.step, 0, 128, 0};
            if (arucohip_board_composite_batch(h, want.data(), 1, W, H, ch, (size_t)W * ch, (size_t)W * H * ch, 0, &ab, 0, Kf, Df, 5, &win, &tex, nullptr, 0, nullptr,
                                               nullptr))
                return 5;
            comp.paint(both, std::vector<aruco::Board>(2, B), cp, solid, 128);
            report(ch == 3 ? "paint_vector_bgr" : "paint_vector_gray", both[1], want, before, true);
            // a board without a pose: the frame keeps every byte
            aruco::Board none;
            cv::Mat kept = frame.clone();
            comp.paint(kept, none, cp, solid);
            report(ch == 3 ? "no_pose_bgr" : "no_pose_gray", kept, before, before, false);
        }
        arucohip_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
