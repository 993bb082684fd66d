// aruco::Mesh and aruco::MeshRenderer (include/aruco_hip_shim.hpp) on mock cv::Mat frames: every result is compared with the bytes of the
// C call with the same arguments on a handle of its own. Prints one "<what> equal" or "<what> DIFFER" line per check
// (tests/test_gpu_render_shim.py).
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
    std::printf("%s_%s %s\n", what, a.elemSize() == 3 ? "bgr" : "gray", bytes_of(a) == want && (want != before) == changed ? "equal" : "DIFFER");
}

// every triangle's normal (b - a) x (c - a) points away from `centre`
static bool outward(const aruco::Mesh& m, const float centre[3]) {
    for (size_t t = 0; t < m.ntris(); t++) {
        const float *a = &m.vertices[3 * m.triangles[3 * t]], *b = &m.vertices[3 * m.triangles[3 * t + 1]], *c = &m.vertices[3 * m.triangles[3 * t + 2]];
        const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const float n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        float dot = 0;
        for (int k = 0; k < 3; k++) dot += n[k] * ((a[k] + b[k] + c[k]) / 3.f - centre[k]);
        if (!(dot > 0)) return false;
    }
    return true;
}

int main() {
    try {
        const int W = 96, H = 64;
        const float Kf[9] = {85.5f, 0, 47.25f, 0, 84.25f, 31.5f, 0, 0, 1}, Df[5] = {0.08f, -0.12f, 0.0011f, -0.0017f, 0.03f};
        aruco::CameraParameters cp(Kf, Df, 5, cv::Size(W, H));
        const float mid[3] = {0.f, 0.f, 0.5f};
        const aruco::Mesh cube = aruco::Mesh::cube();
        std::printf("cube %s\n", cube.nverts() == 8 && cube.ntris() == 12 && outward(cube, mid) ? "equal" : "DIFFER");
        aruco::Mesh sphere = aruco::Mesh::uvSphere(6, 8);
        std::printf("sphere %s\n", sphere.nverts() == 42 && sphere.ntris() == 80 && outward(sphere, mid) ? "equal" : "DIFFER");
        for (size_t t = 0; t < sphere.ntris(); t++)
            for (int k = 0; k < 3; k++) sphere.colors.push_back((unsigned char)(40 + (t * 37 + k * 90) % 200));

        // two markers with a pose and one without between them
        const double poses[3][6] = {{3.0, 0.2, -0.1, -0.05, 0.01, 0.5}, {0, 0, 0, 0, 0, 0}, {2.9, -0.3, 0.2, 0.06, -0.02, 0.6}};
        std::vector<aruco::Marker> markers;
        std::vector<arucohip_marker_t> am(3);
        std::memset(am.data(), 0, am.size() * sizeof(arucohip_marker_t));
        for (int i = 0; i < 3; i++) {
            aruco::Marker m(std::vector<cv::Point2f>(4, cv::Point2f(10.f + i, 12.f)), 5 + i);
            m.ssize = 0.08f;
            if (i != 1) {
                m.Rvec = cv::Mat_<double>(3, 1), m.Tvec = cv::Mat_<double>(3, 1);
                for (int k = 0; k < 3; k++) m.Rvec(k) = poses[i][k], m.Tvec(k) = poses[i][3 + k];
            }
            markers.push_back(m);
            m.to_abi(&am[i]);
        }
        if (!am[0].has_pose || am[1].has_pose || !am[2].has_pose) return 2;
        aruco::Board B;
        B.Rvec = cv::Mat_<double>(3, 1), B.Tvec = cv::Mat_<double>(3, 1);
        arucohip_board_t ab;
        std::memset(&ab, 0, sizeof(ab));
        ab.has_pose = 1;
        for (int k = 0; k < 3; k++) B.Rvec(k) = ab.rvec[k] = poses[2][k], B.Tvec(k) = ab.tvec[k] = poses[2][3 + k];
        cv::Mat mask(H, W, CV_8UC1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) mask.data[(size_t)y * (size_t)mask.step + x] = (unsigned char)(((x >> 2) + (y >> 1)) & 1);
        const std::vector<unsigned char> mask_bytes = bytes_of(mask);

        arucohip_handle* h = nullptr;
        if (arucohip_create(nullptr, 0, 640, 480, 1, &h)) return 3;
        const int32_t n = 3;
        for (int type : {CV_8UC3, CV_8UC1}) {
            const int ch = type == CV_8UC3 ? 3 : 1;
            const cv::Mat frame = textured(H, W, type, 0);
            const std::vector<unsigned char> before = bytes_of(frame);
            aruco::MeshRenderer rend;
            // the defaults on markers: the green cube
            const arucohip_mesh_t acube = cube.abi(), asphere = sphere.abi();
            std::vector<unsigned char> want = before;
            if (arucohip_render_markers_batch(h, want.data(), 1, W, H, ch, (size_t)W * ch, (size_t)W * H * ch, 0, am.data(), n, &n, 0, Kf, Df, 5, &acube, nullptr,
                                              nullptr, 0))
                return 4;
            cv::Mat got = frame.clone();
            rend.draw(got, markers, cp, cube);
            report("markers", got, want, before, true);
            // a style of the caller's, the coloured sphere, a mask
            rend.style().flags = 0, rend.style().opacity = 180, rend.style().ambient = 30, rend.style().scale = 1.5f;
            rend.style().light[0] = 0.4f, rend.style().light[1] = -0.5f, rend.style().light[2] = -0.7f;
            want = before;
            if (arucohip_render_markers_batch(h, want.data(), 1, W, H, ch, (size_t)W * ch, (size_t)W * H * ch, 0, am.data(), n, &n, 0, Kf, Df, 5, &asphere,
                                              &rend.style(), mask_bytes.data(), 0))
                return 5;
            got = frame.clone();
            rend.draw(got, markers, cp, sphere, mask);
            report("markers_mask", got, want, before, true);
            // the board form with a mask: the units are the pose's, so the scale sizes the mesh
            rend.style().scale = 0.1f;
            want = before;
            if (arucohip_render_boards_batch(h, want.data(), 1, W, H, ch, (size_t)W * ch, (size_t)W * H * ch, 0, &ab, 0, Kf, Df, 5, &asphere, &rend.style(),
                                             mask_bytes.data(), 0))
                return 6;
            got = frame.clone();
            rend.draw(got, B, cp, sphere, mask);
            report("board_mask", got, want, before, true);
            // a board without a pose: the frame keeps every byte
            cv::Mat kept = frame.clone();
            rend.draw(kept, aruco::Board(), cp, cube);
            report("no_pose", kept, before, before, false);
        }
        arucohip_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
