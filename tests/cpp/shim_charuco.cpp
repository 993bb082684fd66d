// aruco::CharucoBoard through the shim, once: the board is painted, pasted into a white 640 x 480 frame, detected, its inner corners are
// interpolated and its pose estimated, as a caller of the reference-shaped API would do it.
// Prints "size <w> <h>", "image <hex of an FNV-1a hash of the board image>", "markers <n>", "found <n>", "records <hex bytes of every corner record>",
// "ids <numbers of the found corners>" and "pose <hex bytes of the arucohip_board_t>".
//   shim_charuco <squares x> <squares y> <square px> <marker px> <square size> <id> ...
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "aruco_hip_shim.hpp"

static void hex(const char* name, const void* p, size_t n) {
    std::printf("%s ", name);
    for (size_t i = 0; i < n; i++) std::printf("%02x", ((const unsigned char*)p)[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 7) return 1;
    try {
        std::vector<int> ids;
        for (int i = 6; i < argc; i++) ids.push_back(std::atoi(argv[i]));
        aruco::CharucoBoard board = aruco::CharucoBoard::create(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), ids);
        const float square = (float)std::atof(argv[5]);
        cv::Mat img = board.image();
        std::printf("size %d %d\n", img.cols, img.rows);
        unsigned long long hash = 1469598103934665603ull;
        for (int y = 0; y < img.rows; y++)
            for (int x = 0; x < img.cols; x++) hash = (hash ^ img.at<unsigned char>(y, x)) * 1099511628211ull;
        std::printf("image %016llx\n", hash);
        const int W = 640, H = 480, ox = (W - img.cols) / 2, oy = (H - img.rows) / 2;
        if (ox < 0 || oy < 0) return 1;
        cv::Mat frame(H, W, CV_8UC1);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const bool in = x >= ox && x < ox + img.cols && y >= oy && y < oy + img.rows;
                frame.at<unsigned char>(y, x) = in ? img.at<unsigned char>(y - oy, x - ox) : 255;
            }
        const float K[9] = {600.f, 0.f, 320.f, 0.f, 600.f, 240.f, 0.f, 0.f, 1.f};
        const float dist[4] = {0.f, 0.f, 0.f, 0.f};
        aruco::CameraParameters cp(K, dist, 4, cv::Size(W, H));
        aruco::MarkerDetector det;
        std::vector<aruco::Marker> markers;
        det.detect(frame, markers);
        std::printf("markers %d\n", (int)markers.size());
        const int found = board.detectCorners(det, frame);
        std::printf("found %d\n", found);
        hex("records", board.records.data(), board.records.size() * sizeof(arucohip_charuco_corner_t));
        std::printf("ids");
        for (size_t i = 0; i < board.cornerIds.size(); i++) std::printf(" %d", board.cornerIds[i]);
        std::printf("\n");
        const bool ok = board.estimatePose(cp, square);
        std::printf("has_pose %d\n", ok ? 1 : 0);
        hex("pose", &board.pose, sizeof(board.pose));
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
