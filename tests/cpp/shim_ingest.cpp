// Camera-native input through the shim: MarkerDetector::detect(const RawFrame&) and aruco::convertFrame on one tightly packed host frame.
// Prints "marker <id> x0 y0 ... x3 y3" per marker and writes the frame converted to CV_8UC3 (B,G,R, rows packed) to <out.bgr>.
//   shim_ingest <frame.raw> <format number> <width> <height> <out.bgr>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <vector>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 1;
    try {
        const int format = std::atoi(argv[2]), w = std::atoi(argv[3]), h = std::atoi(argv[4]);
        std::ifstream f(argv[1], std::ios::binary);
        std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const size_t rows = format == ARUCOHIP_PIX_NV12 ? (size_t)h * 3 / 2 : (size_t)h;
        if (bytes.empty() || bytes.size() % rows) return 1;
        aruco::RawFrame raw;
        raw.data = bytes.data(), raw.width = w, raw.height = h, raw.step = bytes.size() / rows;
        raw.format = (aruco::PixelFormat)format, raw.bits = 0, raw.chromaOffset = 0;

        aruco::MarkerDetector det;
        std::vector<aruco::Marker> markers;
        det.detect(raw, markers);
        std::cout << std::setprecision(9);
        for (size_t i = 0; i < markers.size(); i++) {
            std::cout << "marker " << markers[i].id;
            for (int k = 0; k < 4; k++) std::cout << " " << markers[i][k].x << " " << markers[i][k].y;
            std::cout << std::endl;
        }
        cv::Mat bgr;
        aruco::convertFrame(raw, bgr, 3);
        if (bgr.type() != CV_8UC3 || bgr.cols != w || bgr.rows != h) return 3;
        std::ofstream o(argv[5], std::ios::binary);
        for (int y = 0; y < h; y++) o.write((const char*)bgr.data + (size_t)y * bgr.step, (std::streamsize)w * 3);
        bool thrown = false;   // an odd NV12 width is refused before anything runs
        try {
            aruco::RawFrame bad = raw;
            bad.format = aruco::PixelFormat::NV12, bad.width = 7, bad.height = 4, bad.step = 8;
            det.detect(bad, markers);
        } catch (const std::exception&) {
            thrown = true;
        }
        return thrown ? 0 : 5;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
