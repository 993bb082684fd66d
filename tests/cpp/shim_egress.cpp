// Frames out through the shim: aruco::exportFrame of one tightly packed B,G,R host frame to NV12 and to RGBA.
// Writes both exported frames, prints "marker <id> x0 y0 ... x3 y3" per marker that MarkerDetector::detect finds on the NV12 view, and
// checks that the view converts back (aruco::convertFrame) and that a Bayer destination throws.
//   shim_egress <frame.bgr> <width> <height> <out.nv12> <out.rgba>
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
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        std::ifstream f(argv[1], std::ios::binary);
        std::vector<unsigned char> pixels((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (pixels.size() != (size_t)w * h * 3) return 1;
        cv::Mat bgr(h, w, CV_8UC3, pixels.data(), (size_t)w * 3);

        std::vector<uint8_t> nv12, rgba;
        aruco::RawFrame view, view_rgba;
        aruco::exportFrame(bgr, aruco::PixelFormat::NV12, nv12, view);
        if (nv12.size() != (size_t)w * h * 3 / 2 || view.data != nv12.data() || view.width != w || view.height != h || view.step != (size_t)w ||
            view.format != aruco::PixelFormat::NV12)
            return 3;
        aruco::exportFrame(bgr, aruco::PixelFormat::RGBA8, rgba, view_rgba);
        if (rgba.size() != (size_t)w * h * 4 || view_rgba.step != (size_t)w * 4) return 3;
        std::ofstream(argv[4], std::ios::binary).write((const char*)nv12.data(), (std::streamsize)nv12.size());
        std::ofstream(argv[5], std::ios::binary).write((const char*)rgba.data(), (std::streamsize)rgba.size());

        aruco::MarkerDetector det;
        std::vector<aruco::Marker> markers;
        det.detect(view, markers);
        std::cout << std::setprecision(9);
        for (size_t i = 0; i < markers.size(); i++) {
            std::cout << "marker " << markers[i].id;
            for (int k = 0; k < 4; k++) std::cout << " " << markers[i][k].x << " " << markers[i][k].y;
            std::cout << std::endl;
        }
        cv::Mat back;   // the RGBA view is the image again, exactly
        aruco::convertFrame(view_rgba, back, 3);
        if (back.type() != CV_8UC3 || back.cols != w || back.rows != h) return 4;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < 3 * w; x++)
                if (back.data[(size_t)y * back.step + x] != pixels[(size_t)y * 3 * w + x]) return 4;
        bool thrown = false;   // a Bayer mosaic is an input format only
        try {
            std::vector<uint8_t> none;
            aruco::RawFrame nv;
            aruco::exportFrame(bgr, aruco::PixelFormat::BAYER_RGGB, none, nv);
        } catch (const std::exception&) {
            thrown = true;
        }
        return thrown ? 0 : 5;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
