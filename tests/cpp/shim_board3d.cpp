// A board out of a plane through the shim: a METERS board file read by BoardConfiguration::readFromFile, MarkerDetector::detect and
// BoardDetector::detect on one frame, as a caller of the reference-shaped API would pose a folded board.
// Prints "detected <n>", "board <members>", "prob <likelihood>", and "Rvec x y z" / "Tvec x y z" (17 digits) when the board has a pose.
//   shim_board3d <image.pgm> <board.yml> <fx> <fy> <cx> <cy>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 7) return 1;
    try {
        std::ifstream f(argv[1], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        if (!(f >> magic >> w >> h >> maxv) || magic != "P5") return 1;
        f.get();
        cv::Mat gray(h, w, CV_8UC1);
        f.read((char*)gray.data, (std::streamsize)w * h);

        aruco::BoardConfiguration bc;
        bc.readFromFile(argv[2]);
        const float K[9] = {(float)std::atof(argv[3]), 0.f, (float)std::atof(argv[5]), 0.f, (float)std::atof(argv[4]), (float)std::atof(argv[6]), 0.f, 0.f, 1.f};
        const float dist[4] = {0.f, 0.f, 0.f, 0.f};
        aruco::CameraParameters cp(K, dist, 4, cv::Size(w, h));

        aruco::MarkerDetector md;
        std::vector<aruco::Marker> markers;
        md.detect(gray, markers, cp);
        std::cout << "detected " << markers.size() << std::endl;
        aruco::BoardDetector bd;
        aruco::Board board;
        const float prob = bd.detect(markers, bc, board, cp);
        std::cout << "board " << board.size() << std::endl;
        std::printf("prob %.9g\n", (double)prob);
        if (!board.Rvec.empty() && !board.Tvec.empty()) {
            std::printf("Rvec %.17g %.17g %.17g\n", board.Rvec(0), board.Rvec(1), board.Rvec(2));
            std::printf("Tvec %.17g %.17g %.17g\n", board.Tvec(0), board.Tvec(1), board.Tvec(2));
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
