// MarkerDetector::pyrDown(level) (ArUco 1.2; markerdetector.h of the reference keeps the call as a no-op) through the shim: the level is set
// before the first frame, so it has to survive the creation of the device handle, then detect() as a caller of the reference would.
// Prints "marker <id> x0 y0 ... x3 y3" per marker and "thres <cols> <rows>", the size of getThresholdedImage().
//   shim_pyr <image.pgm> <level>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    try {
        std::ifstream f(argv[1], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        if (!(f >> magic >> w >> h >> maxv) || magic != "P5") return 1;
        f.get();
        cv::Mat gray(h, w, CV_8UC1);
        f.read((char*)gray.data, (std::streamsize)w * h);

        aruco::MarkerDetector det;
        bool thrown = false;
        try {
            det.pyrDown(4);
        } catch (const std::exception&) {
            thrown = true;
        }
        if (!thrown) return 5;
        det.pyrDown((unsigned int)std::atoi(argv[2]));
        std::vector<aruco::Marker> markers;
        det.detect(gray, markers);
        std::cout << std::setprecision(9);
        for (size_t i = 0; i < markers.size(); i++) {
            std::cout << "marker " << markers[i].id;
            for (int k = 0; k < 4; k++) std::cout << " " << markers[i][k].x << " " << markers[i][k].y;
            std::cout << std::endl;
        }
        const cv::Mat& t = det.getThresholdedImage();
        std::cout << "thres " << t.cols << " " << t.rows << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
