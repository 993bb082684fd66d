// BoardDetector::recoverMarkers through the shim: detect(im) on a frame whose board has damaged markers, then the recovery, as a caller of
// the reference-shaped API would use it. The board comes as "<n>" then n lines "<id> x y z x y z x y z x y z" (PIX units).
// Prints "detected <n>", "recovered <n>", "marker <id>" per marker of the detector's vector and "board <members>".
//   shim_recover <image.pgm> <board.txt> <fx> <fy> <cx> <cy> <marker size>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 8) return 1;
    try {
        std::ifstream f(argv[1], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        if (!(f >> magic >> w >> h >> maxv) || magic != "P5") return 1;
        f.get();
        cv::Mat gray(h, w, CV_8UC1);
        f.read((char*)gray.data, (std::streamsize)w * h);

        aruco::BoardConfiguration bc;
        bc.mInfoType = aruco::BoardConfiguration::PIX;
        std::ifstream b(argv[2]);
        int n = 0;
        b >> n;
        for (int i = 0; i < n; i++) {
            int id;
            b >> id;
            bc.ids.push_back(id);
            std::vector<cv::Point3f> pts(4);
            for (int k = 0; k < 4; k++) b >> pts[k].x >> pts[k].y >> pts[k].z;
            bc.objPoints.push_back(pts);
        }
        const float K[9] = {(float)std::atof(argv[3]), 0.f, (float)std::atof(argv[5]), 0.f, (float)std::atof(argv[4]), (float)std::atof(argv[6]), 0.f, 0.f, 1.f};
        const float dist[4] = {0.f, 0.f, 0.f, 0.f};
        aruco::CameraParameters cp(K, dist, 4, cv::Size(w, h));
        const float size = (float)std::atof(argv[7]);

        aruco::BoardDetector bd;
        bd.setParams(bc, cp, size);
        bd.detect(gray);
        std::cout << "detected " << bd.getDetectedMarkers().size() << std::endl;
        const int rec = bd.recoverMarkers(bc, cp, size);
        std::cout << "recovered " << rec << std::endl;
        for (size_t i = 0; i < bd.getDetectedMarkers().size(); i++) std::cout << "marker " << bd.getDetectedMarkers()[i].id << std::endl;
        std::cout << "board " << bd.getDetectedBoard().size() << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
