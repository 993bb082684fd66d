// Marker::calculateExtrinsicsBoth through the shim: detect() with a camera on a still, then both planar solutions of every marker.
//   shim_planar <image.pgm> <marker size> fx fy cx cy k1 k2 p1 p2 k3
// Prints per marker "marker <id> n <nSolutions> own r0 r1 r2 t0 t1 t2" and per solution "sol <j> rms r0 r1 r2 t0 t1 t2".
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 12) return 1;
    try {
        std::ifstream f(argv[1], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        if (!(f >> magic >> w >> h >> maxv) || magic != "P5") return 1;
        f.get();
        cv::Mat gray(h, w, CV_8UC1);
        f.read((char*)gray.data, (std::streamsize)w * h);
        const float size = (float)std::atof(argv[2]);
        cv::Mat K = cv::Mat::zeros(3, 3, CV_32FC1), D(1, 5, CV_32FC1);
        K.at<float>(0, 0) = (float)std::atof(argv[3]), K.at<float>(1, 1) = (float)std::atof(argv[4]);
        K.at<float>(0, 2) = (float)std::atof(argv[5]), K.at<float>(1, 2) = (float)std::atof(argv[6]), K.at<float>(2, 2) = 1.f;
        for (int i = 0; i < 5; i++) D.at<float>(0, i) = (float)std::atof(argv[7 + i]);
        float Kf[9], Df[5];
        for (int i = 0; i < 9; i++) Kf[i] = K.at<float>(i / 3, i % 3);
        for (int i = 0; i < 5; i++) Df[i] = D.at<float>(0, i);
        aruco::CameraParameters cp(Kf, Df, 5, cv::Size(w, h));

        aruco::MarkerDetector det;
        std::vector<aruco::Marker> markers;
        det.detect(gray, markers, cp, size, false);
        for (size_t i = 0; i < markers.size(); i++) {
            const aruco::Marker& m = markers[i];
            const aruco::PlanarPoses a = m.calculateExtrinsicsBoth(size, K, D);          // refined, as Marker::Rvec is
            const aruco::PlanarPoses b = m.calculateExtrinsicsBoth(size, cp, true, false);
            if (a.nSolutions != b.nSolutions) return 3;
            std::printf("marker %d n %d own %.17g %.17g %.17g %.17g %.17g %.17g\n", m.id, a.nSolutions, m.Rvec(0), m.Rvec(1), m.Rvec(2), m.Tvec(0), m.Tvec(1),
                        m.Tvec(2));
            for (int j = 0; j < a.nSolutions; j++) {
                if (a.Rvec[j].rows != 3 || a.Rvec[j].cols != 1 || a.Tvec[j].rows != 3 || a.Tvec[j].cols != 1 || a.Rvec[j].type() != CV_64FC1) return 4;
                for (int k = 0; k < 3; k++)
                    if (a.Rvec[j].at<double>(k, 0) != b.Rvec[j].at<double>(k, 0) || a.Tvec[j].at<double>(k, 0) != b.Tvec[j].at<double>(k, 0)) return 5;
                std::printf("sol %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", j, a.rms[j], a.Rvec[j].at<double>(0, 0), a.Rvec[j].at<double>(1, 0),
                            a.Rvec[j].at<double>(2, 0), a.Tvec[j].at<double>(0, 0), a.Tvec[j].at<double>(1, 0), a.Tvec[j].at<double>(2, 0));
            }
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
}
