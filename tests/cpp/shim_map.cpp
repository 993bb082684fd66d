// Marker mapping through the shim: BoardDetector::mapBoard on observations read from a text file, then BoardDetector::detect with the
// returned BoardConfiguration on the markers of one frame, as a caller would map a marker cube once and pose it afterwards.
// Prints "mapped f0 f1 ..", "rms <pixels>", one "obj <id> x y z x y z x y z x y z" line per marker (9 digits: floats), "info <mInfoType>",
// then "board <members>" and "Rvec x y z" / "Tvec x y z" (17 digits) of the frame given.
// With the seven further arguments it also detects the markers of an image with the board detector's own MarkerDetector and maps the
// ids <first id> .. <first id> + <count> - 1 from that one-frame batch where it lies (BoardDetector::mapBoardLastBatch): "last detected
// <n>", "last mapped f0 f1 ..", "last rms <pixels>" and one "last obj <id> ..." line per marker.
//   shim_map <observations.txt> <frame> <marker size> <fx> <fy> <cx> <cy> <k1> <k2> <p1> <p2> <k3> [<image.pgm> <fx> <fy> <cx> <cy> <first id> <count>]
// observations.txt: "<frames> <markers>", the ids, then one line "frame id x0 y0 x1 y1 x2 y2 x3 y3" per observation.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 13) return 1;
    try {
        std::ifstream f(argv[1]);
        int nframes = 0, nboard = 0;
        if (!(f >> nframes >> nboard)) return 1;
        std::vector<int> ids(nboard);
        for (int i = 0; i < nboard; i++) f >> ids[i];
        std::vector<std::vector<aruco::Marker> > frames(nframes);
        int fr, id;
        while (f >> fr >> id) {
            aruco::Marker m;
            m.id = id;
            for (int k = 0; k < 4; k++) {
                float x, y;
                f >> x >> y;
                m.push_back(cv::Point2f(x, y));
            }
            if (fr >= 0 && fr < nframes) frames[fr].push_back(m);
        }
        const int frame = std::atoi(argv[2]);
        const float size = (float)std::atof(argv[3]);
        const float K[9] = {(float)std::atof(argv[4]), 0.f, (float)std::atof(argv[6]), 0.f, (float)std::atof(argv[5]), (float)std::atof(argv[7]), 0.f, 0.f, 1.f};
        float dist[5];
        for (int i = 0; i < 5; i++) dist[i] = (float)std::atof(argv[8 + i]);
        aruco::CameraParameters cp(K, dist, 5, cv::Size(640, 480));

        aruco::BoardDetector bd;
        std::vector<bool> mapped;
        double rms = 0;
        const aruco::BoardConfiguration bc = bd.mapBoard(frames, ids, cp, size, &mapped, &rms);
        std::printf("mapped");
        for (size_t i = 0; i < mapped.size(); i++) std::printf(" %d", mapped[i] ? 1 : 0);
        std::printf("\nrms %.17g\n", rms);
        for (size_t i = 0; i < bc.ids.size(); i++) {
            std::printf("obj %d", bc.ids[i]);
            for (int k = 0; k < 4; k++) std::printf(" %.9g %.9g %.9g", (double)bc.objPoints[i][k].x, (double)bc.objPoints[i][k].y, (double)bc.objPoints[i][k].z);
            std::printf("\n");
        }
        std::printf("info %d\n", bc.mInfoType);
        aruco::Board board;
        bd.detect(frames[frame], bc, board, cp, size);
        std::cout << "board " << board.size() << std::endl;
        if (!board.Rvec.empty() && !board.Tvec.empty()) {
            std::printf("Rvec %.17g %.17g %.17g\n", board.Rvec(0), board.Rvec(1), board.Rvec(2));
            std::printf("Tvec %.17g %.17g %.17g\n", board.Tvec(0), board.Tvec(1), board.Tvec(2));
        }
        if (argc >= 20) {
            std::ifstream g(argv[13], std::ios::binary);
            std::string magic;
            int w, h, maxv;
            if (!(g >> magic >> w >> h >> maxv) || magic != "P5") return 1;
            g.get();
            cv::Mat gray(h, w, CV_8UC1);
            g.read((char*)gray.data, (std::streamsize)w * h);
            const float K2[9] = {(float)std::atof(argv[14]), 0.f, (float)std::atof(argv[16]), 0.f, (float)std::atof(argv[15]), (float)std::atof(argv[17]), 0.f, 0.f, 1.f};
            const float d2[4] = {0.f, 0.f, 0.f, 0.f};
            aruco::CameraParameters cp2(K2, d2, 4, cv::Size(w, h));
            std::vector<int> ids2;
            for (int i = 0; i < std::atoi(argv[19]); i++) ids2.push_back(std::atoi(argv[18]) + i);
            std::vector<aruco::Marker> found;
            bd.getMarkerDetector().detect(gray, found, cp2);
            std::printf("last detected %d\n", (int)found.size());
            std::vector<bool> mapped2;
            double rms2 = 0;
            const aruco::BoardConfiguration bc2 = bd.mapBoardLastBatch(1, ids2, cp2, size, 2, &mapped2, &rms2);
            std::printf("last mapped");
            for (size_t i = 0; i < mapped2.size(); i++) std::printf(" %d", mapped2[i] ? 1 : 0);
            std::printf("\nlast rms %.17g\n", rms2);
            for (size_t i = 0; i < bc2.ids.size(); i++) {
                std::printf("last obj %d", bc2.ids[i]);
                for (int k = 0; k < 4; k++) std::printf(" %.9g %.9g %.9g", (double)bc2.objPoints[i][k].x, (double)bc2.objPoints[i][k].y, (double)bc2.objPoints[i][k].z);
                std::printf("\n");
            }
        }
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
