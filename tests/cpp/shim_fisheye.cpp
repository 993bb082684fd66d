// A fisheye camera through the shim: FisheyeCamera::calibrate on views read from a text file, then a frame seen through that lens is
// detected, its markers are mapped to the ideal camera where they lie on the device (FisheyeCamera::undistortMarkers) and
// BoardDetector::detect poses the board with FisheyeCamera::idealCamera(). The frame itself is also remapped (undistortImage).
// Prints "rms <pixels>", "K <9 values>", "D <4 values>" (17 digits), "detected <n>", "ideal <n>", one "marker <id> x0 y0 .. x3 y3" line per
// ideal marker (9 digits: floats), "board <members>", "Rvec x y z" / "Tvec x y z" (17 digits) and "image <FNV-1a of the remapped frame>".
//   shim_fisheye <views.txt> <image.pgm> <board.yml> <marker size> <new fx> <new fy> <new cx> <new cy>
// views.txt: "<views>", then per view "<points>" and one line "X Y Z u v" per point.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "aruco_hip_shim.hpp"

int main(int argc, char** argv) {
    if (argc < 9) return 1;
    try {
        std::ifstream f(argv[1]);
        int nviews = 0;
        if (!(f >> nviews)) return 1;
        std::vector<std::vector<cv::Point3f> > objs(nviews);
        std::vector<std::vector<cv::Point2f> > imgs(nviews);
        for (int v = 0; v < nviews; v++) {
            int n = 0;
            f >> n;
            for (int i = 0; i < n; i++) {
                float X, Y, Z, u, w;
                f >> X >> Y >> Z >> u >> w;
                objs[v].push_back(cv::Point3f(X, Y, Z)), imgs[v].push_back(cv::Point2f(u, w));
            }
        }
        std::ifstream g(argv[2], std::ios::binary);
        std::string magic;
        int w, h, maxv;
        if (!(g >> magic >> w >> h >> maxv) || magic != "P5") return 1;
        g.get();
        cv::Mat gray(h, w, CV_8UC1);
        g.read((char*)gray.data, (std::streamsize)w * h);

        aruco::FisheyeCamera cam;
        std::vector<cv::Mat> rvecs, tvecs;
        const double rms = cam.calibrate(objs, imgs, cv::Size(w, h), 0, &rvecs, &tvecs);
        if ((int)rvecs.size() != nviews || (int)tvecs.size() != nviews) return 3;
        std::printf("rms %.17g\nK", rms);
        for (int i = 0; i < 9; i++) std::printf(" %.17g", cam.K(i / 3, i % 3));
        std::printf("\nD");
        for (int i = 0; i < 4; i++) std::printf(" %.17g", cam.D(i));
        std::printf("\n");

        cam.newCameraMatrix = cv::Mat_<double>(3, 3);
        const double kn[9] = {std::atof(argv[5]), 0, std::atof(argv[7]), 0, std::atof(argv[6]), std::atof(argv[8]), 0, 0, 1};
        for (int i = 0; i < 9; i++) cam.newCameraMatrix(i / 3, i % 3) = kn[i];

        aruco::BoardDetector bd;
        aruco::BoardConfiguration bc;
        bc.readFromFile(argv[3]);
        std::vector<aruco::Marker> found;
        bd.getMarkerDetector().detect(gray, found);
        std::printf("detected %d\n", (int)found.size());
        const std::vector<aruco::Marker> ideal = cam.undistortMarkers(bd.getMarkerDetector());
        std::printf("ideal %d\n", (int)ideal.size());
        for (size_t i = 0; i < ideal.size(); i++) {
            std::printf("marker %d", ideal[i].id);
            for (int k = 0; k < 4; k++) std::printf(" %.9g %.9g", (double)ideal[i][k].x, (double)ideal[i][k].y);
            std::printf("\n");
        }
        aruco::Board board;
        bd.detect(ideal, bc, board, cam.idealCamera(), (float)std::atof(argv[4]));
        std::cout << "board " << board.size() << std::endl;
        if (!board.Rvec.empty() && !board.Tvec.empty()) {
            std::printf("Rvec %.17g %.17g %.17g\n", board.Rvec(0), board.Rvec(1), board.Rvec(2));
            std::printf("Tvec %.17g %.17g %.17g\n", board.Tvec(0), board.Tvec(1), board.Tvec(2));
        }
        cv::Mat flat;
        cam.undistortImage(gray, flat);
        unsigned long long hash = 1469598103934665603ull;
        for (int r = 0; r < flat.rows; r++)
            for (int c = 0; c < flat.cols; c++) hash = (hash ^ flat.at<unsigned char>(r, c)) * 1099511628211ull;
        std::printf("image %llu\n", hash);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
