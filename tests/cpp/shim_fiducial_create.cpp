// The reference's CreateMarker and CreateBoard test sequences (test/core_tests.cpp:32-75, :118-162) and the calls of its generator
// utilities (aruco_create_marker, aruco_create_board, aruco_selectoptimalmarkers) through the shim: FiducidalMarkers::createMarkerImage,
// getMarkerMat, createBoardImage, createBoardImage_ChessBoard, createBoardImage_Frame with cv::theRNG().state = 4711.
// Prints one JSON line that tests/test_gpu_fiducial.py compares with tests/golden/fiducial.json: FNV-1a digests of the images, the
// three boards' ids and corners.
#include <cstdio>
#include <vector>

#include "aruco_hip_shim.hpp"

static unsigned long long digest(const cv::Mat& m) {
    unsigned long long h = 1469598103934665603ull;
    for (int r = 0; r < m.rows; r++) {
        const unsigned char* p = m.ptr<unsigned char>(r);
        for (int c = 0; c < m.cols; c++) h = (h ^ p[c]) * 1099511628211ull;
    }
    return h;
}

static void print_board(const char* name, const aruco::BoardConfiguration& b, const cv::Mat& img) {
    std::printf("\"%s\": {\"info_type\": %d, \"shape\": [%d, %d], \"digest\": \"%llx\", \"ids\": [", name, b.mInfoType, img.rows, img.cols, digest(img));
    for (size_t i = 0; i < b.ids.size(); i++) std::printf("%s%d", i ? ", " : "", b.ids[i]);
    std::printf("], \"obj\": [");
    for (size_t i = 0; i < b.objPoints.size(); i++)
        for (size_t k = 0; k < b.objPoints[i].size(); k++)
            std::printf("%s%.9g, %.9g, %.9g", i + k ? ", " : "", (double)b.objPoints[i][k].x, (double)b.objPoints[i][k].y, (double)b.objPoints[i][k].z);
    std::printf("]}, ");
}

int main() {
    const int pixSize = 500, markerId = 471;
    cv::Mat locked = aruco::FiducidalMarkers::createMarkerImage(markerId, pixSize, false, true);
    cv::Mat plain = aruco::FiducidalMarkers::createMarkerImage(markerId, pixSize, false, false);
    cv::Mat marked = aruco::FiducidalMarkers::createMarkerImage(markerId, pixSize, true, false);   // the watermark is not drawn
    cv::Mat defaults = aruco::FiducidalMarkers::createMarkerImage(markerId, 70);
    cv::Mat cells = aruco::FiducidalMarkers::getMarkerMat(markerId);
    int ones = 0;
    for (int y = 0; y < 5; y++)
        for (int x = 0; x < 5; x++) ones += cells.at<unsigned char>(y, x);
    std::printf("{\"marker\": {\"side\": %d, \"digest\": \"%llx\"}, \"locked\": {\"side\": %d, \"digest\": \"%llx\"}, \"watermark_arg\": \"%llx\", "
                "\"default_side\": %d, \"cells\": %d, ",
                plain.rows, digest(plain), locked.rows, digest(locked), digest(marked), defaults.rows, ones);

    const float interMarkerDistance = 0.2f;
    cv::Size gridSize(5, 5);
    const int boardPix = 100;
    cv::theRNG().state = 4711;
    aruco::BoardConfiguration DefaultBoard, ChessBoard, FrameBoard;
    // what the containers held before: the panel form replaces it, the other two append to it
    DefaultBoard.ids.assign(3, 7), DefaultBoard.objPoints.resize(3);
    cv::Mat i0 = aruco::FiducidalMarkers::createBoardImage(gridSize, boardPix, boardPix * interMarkerDistance, DefaultBoard);
    cv::Mat i1 = aruco::FiducidalMarkers::createBoardImage_ChessBoard(gridSize, boardPix, ChessBoard);
    cv::Mat i2 = aruco::FiducidalMarkers::createBoardImage_Frame(gridSize, boardPix, boardPix * interMarkerDistance, FrameBoard);
    print_board("default", DefaultBoard, i0);
    print_board("chessboard", ChessBoard, i1);
    print_board("frame", FrameBoard, i2);
    const size_t before = FrameBoard.ids.size();
    std::vector<int> excluded(FrameBoard.ids.begin(), FrameBoard.ids.end());
    aruco::FiducidalMarkers::createBoardImage_Frame(cv::Size(2, 2), 56, 4, FrameBoard, false, excluded);
    bool appended = FrameBoard.ids.size() == before + 4 && FrameBoard.objPoints.size() == before + 4 && FrameBoard.objPoints[before][0].x == 0 &&
                    FrameBoard.objPoints[before][0].y == 0;
    for (size_t i = before; i < FrameBoard.ids.size(); i++)
        for (size_t k = 0; k < before; k++) appended = appended && FrameBoard.ids[i] != FrameBoard.ids[k];
    bool threw = false;
    try {
        aruco::FiducidalMarkers::createMarkerImage(1024, 100);
    } catch (const cv::Exception&) {
        threw = true;
    }
    std::printf("\"appended\": %s, \"pixels\": %s, \"bad_id_throws\": %s}\n", appended ? "true" : "false",
                DefaultBoard.isExpressedInPixels() && !DefaultBoard.isExpressedInMeters() ? "true" : "false", threw ? "true" : "false");
    return 0;
}
