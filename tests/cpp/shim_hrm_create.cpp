// The calls of the reference's utils_hrm/aruco_hrm_create_dictionary and aruco_hrm_create_board through the shim:
// HighlyReliableMarkers::createDicitionary, Dictionary::toFile / fromFile, createBoardImage (gray and chromatic),
// BoardConfiguration::saveToFile / readFromFile, and MarkerCode's distances. Usage: shim_hrm_create <out dir>.
// Writes board.raw and board_chromatic.raw there and prints one JSON line that tests/test_gpu_hrm_create.py checks.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "aruco_hip_shim.hpp"

static void write_raw(const std::string& path, const cv::Mat& m) {
    std::ofstream f(path.c_str(), std::ios::binary);
    const size_t row = (size_t)m.cols * m.elemSize();
    for (int r = 0; r < m.rows; r++) f.write((const char*)m.ptr<unsigned char>(r), (std::streamsize)row);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    // aruco_hrm_create_dictionary: createDicitionary(dictSize, n) after srand(...), then toFile
    aruco::Dictionary D = aruco::HighlyReliableMarkers::createDicitionary(12, 5, 7u);
    D.toFile(dir + "/dict.yml");
    aruco::Dictionary D2;
    D2.fromFile(dir + "/dict.yml");
    bool dict_rt = D2.size() == D.size() && D2.tau0 == D.tau0;
    for (size_t i = 0; dict_rt && i < D.size(); i++) dict_rt = D2[i].toString() == D[i].toString() && D2[i].getId() == D[i].getId();
    // the two-argument form takes its seed from one std::rand() call
    std::srand(11);
    const unsigned int seed = (unsigned int)std::rand();
    std::srand(11);
    aruco::Dictionary Da = aruco::HighlyReliableMarkers::createDicitionary(4, 4);
    aruco::Dictionary Db = aruco::HighlyReliableMarkers::createDicitionary(4, 4, seed);
    bool two_arg = Da.size() == 4 && Da.tau0 == Db.tau0;
    for (size_t i = 0; two_arg && i < Da.size(); i++) two_arg = Da[i].toString() == Db[i].toString();

    // aruco_hrm_create_board: createBoardImage, saveToFile
    aruco::BoardConfiguration BC;
    cv::Mat img = aruco::HighlyReliableMarkers::createBoardImage(cv::Size(2, 2), D, BC);
    write_raw(dir + "/board.raw", img);
    aruco::BoardConfiguration BCc;
    cv::Mat cimg = aruco::HighlyReliableMarkers::createBoardImage(cv::Size(2, 2), D, BCc, true);
    write_raw(dir + "/board_chromatic.raw", cimg);
    BC.saveToFile(dir + "/board.yml");
    aruco::BoardConfiguration BC2;
    BC2.readFromFile(dir + "/board.yml");
    bool board_rt = BC2.ids == BC.ids && BC2.mInfoType == BC.mInfoType && BC2.objPoints.size() == BC.objPoints.size() && BC.ids.size() == 4;
    for (size_t i = 0; board_rt && i < BC.objPoints.size(); i++)
        for (int k = 0; k < 4; k++)
            board_rt = board_rt && BC2.objPoints[i][k].x == BC.objPoints[i][k].x && BC2.objPoints[i][k].y == BC.objPoints[i][k].y &&
                       BC2.objPoints[i][k].z == BC.objPoints[i][k].z;

    aruco::Dictionary rest;
    rest.assign(D.begin() + 1, D.end());
    cv::Mat mimg = D[0].getImg(70);
    int white = 0;
    for (int r = 0; r < mimg.rows; r++)
        for (int c = 0; c < mimg.cols; c++) white += mimg.at<unsigned char>(r, c) == 255;

    std::printf("{\"codes\": [");
    for (size_t i = 0; i < D.size(); i++) {
        unsigned long long c = 0;
        for (unsigned int b = 0; b < D[i].size(); b++)
            if (D[i].get(b)) c |= 1ull << b;
        std::printf("%s%llu", i ? ", " : "", c);
    }
    std::printf("], \"tau0\": %d, \"self\": [", D.tau0);
    for (size_t i = 0; i < D.size(); i++) std::printf("%s%u", i ? ", " : "", D[i].selfDistance());
    std::printf("], \"ids\": [");
    for (size_t i = 0; i < 4; i++) std::printf("%s%d", i ? ", " : "", BC.ids[i]);
    std::printf("], \"d01\": %u, \"dict_distance\": %u, \"min_distance\": %u, \"marker_img\": %d, \"dict_roundtrip\": %s, "
                "\"board_roundtrip\": %s, \"two_arg\": %s}\n",
                D[0].distance(D[1]), rest.distance(D[0]), D.minimunDistance(), white, dict_rt ? "true" : "false", board_rt ? "true" : "false",
                two_arg ? "true" : "false");
    return 0;
}
