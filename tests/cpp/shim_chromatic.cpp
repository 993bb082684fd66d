// The reference's ChromaticMask call sequence through the shim: setParams(BC, markersize), train, classify2, getMask, update, classify2,
// getMask, getCellMap. Usage: shim_chromatic <in.txt> <frame.raw> <occluded.raw> <out.raw>. in.txt: W H, K (9), rvec (3), tvec (3),
// mc nc thresh markersize info_type nmarkers, then 12 floats per marker. out.raw: mask, mask after update, cell map (W x H each).
#include <cstdio>
#include <fstream>

#include "aruco_hip_shim.hpp"

static cv::Mat read_plane(const char* path, int W, int H) {
    cv::Mat m(H, W, CV_8UC1);
    std::ifstream f(path, std::ios::binary);
    f.read((char*)m.data, (std::streamsize)W * H);
    return m;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    std::ifstream in(argv[1]);
    int W, H, mc, nc, info, nm;
    float K[9], markersize;
    double r[3], t[3], thresh;
    in >> W >> H;
    for (float& k : K) in >> k;
    for (double& v : r) in >> v;
    for (double& v : t) in >> v;
    in >> mc >> nc >> thresh >> markersize >> info >> nm;
    aruco::BoardConfiguration bc;
    bc.mInfoType = info;
    for (int i = 0; i < nm; i++) {
        std::vector<cv::Point3f> pts(4);
        for (int j = 0; j < 4; j++) in >> pts[j].x >> pts[j].y >> pts[j].z;
        bc.objPoints.push_back(pts), bc.ids.push_back(i);
    }
    const float d[5] = {0, 0, 0, 0, 0};
    aruco::CameraParameters cp;
    cp.setParams(K, d, 5, cv::Size(W, H));
    aruco::Board board;
    board.Rvec = cv::Mat_<double>(3, 1), board.Tvec = cv::Mat_<double>(3, 1);
    for (int k = 0; k < 3; k++) board.Rvec(k) = r[k], board.Tvec(k) = t[k];
    cv::Mat frame = read_plane(argv[2], W, H), occ = read_plane(argv[3], W, H);
    ChromaticMask cm;
    cm.setParams(mc, nc, thresh, cp, bc, markersize);
    if (cm.isValid()) return 3;
    cm.train(frame, board);
    if (!cm.isValid()) return 4;
    cm.classify2(occ, board);
    cv::Mat m1 = cm.getMask();
    cm.update(occ);
    cm.classify2(occ, board);
    cv::Mat m2 = cm.getMask(), cells = cm.getCellMap();
    std::ofstream out(argv[4], std::ios::binary);
    for (const cv::Mat* m : {&m1, &m2, &cells}) out.write((const char*)m->data, (std::streamsize)W * H);
    EMClassifier em;
    for (int i = 0; i < 300; i++) em.addSample((unsigned char)(i % 2 ? 40 + i % 5 : 200 + i % 7));
    em.train();
    std::printf("%u %d %d %.6g\n", em.numsamples(), (int)em.classify(42), (int)em.classify(120), em.getProb(42));
    return 0;
}
