// Camera rigs through the shim: the frames of a two-camera stream (view v = instant * 2 + camera) are detected one by one with a
// MarkerDetector, aruco::CameraRig::calibrate finds camera 1's transform from the markers of every view, CameraRig::detect poses the
// board in the rig frame from both cameras, and the batch overload is asked for the detector's last batch, which is one frame and no whole
// instant of two cameras: it must refuse (cv::Exception code -215, the shim's code of ARUCOHIP_E_INVALID). Then the same frames go through
// arucohip_detect_batch on a handle with room for them, and the last-batch overloads of calibrate and detect run on that handle where the
// markers lie; the overloads that take the views run on the markers read back.
// Prints "views n0 n1 ..", "calibrated f0 f1", "rms <pixels>", "cam <c> rx ry rz tx ty tz" (17 digits), "calib <t> rx .. tz" per used
// instant, "pose <t> rx .. tz" per instant with a pose, "batch calibrate <exception code>"; of the last-batch overloads "bviews n0 n1 ..",
// "brms", "bcam", "bcalib", "bpose" in the same form, and "batch equals views <0 or 1>": whether every number equals the one that the
// overloads taking the views give on the markers read back.
//   shim_rig <fx> <fy> <cx> <cy> <board.txt> <frame0.pgm> <frame1.pgm> ...
// board.txt: one line per marker, its id and 12 numbers: its corners in metres.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "aruco_hip_shim.hpp"

static void print6(const char* tag, int i, const cv::Mat_<double>& r, const cv::Mat_<double>& t) {
    std::printf("%s %d %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, i, r(0), r(1), r(2), t(0), t(1), t(2));
}

static bool same3(const cv::Mat_<double>& a, const cv::Mat_<double>& b) {
    if (a.empty() != b.empty()) return false;
    for (int k = 0; k < 3 && !a.empty(); k++)
        if (a(k) != b(k)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 8) return 1;
    try {
        const float K[9] = {(float)std::atof(argv[1]), 0.f, (float)std::atof(argv[3]), 0.f, (float)std::atof(argv[2]), (float)std::atof(argv[4]), 0.f, 0.f, 1.f};
        const float d4[4] = {0.f, 0.f, 0.f, 0.f};
        aruco::CameraParameters cp(K, d4, 4, cv::Size(640, 480));
        aruco::BoardConfiguration bc;
        bc.mInfoType = aruco::BoardConfiguration::METERS;
        std::ifstream bf(argv[5]);
        int id;
        while (bf >> id) {
            std::vector<cv::Point3f> c(4);
            for (int k = 0; k < 4; k++) bf >> c[k].x >> c[k].y >> c[k].z;
            bc.ids.push_back(id), bc.objPoints.push_back(c);
        }
        aruco::MarkerDetector md;
        std::vector<std::vector<aruco::Marker> > views;
        for (int a = 6; a < argc; a++) {
            std::ifstream g(argv[a], std::ios::binary);
            std::string magic;
            int w, h, maxv;
            if (!(g >> magic >> w >> h >> maxv) || magic != "P5") return 1;
            g.get();
            cv::Mat gray(h, w, CV_8UC1);
            g.read((char*)gray.data, (std::streamsize)w * h);
            std::vector<aruco::Marker> found;
            md.detect(gray, found);
            views.push_back(found);
        }
        std::printf("views");
        for (size_t v = 0; v < views.size(); v++) std::printf(" %d", (int)views[v].size());
        std::printf("\n");

        aruco::CameraRig rig(std::vector<aruco::CameraParameters>(2, cp));
        const std::vector<aruco::Board> at = rig.calibrate(md, views, bc);
        std::printf("calibrated %d %d\nrms %.17g\n", rig.calibrated[0] ? 1 : 0, rig.calibrated[1] ? 1 : 0, rig.rms);
        for (int c = 0; c < 2; c++) print6("cam", c, rig.Rvec[c], rig.Tvec[c]);
        for (size_t t = 0; t < at.size(); t++)
            if (!at[t].Rvec.empty()) print6("calib", (int)t, at[t].Rvec, at[t].Tvec);
        const std::vector<aruco::Board> poses = rig.detect(md, views, bc);
        for (size_t t = 0; t < poses.size(); t++)
            if (!poses[t].Rvec.empty()) print6("pose", (int)t, poses[t].Rvec, poses[t].Tvec);

        // the detector's last batch is the last frame alone: no whole instant of two cameras
        int code = 0;
        try {
            aruco::CameraRig again(rig.cameras);
            again.calibrate(md, bc, -1.f, 2, 1);
        } catch (const cv::Exception& e) {
            code = e.code;
        }
        std::printf("batch calibrate %d\n", code);

        const int nf = argc - 6, w = 640, h = 480, cap = 128;
        std::vector<unsigned char> packed((size_t)nf * w * h);
        for (int f = 0; f < nf; f++) {
            std::ifstream g(argv[6 + f], std::ios::binary);
            std::string magic;
            int fw, fh, maxv;
            if (!(g >> magic >> fw >> fh >> maxv) || fw != w || fh != h) return 1;
            g.get();
            g.read((char*)packed.data() + (size_t)f * w * h, (std::streamsize)w * h);
        }
        arucohip_handle* hb = nullptr;
        if (arucohip_create(nullptr, 0, w, h, nf, &hb) != ARUCOHIP_OK) return 3;
        std::vector<arucohip_marker_t> found((size_t)nf * cap);
        std::vector<int32_t> n(nf, 0);
        if (arucohip_detect_batch(hb, packed.data(), nf, w, h, (size_t)w, (size_t)w * h, 0, nullptr, nullptr, 0, -1.f, 0, found.data(), cap, n.data(), 0) != ARUCOHIP_OK)
            return 3;
        std::vector<std::vector<aruco::Marker> > bviews(nf);
        std::printf("bviews");
        for (int f = 0; f < nf; f++) {
            for (int i = 0; i < n[f]; i++) bviews[f].push_back(aruco::Marker::from_abi(found[(size_t)f * cap + i]));
            std::printf(" %d", (int)n[f]);
        }
        std::printf("\n");
        aruco::CameraRig brig(rig.cameras), vrig(rig.cameras);
        const std::vector<aruco::Board> bat = brig.calibrate(hb, bc, -1.f, 2, nf);
        const std::vector<aruco::Board> bposes = brig.detect(hb, bc, -1.f, nf);
        std::printf("brms %.17g\n", brig.rms);
        for (int c = 0; c < 2; c++) print6("bcam", c, brig.Rvec[c], brig.Tvec[c]);
        for (size_t t = 0; t < bat.size(); t++)
            if (!bat[t].Rvec.empty()) print6("bcalib", (int)t, bat[t].Rvec, bat[t].Tvec);
        for (size_t t = 0; t < bposes.size(); t++)
            if (!bposes[t].Rvec.empty()) print6("bpose", (int)t, bposes[t].Rvec, bposes[t].Tvec);
        // the overloads that take the views, on the markers read back
        bool same = false;
        {
            const std::vector<aruco::Board> vat = vrig.calibrate(md, bviews, bc);
            const std::vector<aruco::Board> vposes = vrig.detect(md, bviews, bc);
            same = vat.size() == bat.size() && vposes.size() == bposes.size() && vrig.rms == brig.rms;
            for (int c = 0; c < 2 && same; c++)
                same = vrig.calibrated[c] == brig.calibrated[c] && same3(vrig.Rvec[c], brig.Rvec[c]) && same3(vrig.Tvec[c], brig.Tvec[c]);
            for (size_t t = 0; t < bat.size() && same; t++) same = same3(vat[t].Rvec, bat[t].Rvec) && same3(vat[t].Tvec, bat[t].Tvec);
            for (size_t t = 0; t < bposes.size() && same; t++) same = same3(vposes[t].Rvec, bposes[t].Rvec) && same3(vposes[t].Tvec, bposes[t].Tvec);
        }
        std::printf("batch equals views %d\n", same ? 1 : 0);
        arucohip_destroy(hb);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 2;
    }
}
