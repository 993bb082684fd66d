// Header-only C++ shim: the reference's classes for the detection path, implemented on the arucohip C ABI.
//
//   aruco::MarkerDetector   /root/reference/src/markerdetector.h:42-310
//   aruco::Marker           /root/reference/src/marker.h:43-140
//   aruco::CameraParameters /root/reference/src/cameraparameters.h:36-127 (data, resize, readFromXMLFile, GL / Ogre projection)
//   aruco::BoardConfiguration, aruco::Board  /root/reference/src/board.h:54-137 (data, readFromFile, GL / Ogre pose)
//   aruco::BoardDetector    /root/reference/src/boarddetector.h:40-148
//   aruco::Dictionary, aruco::MarkerCode, aruco::HighlyReliableMarkers  /root/reference/src/highlyreliablemarkers.h:50-260
//                           (dictionary files, loadDictionary, the decoder token for setMakerDetectorFunction,
//                           createDicitionary and createBoardImage on the device, MarkerCode's rotations and distances)
//   aruco::FiducidalMarkers src/arucofidmarkers.h:82-130 (the decoder token; createMarkerImage, getMarkerMat and the three
//                           createBoardImage* layouts on the device, their ids from cv::theRNG())
//
// Same member names, argument meaning and failure behaviour (CV_Assert -> cv::Exception) as the reference, so a caller
// of the reference compiles against this header and links libarucohip.so instead of libaruco + OpenCV imgproc/calib3d.
// When <opencv2/core.hpp> is on the include path the real cv:: types are used; otherwise a minimal stand-in with the
// same spelling (cv::Mat view, Point2f, Point3f, Size, Mat_<T>, Exception) keeps the header self-contained — that is
// the configuration tested in this repository (OpenCV is not installed in the build image).
#pragma once
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <string>
#include <cstdlib>
#include <iterator>
#include <fstream>
#include <type_traits>
#include <vector>

#include "arucohip.h"

#if defined(ARUCOHIP_USE_OPENCV) || (defined(__has_include) && __has_include(<opencv2/core.hpp>) && !defined(ARUCOHIP_NO_OPENCV))
#include <opencv2/core.hpp>
#define ARUCOHIP_HAVE_OPENCV 1
#else
#define ARUCOHIP_HAVE_OPENCV 0
namespace cv {
enum { CV_8UC1_ = 0, CV_8UC3_ = 16, CV_32FC1_ = 5, CV_64FC1_ = 6 };
#ifndef CV_8UC1
#define CV_8UC1 cv::CV_8UC1_
#define CV_8UC3 cv::CV_8UC3_
#define CV_32FC1 cv::CV_32FC1_
#define CV_64FC1 cv::CV_64FC1_
#endif
struct Point2f {
    float x, y;
    Point2f(float x_ = 0, float y_ = 0) : x(x_), y(y_) {}
};
struct Point3f {
    float x, y, z;
    Point3f(float x_ = 0, float y_ = 0, float z_ = 0) : x(x_), y(y_), z(z_) {}
};
struct Point {   // cv::Point = Point_<int>: contour points (MarkerCandidate::contour)
    int x, y;
    Point(int x_ = 0, int y_ = 0) : x(x_), y(y_) {}
};
struct Size {
    int width, height;
    Size(int w = 0, int h = 0) : width(w), height(h) {}
    bool operator==(const Size& o) const { return width == o.width && height == o.height; }
};
inline std::ostream& operator<<(std::ostream& s, const Point2f& p) { return s << "[" << p.x << ", " << p.y << "]"; }
class Exception : public std::runtime_error {
public:
    int code;
    Exception(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
// Dense 2-D array: owns its storage or views caller memory (like a cv::Mat header over external data).
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step = 0;
    unsigned char* data = nullptr;
    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(int r, int c, int type, void* ext, size_t step_ = 0) : rows(r), cols(c), data((unsigned char*)ext), type_(type) {
        step = step_ ? step_ : (size_t)c * elemSize();
    }
    void create(int r, int c, int type) {
        type_ = type, rows = r, cols = c;
        step = (size_t)c * elemSize();
        store_ = std::make_shared<std::vector<unsigned char> >((size_t)r * step, (unsigned char)0);
        data = store_->data();
    }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    int type() const { return type_; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    size_t total() const { return (size_t)rows * cols; }
    size_t elemSize() const { return type_ == CV_8UC1_ ? 1 : type_ == CV_8UC3_ ? 3 : type_ == CV_32FC1_ ? 4 : 8; }
    Size size() const { return Size(cols, rows); }
    template <class T> T& at(int r, int c) { return *(T*)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <class T> const T& at(int r, int c) const { return *(const T*)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <class T> T* ptr(int r = 0) { return (T*)(data + (size_t)r * step); }
    template <class T> const T* ptr(int r = 0) const { return (const T*)(data + (size_t)r * step); }
    Mat clone() const {
        Mat m(rows, cols, type_);
        for (int r = 0; r < rows; r++) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols * elemSize());
        return m;
    }
protected:
    int type_ = CV_8UC1_;
    std::shared_ptr<std::vector<unsigned char> > store_;
};
template <class T> struct MatDepth_;
template <> struct MatDepth_<float> { enum { value = CV_32FC1_ }; };
template <> struct MatDepth_<double> { enum { value = CV_64FC1_ }; };
template <> struct MatDepth_<unsigned char> { enum { value = CV_8UC1_ }; };
template <class T> class Mat_ : public Mat {
public:
    Mat_() { type_ = MatDepth_<T>::value; }
    Mat_(int r, int c) : Mat(r, c, MatDepth_<T>::value) {}
    T& operator()(int r, int c) { return at<T>(r, c); }
    const T& operator()(int r, int c) const { return at<T>(r, c); }
    T& operator()(int i) { return ((T*)data)[i]; }
    const T& operator()(int i) const { return ((const T*)data)[i]; }
};
typedef const Mat& InputArray;
typedef Mat& OutputArray;
}  // namespace cv
#endif
#ifndef CV_VERSION
// cv::theRNG(): the generator FiducidalMarkers::createBoardImage* shuffle the marker ids with. Every OpenCV has it (and CV_VERSION);
// without OpenCV only its public state exists (callers assign it: cv::theRNG().state = 4711), and arucohip_fiducial_shuffle_ids
// advances it as cv::RNG would.
namespace cv {
struct RNG {
    unsigned long long state;
    RNG(unsigned long long s = 0xffffffff) : state(s) {}
};
inline RNG& theRNG() {
    static RNG r;
    return r;
}
}  // namespace cv
#endif

namespace aruco {

inline void arucohip_throw_(int rc, const char* what, arucohip_handle* h) {
    if (rc == ARUCOHIP_OK) return;
    std::string msg = std::string(what) + ": " + (h ? arucohip_last_error_string(h) : "") + " (arucohip status " + std::to_string(rc) + ")";
    throw cv::Exception(rc == ARUCOHIP_E_INVALID ? -215 /* StsAssert */ : -2, msg
#if ARUCOHIP_HAVE_OPENCV
                        , "arucohip", __FILE__, __LINE__
#endif
    );
}

// ---- small conversions between the caller's matrices and the ABI's plain arrays
inline bool mat_to_K_(const cv::Mat& m, float K[9]) {
    if (m.empty()) return false;
    if (m.rows != 3 || m.cols != 3) arucohip_throw_(ARUCOHIP_E_INVALID, "camera matrix must be 3x3", nullptr);
    for (int i = 0; i < 9; i++)
        K[i] = m.type() == CV_64FC1 ? (float)m.at<double>(i / 3, i % 3) : m.at<float>(i / 3, i % 3);
    return true;
}
inline int mat_to_dist_(const cv::Mat& m, float d[8]) {
    if (m.empty()) return 0;
    int n = (int)std::min<size_t>(m.total(), 8);
    for (int i = 0; i < n; i++) {
        int r = m.cols == 1 ? i : 0, c = m.cols == 1 ? 0 : i;
        d[i] = m.type() == CV_64FC1 ? (float)m.at<double>(r, c) : m.at<float>(r, c);
    }
    return n;
}

// ---- minimal reader for the OpenCV FileStorage YAML files the reference ships and writes (camera intrinsics
// src/cameraparameters.cpp:187-222, board configurations src/serialization.cpp:94-120): top-level scalars, !!opencv-matrix
// blocks and the flow-style marker list. Not a general YAML parser.
namespace yml_ {
inline std::string slurp(const std::string& path) {
    std::ifstream f(path.c_str());
    if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot open " + path).c_str(), nullptr);
    std::string all((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return all;
}
// position right after "key:" where key starts a line (top level); npos if absent
inline size_t top_key(const std::string& t, const std::string& key, size_t from = 0) {
    for (size_t p = t.find(key + ":", from); p != std::string::npos; p = t.find(key + ":", p + 1))
        if (p == 0 || t[p - 1] == '\n') return p + key.size() + 1;
    return std::string::npos;
}
inline bool scalar(const std::string& t, const std::string& key, double* v) {
    size_t p = top_key(t, key);
    if (p == std::string::npos) return false;
    *v = std::strtod(t.c_str() + p, nullptr);
    return true;
}
// numbers of the next [...] group(s) starting at p: reads until `count` numbers were found or the text ends
inline std::vector<double> numbers(const std::string& t, size_t p, size_t count, size_t* endp = nullptr) {
    std::vector<double> out;
    while (p < t.size() && out.size() < count) {
        const char c = t[p];
        if ((c >= '0' && c <= '9') || c == '-' || c == '+' || (c == '.' && p + 1 < t.size() && t[p + 1] >= '0' && t[p + 1] <= '9')) {
            char* e = nullptr;
            out.push_back(std::strtod(t.c_str() + p, &e));
            p = (size_t)(e - t.c_str());
        } else {
            p++;
        }
    }
    if (endp) *endp = p;
    return out;
}
// !!opencv-matrix block: rows, cols and rows*cols values of data: [...]
inline bool matrix(const std::string& t, const std::string& key, int* rows, int* cols, std::vector<double>* data) {
    size_t p = top_key(t, key);
    if (p == std::string::npos) return false;
    size_t r = t.find("rows:", p), c = t.find("cols:", p), d = t.find("data:", p);
    if (r == std::string::npos || c == std::string::npos || d == std::string::npos) return false;
    *rows = (int)std::strtol(t.c_str() + r + 5, nullptr, 10);
    *cols = (int)std::strtol(t.c_str() + c + 5, nullptr, 10);
    if (*rows <= 0 || *cols <= 0) return false;
    *data = numbers(t, d + 5, (size_t)*rows * *cols);
    return data->size() == (size_t)*rows * *cols;
}
}  // namespace yml_

class CameraParameters {
public:
    cv::Mat_<float> CameraMatrix;  // 3x3 (fx 0 cx, 0 fy cy, 0 0 1)
    cv::Mat_<float> Distorsion;    // k1,k2,p1,p2[,k3]
    cv::Size CamSize;
    CameraParameters() : CamSize(-1, -1) {}
    CameraParameters(const float K[9], const float* dist, int ndist, cv::Size size) { setParams(K, dist, ndist, size); }
    void setParams(const float K[9], const float* dist, int ndist, cv::Size size) {
        CameraMatrix = cv::Mat_<float>(3, 3);
        for (int i = 0; i < 9; i++) CameraMatrix(i / 3, i % 3) = K[i];
        Distorsion = cv::Mat_<float>(1, ndist);
        for (int i = 0; i < ndist; i++) Distorsion(0, i) = dist[i];
        CamSize = size;
    }
    bool isValid() const { return !CameraMatrix.empty() && !Distorsion.empty() && CamSize.width != -1 && CamSize.height != -1; }
    // cameraparameters.cpp:187-222: image_width / image_height, camera_matrix -> float, the first 5 distortion coefficients -> float
    void readFromXMLFile(const std::string& filePath) {
        const std::string t = yml_::slurp(filePath);
        double w = -1, h = -1;
        yml_::scalar(t, "image_width", &w), yml_::scalar(t, "image_height", &h);
        int kr = 0, kc = 0, dr = 0, dc = 0;
        std::vector<double> K, D;
        if (!yml_::matrix(t, "camera_matrix", &kr, &kc, &K) || K.size() != 9)
            arucohip_throw_(ARUCOHIP_E_INVALID, ("File :" + filePath + " does not contains valid camera matrix").c_str(), nullptr);
        if (w == -1 || h == 0) arucohip_throw_(ARUCOHIP_E_INVALID, ("File :" + filePath + " does not contains valid camera dimensions").c_str(), nullptr);
        if (!yml_::matrix(t, "distortion_coefficients", &dr, &dc, &D) || D.size() < 4)
            arucohip_throw_(ARUCOHIP_E_INVALID, ("File :" + filePath + " does not contains valid distortion_coefficients").c_str(), nullptr);
        float Kf[9], Df[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 9; i++) Kf[i] = (float)K[i];
        for (size_t i = 0; i < 5 && i < D.size(); i++) Df[i] = (float)D[i];
        setParams(Kf, Df, 5, cv::Size((int)w, (int)h));
    }
    // cameraparameters.h:79: the OpenCV FileStorage YAML readFromXMLFile reads back (values printed exactly)
    void saveToFile(const std::string& path, bool /*inXML*/ = true) const {
        if (!isValid()) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid camera parameters", nullptr);
        std::ofstream f(path.c_str());
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + path).c_str(), nullptr);
        char num[64];
        auto block = [&](const char* key, int rows, int cols, const float* v) {
            f << key << ": !!opencv-matrix\n   rows: " << rows << "\n   cols: " << cols << "\n   dt: d\n   data: [ ";
            for (int i = 0; i < rows * cols; i++) {
                std::snprintf(num, sizeof(num), "%.17g", (double)v[i]);
                f << num << (i + 1 < rows * cols ? ", " : " ]\n");
            }
        };
        float K[9], D[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 9; i++) K[i] = CameraMatrix(i / 3, i % 3);
        for (int i = 0; i < 5 && i < (int)Distorsion.total(); i++) D[i] = Distorsion(i);
        f << "%YAML:1.0\n---\nimage_width: " << CamSize.width << "\nimage_height: " << CamSize.height << "\n";
        block("camera_matrix", 3, 3, K);
        block("distortion_coefficients", 1, 5, D);
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + path).c_str(), nullptr);
    }
    // cameraparameters.cpp:166-179
    void resize(cv::Size size) {
        if (!isValid()) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid camera parameters", nullptr);
        if (size == CamSize) return;
        float AxFactor = float(size.width) / float(CamSize.width);
        float AyFactor = float(size.height) / float(CamSize.height);
        CameraMatrix(0, 0) *= AxFactor;
        CameraMatrix(0, 2) *= AxFactor;
        CameraMatrix(1, 1) *= AyFactor;
        CameraMatrix(1, 2) *= AyFactor;
    }
    // cameraparameters.cpp:226-266 (like the reference it first resizes *this to `size`); orgImgSize is unused there too
    void glGetProjectionMatrix(cv::Size /*orgImgSize*/, cv::Size size, double proj_matrix[16], double gnear, double gfar, bool invert = false) {
        if (!isValid()) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid camera parameters", nullptr);
        float K[9];
        for (int i = 0; i < 9; i++) K[i] = CameraMatrix(i / 3, i % 3);
        arucohip_throw_(arucohip_gl_projection(K, CamSize.width, CamSize.height, size.width, size.height, gnear, gfar, invert, proj_matrix),
                        "glGetProjectionMatrix", nullptr);
        resize(size);   // the reference's call leaves the matrix resized (and CamSize as it was)
    }
    // cameraparameters.cpp:271-295
    void OgreGetProjectionMatrix(cv::Size orgImgSize, cv::Size size, double proj_matrix[16], double gnear, double gfar, bool invert = false) {
        double t[16];
        glGetProjectionMatrix(orgImgSize, size, t, gnear, gfar, invert);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) proj_matrix[r * 4 + c] = (c == 3 ? 1.0 : -1.0) * t[c * 4 + r];
    }
};

// utils.cpp:32-147 behind the C ABI: shared by Marker and Board
inline void arucohip_gl_modelview_(const cv::Mat_<double>& Rvec, const cv::Mat_<double>& Tvec, double modelview_matrix[16]) {
    if (Rvec.empty() || Tvec.empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "extrinsic parameters are not set", nullptr);
    const double r[3] = {Rvec(0), Rvec(1), Rvec(2)}, t[3] = {Tvec(0), Tvec(1), Tvec(2)};
    arucohip_throw_(arucohip_gl_modelview(r, t, modelview_matrix), "glGetModelViewMatrix", nullptr);
}
inline void arucohip_ogre_pose_(const cv::Mat_<double>& Rvec, const cv::Mat_<double>& Tvec, double position[3], double orientation[4]) {
    if (Rvec.empty() || Tvec.empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "extrinsic parameters are not set", nullptr);
    const double r[3] = {Rvec(0), Rvec(1), Rvec(2)}, t[3] = {Tvec(0), Tvec(1), Tvec(2)};
    arucohip_throw_(arucohip_ogre_pose(r, t, position, orientation), "OgreGetPoseParameters", nullptr);
}

// Process-wide handle for calls that have no detector object to hang on (Marker::calculateExtrinsics): created on first
// use on device ARUCOHIP_DEVICE (default 0), shared under a mutex (a handle is not re-entrant), never destroyed — the HIP
// runtime may already be gone when static destructors run.
struct SharedHandle_ {
    std::mutex mu;
    arucohip_handle* h = nullptr;
    static SharedHandle_& get() {
        static SharedHandle_* s = new SharedHandle_();
        return *s;
    }
    int w = 0, hh = 0;
    arucohip_handle* ensure(int width = 64, int height = 64) {   // call with mu held
        if (!h || width > w || height > hh) {
            arucohip_destroy(h);
            h = nullptr;
            w = std::max(std::max(w, width), 32), hh = std::max(std::max(hh, height), 32);
            const char* e = std::getenv("ARUCOHIP_DEVICE");
            arucohip_throw_(arucohip_create(nullptr, e ? std::atoi(e) : 0, w, hh, 1, &h), "arucohip_create", nullptr);
        }
        return h;
    }
};

// cv::undistort(src, dst, cameraMatrix, distCoeffs) on the device: what the reference's GL apps run on
// every frame before detect() (utils/aruco_test_gl.cpp:237-240). 8-bit frames, 1 or 3 channels.
inline void undistort(const cv::Mat& src, cv::Mat& dst, const cv::Mat& cameraMatrix, const cv::Mat& distCoeffs) {
    if (src.type() != CV_8UC1 && src.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "undistort: CV_8UC1 or CV_8UC3 frames", nullptr);
    float K[9], d[8];
    if (!mat_to_K_(cameraMatrix, K)) arucohip_throw_(ARUCOHIP_E_INVALID, "undistort: camera matrix is empty", nullptr);
    const int nd = mat_to_dist_(distCoeffs, d);
    const int cn = src.type() == CV_8UC3 ? 3 : 1;
    cv::Mat out(src.rows, src.cols, src.type());
    SharedHandle_& sh = SharedHandle_::get();
    std::lock_guard<std::mutex> lock(sh.mu);
    arucohip_handle* h = sh.ensure(src.cols, src.rows);
    arucohip_throw_(arucohip_undistort(h, src.data, 1, src.cols, src.rows, src.step, (size_t)src.rows * src.step, cn, 0, K, nd ? d : nullptr, nd, out.data, 0),
                    "undistort", h);
    dst = out;
}

// Camera-native input (include/arucohip.h, "Camera-native input"): a frame as a camera or a video decoder delivers it, in host memory.
// No counterpart in the reference, which takes what cv::VideoCapture hands it.
enum class PixelFormat {
    GRAY8 = ARUCOHIP_PIX_GRAY8, BGR8 = ARUCOHIP_PIX_BGR8, RGB8 = ARUCOHIP_PIX_RGB8, BGRA8 = ARUCOHIP_PIX_BGRA8, RGBA8 = ARUCOHIP_PIX_RGBA8,
    GRAY16 = ARUCOHIP_PIX_GRAY16, YUYV = ARUCOHIP_PIX_YUYV, UYVY = ARUCOHIP_PIX_UYVY, NV12 = ARUCOHIP_PIX_NV12,
    BAYER_RGGB = ARUCOHIP_PIX_BAYER_RGGB, BAYER_BGGR = ARUCOHIP_PIX_BAYER_BGGR, BAYER_GRBG = ARUCOHIP_PIX_BAYER_GRBG,
    BAYER_GBRG = ARUCOHIP_PIX_BAYER_GBRG
};
struct RawFrame {
    const void* data;      // host memory
    int width, height;     // pixels
    size_t step;           // bytes between rows (of both planes of NV12)
    PixelFormat format;
    int bits;              // GRAY16 only: 8..16
    size_t chromaOffset;   // NV12 only: bytes from data to the U,V plane; 0: step * height
};
// one host frame through arucohip_convert_batch on handle h into a new CV_8UC1 (channels = 1) or CV_8UC3 (B,G,R) image
inline void convert_frame_(arucohip_handle* h, const RawFrame& in, cv::Mat& dst, int channels) {
    if (channels != 1 && channels != 3) arucohip_throw_(ARUCOHIP_E_INVALID, "convertFrame: channels is 1 or 3", nullptr);
    if (!in.data || in.width < 1 || in.height < 1) arucohip_throw_(ARUCOHIP_E_INVALID, "convertFrame: empty frame", nullptr);
    arucohip_frame_format_t fmt;
    fmt.format = (int32_t)in.format, fmt.bits = in.bits, fmt.chroma_offset = in.chromaOffset;
    cv::Mat out(in.height, in.width, channels == 3 ? CV_8UC3 : CV_8UC1);
    const size_t fs = arucohip_frame_min_stride(&fmt, in.width, in.height, in.step);   // one frame: never used as a stride
    arucohip_throw_(arucohip_convert_batch(h, in.data, &fmt, 1, in.width, in.height, in.step, fs, 0, channels, out.data, out.step,
                                           (size_t)in.height * out.step, 0),
                    "convertFrame", h);
    dst = out;
}
// The conversion alone, on the process-wide handle: dst becomes CV_8UC1 (channels = 1) or CV_8UC3 in B,G,R order (channels = 3).
inline void convertFrame(const RawFrame& src, cv::Mat& dst, int channels) {
    SharedHandle_& sh = SharedHandle_::get();
    std::lock_guard<std::mutex> lock(sh.mu);
    convert_frame_(sh.ensure(src.width, src.height), src, dst, channels);
}
// Frames out (include/arucohip.h, "Frames out"): one CV_8UC1 (grey) or CV_8UC3 (B,G,R) image through arucohip_export_batch on the
// process-wide handle. bytes receives the tightly packed frame in `format` (NV12: the U,V plane behind the Y plane) and view describes
// it, so that convertFrame(view, ...) and MarkerDetector::detect(view, ...) accept it; view points into bytes. flags: ARUCOHIP_EXPORT_*.
inline void exportFrame(const cv::Mat& src, PixelFormat format, std::vector<uint8_t>& bytes, RawFrame& view, int flags = 0) {
    if (src.empty() || (src.type() != CV_8UC1 && src.type() != CV_8UC3)) arucohip_throw_(ARUCOHIP_E_INVALID, "exportFrame: CV_8UC1 or CV_8UC3 frames", nullptr);
    arucohip_frame_format_t fmt;
    fmt.format = (int32_t)format, fmt.bits = 0, fmt.chroma_offset = 0;
    const size_t step = arucohip_frame_min_row_stride(&fmt, src.cols);
    const size_t size = arucohip_frame_min_stride(&fmt, src.cols, src.rows, step);   // 0: the call below refuses the format or the size
    std::vector<uint8_t> out(size ? size : 1);
    SharedHandle_& sh = SharedHandle_::get();
    std::lock_guard<std::mutex> lock(sh.mu);
    arucohip_handle* h = sh.ensure(src.cols, src.rows);
    arucohip_throw_(arucohip_export_batch(h, src.data, src.type() == CV_8UC3 ? 3 : 1, 1, src.cols, src.rows, src.step, (size_t)src.rows * src.step, 0, &fmt,
                                          flags, out.data(), step, size, 0),
                    "exportFrame", h);
    bytes.swap(out);
    view.data = bytes.data(), view.width = src.cols, view.height = src.rows, view.step = step;
    view.format = format, view.bits = 0, view.chromaOffset = 0;
}

// cv::calibrateCamera(objectPoints, imagePoints, imageSize, cameraMatrix, distCoeffs, rvecs, tvecs, flags) for planar views
// (utils/aruco_calibration.cpp's call) on the process-wide handle. flags: cv::CALIB_* values (ARUCOHIP_CALIB_*). Returns the RMS
// reprojection error; cameraMatrix (3x3), distCoeffs (1x5), rvecs / tvecs (3x1 each) come back as CV_64F.
inline double calibrateCamera(const std::vector<std::vector<cv::Point3f> >& objPointsV, const std::vector<std::vector<cv::Point2f> >& imgPointsV,
                              cv::Size imageSize, cv::Mat& cameraMatrix, cv::Mat& distCoeffs, std::vector<cv::Mat>& rvecs,
                              std::vector<cv::Mat>& tvecs, int flags = 0) {
    if (objPointsV.size() != imgPointsV.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "calibrateCamera: object and image point lists differ", nullptr);
    const int nv = (int)objPointsV.size();
    std::vector<float> obj, img;
    std::vector<int32_t> np;
    for (int v = 0; v < nv; v++) {
        if (objPointsV[v].size() != imgPointsV[v].size()) arucohip_throw_(ARUCOHIP_E_INVALID, "calibrateCamera: a view's point counts differ", nullptr);
        np.push_back((int32_t)objPointsV[v].size());
        for (const cv::Point3f& p : objPointsV[v]) obj.push_back(p.x), obj.push_back(p.y), obj.push_back(p.z);
        for (const cv::Point2f& p : imgPointsV[v]) img.push_back(p.x), img.push_back(p.y);
    }
    double K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1}, d[5] = {0, 0, 0, 0, 0};
    if (!cameraMatrix.empty() && cameraMatrix.rows == 3 && cameraMatrix.cols == 3)
        for (int i = 0; i < 9; i++)
            K[i] = cameraMatrix.type() == CV_64FC1 ? cameraMatrix.at<double>(i / 3, i % 3) : cameraMatrix.at<float>(i / 3, i % 3);
    for (int i = 0; i < 5 && !distCoeffs.empty() && i < (int)distCoeffs.total(); i++) {
        const int r = distCoeffs.cols == 1 ? i : 0, c = distCoeffs.cols == 1 ? 0 : i;
        d[i] = distCoeffs.type() == CV_64FC1 ? distCoeffs.at<double>(r, c) : distCoeffs.at<float>(r, c);
    }
    std::vector<double> rv((size_t)nv * 3), tv((size_t)nv * 3);
    double rms = 0;
    {
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_calibrate_camera(h, obj.data(), img.data(), np.data(), nv, 0, imageSize.width, imageSize.height, flags, K, d,
                                                  rv.data(), tv.data(), nullptr, &rms),
                        "calibrateCamera", h);
    }
    cameraMatrix = cv::Mat(3, 3, CV_64FC1);
    for (int i = 0; i < 9; i++) cameraMatrix.at<double>(i / 3, i % 3) = K[i];
    distCoeffs = cv::Mat(1, 5, CV_64FC1);
    for (int i = 0; i < 5; i++) distCoeffs.at<double>(0, i) = d[i];
    rvecs.clear(), tvecs.clear();
    for (int v = 0; v < nv; v++) {
        cv::Mat r(3, 1, CV_64FC1), t(3, 1, CV_64FC1);
        for (int k = 0; k < 3; k++) r.at<double>(k, 0) = rv[3 * v + k], t.at<double>(k, 0) = tv[3 * v + k];
        rvecs.push_back(r), tvecs.push_back(t);
    }
    return rms;
}

// Both pose solutions of a planar marker (Marker::calculateExtrinsicsBoth): solution j is Rvec[j] / Tvec[j] (3x1 double like
// Marker::Rvec) with reprojection error rms[j] in pixels, rms[0] <= rms[1]; nSolutions is 2, or 0 for degenerate corners (empty Mats).
struct PlanarPoses {
    cv::Mat Rvec[2], Tvec[2];
    double rms[2];
    int nSolutions;
};

class Marker : public std::vector<cv::Point2f> {
public:
    int id;
    float ssize;
    cv::Mat_<double> Rvec, Tvec;
    Marker() : id(-1), ssize(-1) {}
    explicit Marker(const std::vector<cv::Point2f>& corners, int _id = -1) : std::vector<cv::Point2f>(corners), id(_id), ssize(-1) {}
    bool isValid() const { return id != -1 && size() == 4; }
    cv::Point2f getCenter() const {
        cv::Point2f cent(0, 0);
        for (size_t i = 0; i < size(); i++) cent.x += (*this)[i].x, cent.y += (*this)[i].y;
        cent.x /= float(size());
        cent.y /= float(size());
        return cent;
    }
    float getPerimeter() const {  // utils.h:39-46
        float sum = 0;
        for (size_t i = 0; i < size(); i++) {
            size_t j = (i + 1) % size();
            float dx = (*this)[i].x - (*this)[j].x, dy = (*this)[i].y - (*this)[j].y;
            sum += std::sqrt((double)dx * dx + (double)dy * dy);
        }
        return sum;
    }
    float getArea() const {  // marker.cpp:141-151
        assert(size() == 4);
        const Marker& m = *this;
        float a1 = std::fabs((m[1].x - m[0].x) * (m[3].y - m[0].y) - (m[1].y - m[0].y) * (m[3].x - m[0].x));
        float a2 = std::fabs((m[1].x - m[2].x) * (m[3].y - m[2].y) - (m[1].y - m[2].y) * (m[3].x - m[2].x));
        return (a2 + a1) / 2.f;
    }
    // marker.h:77 / marker.cpp:85-90
    void calculateExtrinsics(float markerSize, const CameraParameters& CP, bool setYPerpendicular = true) {
        if (!CP.isValid()) arucohip_throw_(ARUCOHIP_E_INVALID, "!CP.isValid(): invalid camera parameters. It is not possible to calculate extrinsics", nullptr);
        calculateExtrinsics(markerSize, CP.CameraMatrix, CP.Distorsion, setYPerpendicular);
    }
    // marker.h:85 / marker.cpp:112-124: solvePnP of the 4 corners against the marker's own square (device kernel behind
    // arucohip_calculate_extrinsics, on the process-wide handle). MarkerDetector::calculateExtrinsics is the batched form.
    void calculateExtrinsics(float markerSize, cv::Mat CameraMatrix, cv::Mat Distorsion = cv::Mat(), bool setYPerpendicular = true) {
        if (!(markerSize > 0 && isValid())) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid marker. It is not possible to calculate extrinsics", nullptr);
        float K[9], d[8];
        if (!mat_to_K_(CameraMatrix, K)) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraMatrix is empty", nullptr);
        const int nd = mat_to_dist_(Distorsion, d);
        arucohip_marker_t m;
        to_abi(&m);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_calculate_extrinsics(h, &m, 1, K, nd ? d : nullptr, nd, markerSize, setYPerpendicular ? 1 : 0), "Marker::calculateExtrinsics", h);
        Rvec = cv::Mat_<double>(3, 1), Tvec = cv::Mat_<double>(3, 1);
        for (int k = 0; k < 3; k++) Rvec(k) = m.rvec[k], Tvec(k) = m.tvec[k];
        ssize = markerSize;
    }
    // No reference counterpart: the two poses a square has under weak perspective (arucohip_planar_poses on the process-wide handle), each
    // refined by the library's Levenberg-Marquardt when refine is set. The marker itself is not changed: its Rvec / Tvec stay the pose
    // calculateExtrinsics gave it. Throws where calculateExtrinsics throws.
    PlanarPoses calculateExtrinsicsBoth(float markerSize, cv::Mat CameraMatrix, cv::Mat Distorsion = cv::Mat(), bool refine = true,
                                        bool setYPerpendicular = false) const {
        if (!(markerSize > 0 && isValid())) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid marker. It is not possible to calculate extrinsics", nullptr);
        float K[9], d[8];
        if (!mat_to_K_(CameraMatrix, K)) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraMatrix is empty", nullptr);
        const int nd = mat_to_dist_(Distorsion, d);
        arucohip_marker_t m;
        to_abi(&m);
        arucohip_planar_poses_t pp;
        {
            SharedHandle_& sh = SharedHandle_::get();
            std::lock_guard<std::mutex> lock(sh.mu);
            arucohip_handle* h = sh.ensure();
            arucohip_throw_(arucohip_planar_poses(h, &m, 1, 0, K, nd ? d : nullptr, nd, markerSize, refine ? 1 : 0, setYPerpendicular ? 1 : 0, &pp),
                            "Marker::calculateExtrinsicsBoth", h);
        }
        PlanarPoses out;
        out.nSolutions = pp.n_solutions;
        for (int j = 0; j < 2; j++) {
            out.rms[j] = pp.rms[j];
            if (!pp.n_solutions) continue;
            cv::Mat_<double> r(3, 1), t(3, 1);
            for (int k = 0; k < 3; k++) r(k) = pp.rvec[j][k], t(k) = pp.tvec[j][k];
            out.Rvec[j] = r, out.Tvec[j] = t;
        }
        return out;
    }
    PlanarPoses calculateExtrinsicsBoth(float markerSize, const CameraParameters& CP, bool refine = true, bool setYPerpendicular = false) const {
        if (!CP.isValid()) arucohip_throw_(ARUCOHIP_E_INVALID, "!CP.isValid(): invalid camera parameters. It is not possible to calculate extrinsics", nullptr);
        return calculateExtrinsicsBoth(markerSize, CP.CameraMatrix, CP.Distorsion, refine, setYPerpendicular);
    }
    void glGetModelViewMatrix(double modelview_matrix[16]) const { arucohip_gl_modelview_(Rvec, Tvec, modelview_matrix); }              // marker.h:90
    void OgreGetPoseParameters(double position[3], double orientation[4]) const { arucohip_ogre_pose_(Rvec, Tvec, position, orientation); }  // marker.h:104
#if ARUCOHIP_HAVE_OPENCV
    // marker.h:69. The member is DECLARED so that the reference's callers compile (utils/aruco_simple.cpp:82). Its definition is the
    // includer's choice: the reference's own cv::line / cv::putText code (src/marker.cpp:54-81), or, with ARUCOHIP_SHIM_DEFINE_DRAWING
    // defined before this header, the device overlay below (aruco::DeviceDrawing) - INTEGRATION.md "drawing".
    void draw(cv::Mat& in, cv::Scalar color, int lineWidth = 1, bool writeId = true) const;
#endif
    friend bool operator<(const Marker& a, const Marker& b) { return a.id < b.id; }
    friend std::ostream& operator<<(std::ostream& str, const Marker& M) {  // marker.h:128-139
        str << M.id << "=";
        for (int i = 0; i < 4 && i < (int)M.size(); i++) str << "(" << M[i].x << "," << M[i].y << ") ";
        if (!M.Tvec.empty() && !M.Rvec.empty()) {
            str << "Txyz=" << M.Tvec(0) << " " << M.Tvec(1) << " " << M.Tvec(2) << " ";
            str << "Rxyz=" << M.Rvec(0) << " " << M.Rvec(1) << " " << M.Rvec(2) << " ";
        }
        return str;
    }
    void to_abi(arucohip_marker_t* o) const {
        std::memset(o, 0, sizeof(*o));
        o->id = id, o->ssize = ssize;
        for (int k = 0; k < 4 && k < (int)size(); k++) o->corners[2 * k] = (*this)[k].x, o->corners[2 * k + 1] = (*this)[k].y;
        if (!Rvec.empty() && !Tvec.empty()) {
            o->has_pose = 1;
            for (int k = 0; k < 3; k++) o->rvec[k] = Rvec(k), o->tvec[k] = Tvec(k);
        }
    }
    static Marker from_abi(const arucohip_marker_t& m) {
        Marker r;
        r.id = m.id, r.ssize = m.ssize;
        for (int k = 0; k < 4; k++) r.push_back(cv::Point2f(m.corners[2 * k], m.corners[2 * k + 1]));
        if (m.has_pose) {
            r.Rvec = cv::Mat_<double>(3, 1), r.Tvec = cv::Mat_<double>(3, 1);
            for (int k = 0; k < 3; k++) r.Rvec(k) = m.rvec[k], r.Tvec(k) = m.tvec[k];
        }
        return r;
    }
};

class BoardConfiguration {
public:
    std::vector<int> ids;
    std::vector<std::vector<cv::Point3f> > objPoints;
    enum MarkerInfoType { NONE = -1, PIX = 0, METERS = 1 };
    int mInfoType;
    BoardConfiguration() : mInfoType(NONE) {}
    // board.cpp:52-56 + src/serialization.cpp:94-120: aruco_bc_nmarkers, aruco_bc_mInfoType, aruco_bc_markers: - { id:.., corners:[ [x,y,z] x4 ] }
    void readFromFile(const std::string& sfile) {
        const std::string t = yml_::slurp(sfile);
        double nm = -1, it = -1;
        if (!yml_::scalar(t, "aruco_bc_nmarkers", &nm)) arucohip_throw_(ARUCOHIP_E_INVALID, "invalid file type", nullptr);
        yml_::scalar(t, "aruco_bc_mInfoType", &it);
        mInfoType = (int)it;
        ids.clear(), objPoints.clear();
        size_t p = yml_::top_key(t, "aruco_bc_markers");
        while (p != std::string::npos) {
            size_t q = t.find("id:", p);
            if (q == std::string::npos) break;
            ids.push_back((int)std::strtol(t.c_str() + q + 3, nullptr, 10));
            size_t c = t.find("corners:", q);
            if (c == std::string::npos) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardConfiguration: marker without corners", nullptr);
            size_t end = c;
            std::vector<double> v = yml_::numbers(t, c + 8, 12, &end);
            if (v.size() != 12) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardConfiguration: a marker needs 4 corners", nullptr);
            std::vector<cv::Point3f> pts(4);
            for (int k = 0; k < 4; k++) pts[k] = cv::Point3f((float)v[3 * k], (float)v[3 * k + 1], (float)v[3 * k + 2]);
            objPoints.push_back(pts);
            p = end;
        }
        if ((int)ids.size() != (int)nm) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardConfiguration: aruco_bc_nmarkers does not match the marker list", nullptr);
    }
    // board.cpp:45-49 + src/serialization.cpp:60-92: the file readFromFile reads back (values printed exactly)
    void saveToFile(const std::string& sfile) const {
        std::ofstream f(sfile.c_str());
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + sfile).c_str(), nullptr);
        char num[48];
        f << "%YAML:1.0\naruco_bc_nmarkers: " << ids.size() << "\naruco_bc_mInfoType: " << mInfoType << "\naruco_bc_markers:\n";
        for (size_t i = 0; i < ids.size(); i++) {
            f << "   - { id:" << ids[i] << ", corners:[ ";
            for (size_t c = 0; c < objPoints[i].size(); c++) {
                const cv::Point3f& p = objPoints[i][c];
                f << (c ? ", [ " : "[ ");
                const float v[3] = {p.x, p.y, p.z};
                for (int k = 0; k < 3; k++) {
                    std::snprintf(num, sizeof(num), "%.9g", (double)v[k]);
                    f << num << (k < 2 ? ", " : " ]");
                }
            }
            f << " ] }\n";
        }
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + sfile).c_str(), nullptr);
    }
    bool isExpressedInMeters() const { return mInfoType == METERS; }
    bool isExpressedInPixels() const { return mInfoType == PIX; }
    const std::vector<cv::Point3f>& getMarkerInfo(int id) const {  // board.cpp:60-66
        for (size_t i = 0; i < ids.size(); i++)
            if (ids[i] == id) return objPoints[i];
        arucohip_throw_(ARUCOHIP_E_INVALID, "BoardConfiguration::getMarkerInfo: marker with the id given is not found", nullptr);
        return objPoints[0];
    }
};

class Board : public std::vector<Marker> {
public:
    BoardConfiguration conf;
    cv::Mat_<double> Rvec, Tvec;
    void glGetModelViewMatrix(double modelview_matrix[16]) const { arucohip_gl_modelview_(Rvec, Tvec, modelview_matrix); }              // board.h:109
    void OgreGetPoseParameters(double position[3], double orientation[4]) const { arucohip_ogre_pose_(Rvec, Tvec, position, orientation); }  // board.h:123
    // board.h:99 Board::draw: Marker::draw of every member marker, on the device (DeviceDrawing::draw); colour as B, G, R
    inline void draw(cv::Mat& im, unsigned char b, unsigned char g, unsigned char r, int lineWidth = 1, bool writeId = true) const;
#if ARUCOHIP_HAVE_OPENCV
    void draw(cv::Mat& im, cv::Scalar color, int lineWidth = 1, bool writeId = true) const {
        draw(im, (unsigned char)color[0], (unsigned char)color[1], (unsigned char)color[2], lineWidth, writeId);
    }
#endif
};

// a Board as the batched calls take it: the pose when it carries one (Rvec and Tvec), has_pose = 0 otherwise
inline arucohip_board_t board_record_(const Board& B) {
    arucohip_board_t b;
    std::memset(&b, 0, sizeof(b));
    b.n_markers = (int32_t)B.size();
    if (!B.Rvec.empty() && !B.Tvec.empty()) {
        b.has_pose = 1;
        for (int k = 0; k < 3; k++) b.rvec[k] = B.Rvec(k), b.tvec[k] = B.Tvec(k);
    }
    return b;
}

// Marker::draw, Board::draw and CvDrawingUtils::draw3dAxis / draw3dCube through the device overlay pass (arucohip_draw_markers_batch /
// arucohip_draw_boards_batch on the process-wide handle): the frame goes up, is painted and comes back. The reference's primitives, order,
// colours and geometry; lines are not antialiased and the text uses the library's bitmap font (INTEGRATION.md "drawing"). 8-bit frames
// with 1 or 3 (B G R) channels. A caller that keeps its frames on the device calls the C ABI directly and copies nothing.
class DeviceDrawing {
public:
    // flags: ARUCOHIP_DRAW_*; CP is needed for AXIS / CUBE
    static void draw(cv::Mat& image, const std::vector<Marker>& markers, int flags = ARUCOHIP_DRAW_OUTLINE | ARUCOHIP_DRAW_IDS, int lineWidth = 1,
                     unsigned char b = 0, unsigned char g = 0, unsigned char r = 255, const CameraParameters* CP = nullptr) {
        if (markers.empty()) return;
        std::vector<arucohip_marker_t> m(markers.size());
        for (size_t i = 0; i < markers.size(); i++) markers[i].to_abi(&m[i]);
        const int32_t n = (int32_t)m.size();
        const arucohip_overlay_t st = {flags, lineWidth, {b, g, r, 0}};
        float K[9], d[8];
        const bool hasK = CP && mat_to_K_(CP->CameraMatrix, K);
        const int nd = CP ? mat_to_dist_(CP->Distorsion, d) : 0;
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure(image.cols, image.rows);
        arucohip_throw_(arucohip_draw_markers_batch(h, image.data, 1, image.cols, image.rows, channels_(image), (size_t)image.step,
                                                    (size_t)image.step * image.rows, 0, m.data(), n, &n, 0, hasK ? K : nullptr, nd ? d : nullptr, nd, &st),
                        "DeviceDrawing::draw", h);
    }
    static void draw3dAxis(cv::Mat& image, const Marker& m, const CameraParameters& CP) {
        draw(image, std::vector<Marker>(1, m), ARUCOHIP_DRAW_AXIS, 1, 0, 0, 255, &CP);
    }
    static void draw3dCube(cv::Mat& image, const Marker& m, const CameraParameters& CP, bool setYperpendicular = false) {
        draw(image, std::vector<Marker>(1, m), ARUCOHIP_DRAW_CUBE | (setYperpendicular ? ARUCOHIP_DRAW_Y_PERPENDICULAR : 0), 1, 0, 0, 255, &CP);
    }
    static void draw3dAxis(cv::Mat& image, const Board& B, const CameraParameters& CP) { board_(image, B, CP, ARUCOHIP_DRAW_AXIS); }
    static void draw3dCube(cv::Mat& image, const Board& B, const CameraParameters& CP, bool setYperpendicular = false) {
        board_(image, B, CP, ARUCOHIP_DRAW_CUBE | (setYperpendicular ? ARUCOHIP_DRAW_Y_PERPENDICULAR : 0));
    }

private:
    static int channels_(const cv::Mat& image) {
        if (image.type() != CV_8UC1 && image.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "drawing: CV_8UC1 or CV_8UC3 frames", nullptr);
        return image.type() == CV_8UC3 ? 3 : 1;
    }
    static void board_(cv::Mat& image, const Board& B, const CameraParameters& CP, int flags) {
        if (B.empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "drawing: the board holds no marker (B[0].ssize is its scale)", nullptr);
        const arucohip_board_t b = board_record_(B);
        float K[9], d[8];
        const bool hasK = mat_to_K_(CP.CameraMatrix, K);
        const int nd = mat_to_dist_(CP.Distorsion, d);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure(image.cols, image.rows);
        arucohip_throw_(arucohip_draw_boards_batch(h, image.data, 1, image.cols, image.rows, channels_(image), (size_t)image.step,
                                                   (size_t)image.step * image.rows, 0, &b, 0, B[0].ssize, hasK ? K : nullptr, nd ? d : nullptr, nd, flags),
                        "DeviceDrawing::draw3d (board)", h);
    }
};
inline void Board::draw(cv::Mat& im, unsigned char b, unsigned char g, unsigned char r, int lineWidth, bool writeId) const {
    DeviceDrawing::draw(im, *this, ARUCOHIP_DRAW_OUTLINE | (writeId ? ARUCOHIP_DRAW_IDS : 0), lineWidth, b, g, r);
}

// The fronto-parallel view of the plane a board lies in (arucohip_board_rectify_batch on the process-wide handle): the frame goes up, is
// resampled through the board's pose and the camera, and the view comes back. No reference counterpart. 8-bit frames with 1 or 3 channels.
// A caller that keeps its frames on the device calls the C ABI directly, a whole batch at a time, and copies nothing.
class BoardRectifier {
public:
    BoardRectifier() { std::memset(&win_, 0, sizeof(win_)); }
    // The window: the board's bounding box plus `margin` at pxPerUnit output pixels per plane unit. The units are those of the pose:
    // metres for a PIX board with markerSize (as BoardDetector scales it), the board's own for a METERS board. flipY: boards whose y points up.
    void setWindow(const BoardConfiguration& bc, float markerSize, float pxPerUnit, float margin = 0.f, bool flipY = false) {
        std::vector<float> obj;
        for (const std::vector<cv::Point3f>& m : bc.objPoints) {
            if (m.size() != 4) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardRectifier::setWindow: a marker needs 4 corners", nullptr);
            for (const cv::Point3f& p : m) obj.push_back(p.x), obj.push_back(p.y), obj.push_back(p.z);
        }
        arucohip_throw_(arucohip_rectify_board_window(obj.data(), (int)bc.objPoints.size(), bc.mInfoType, markerSize, pxPerUnit, margin, flipY ? 1 : 0, &win_),
                        "BoardRectifier::setWindow: no board, or a window below 1 or above 16383 pixels", nullptr);
    }
    void setWindow(const arucohip_rectify_t& window) { win_ = window; }
    const arucohip_rectify_t& getWindow() const { return win_; }
    // the view of B's plane in `frame`; all zero when B carries no pose
    cv::Mat rectify(const cv::Mat& frame, const Board& B, const CameraParameters& CP) const {
        const int cn = channels_(frame);
        float K[9], d[8];
        const bool hasK = mat_to_K_(CP.CameraMatrix, K);
        const int nd = mat_to_dist_(CP.Distorsion, d);
        const arucohip_board_t b = board_record_(B);
        if (win_.out_width < 1 || win_.out_height < 1) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardRectifier::rectify: no window set", nullptr);
        cv::Mat out(win_.out_height, win_.out_width, frame.type());
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_board_rectify_batch(h, frame.data, 1, frame.cols, frame.rows, cn, (size_t)frame.step, (size_t)frame.step * frame.rows, 0, &b, 0,
                                                     hasK ? K : nullptr, nd ? d : nullptr, nd, &win_, out.data, (size_t)out.step,
                                                     (size_t)out.step * out.rows, 0, nullptr, nullptr),
                        "BoardRectifier::rectify", h);
        return out;
    }
    // frames[i] on the plane of boards[i]
    std::vector<cv::Mat> rectify(const std::vector<cv::Mat>& frames, const std::vector<Board>& boards, const CameraParameters& CP) const {
        if (frames.size() != boards.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardRectifier::rectify: one board per frame", nullptr);
        std::vector<cv::Mat> out;
        for (size_t i = 0; i < frames.size(); i++) out.push_back(rectify(frames[i], boards[i], CP));
        return out;
    }
    // cv::warpPerspective(src, dst, M, size, INTER_LINEAR | WARP_INVERSE_MAP, BORDER_CONSTANT 0) with every pixel projected in double
    // (arucohip_warp_plane_batch without a camera): dst (u, v) = src at M (u, v, 1). M: 3 x 3, CV_64F or CV_32F.
    static cv::Mat warpPerspectiveInverse(const cv::Mat& src, const cv::Mat& M, cv::Size size) {
        const int cn = channels_(src);
        if (M.rows != 3 || M.cols != 3 || (M.type() != CV_64FC1 && M.type() != CV_32FC1))
            arucohip_throw_(ARUCOHIP_E_INVALID, "warpPerspectiveInverse: M must be 3x3, CV_64F or CV_32F", nullptr);
        double m[9];
        for (int i = 0; i < 9; i++) m[i] = M.type() == CV_64FC1 ? M.at<double>(i / 3, i % 3) : (double)M.at<float>(i / 3, i % 3);
        if (size.width < 1 || size.height < 1) arucohip_throw_(ARUCOHIP_E_INVALID, "warpPerspectiveInverse: empty size", nullptr);
        cv::Mat out(size.height, size.width, src.type());
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_warp_plane_batch(h, src.data, 1, src.cols, src.rows, cn, (size_t)src.step, (size_t)src.step * src.rows, 0, m, nullptr, 0, nullptr,
                                                  nullptr, 0, out.data, size.width, size.height, (size_t)out.step, (size_t)out.step * out.rows, 0),
                        "warpPerspectiveInverse", h);
        return out;
    }

private:
    arucohip_rectify_t win_;
    static int channels_(const cv::Mat& image) {
        if (image.type() != CV_8UC1 && image.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "rectification: CV_8UC1 or CV_8UC3 frames", nullptr);
        return image.type() == CV_8UC3 ? 3 : 1;
    }
};

// A picture on the plane a board lies in (arucohip_board_composite_batch on the process-wide handle): the frame goes up, the texture is
// blended onto the board as the camera sees it and the frame comes back. No reference counterpart. 8-bit frames with 1 or 3 channels; the
// texture has the frame's channels, or one more (CV_8UC2 / CV_8UC4: the last is straight alpha), and the window's size. A caller that keeps
// its frames on the device calls the C ABI directly, a whole batch at a time, and copies nothing.
class BoardCompositor {
public:
    // The window the texture covers, as BoardRectifier::setWindow defines it: texel (s, t) lies where output pixel (s, t) of the rectified view lies.
    void setWindow(const BoardConfiguration& bc, float markerSize, float pxPerUnit, float margin = 0.f, bool flipY = false) {
        rect_.setWindow(bc, markerSize, pxPerUnit, margin, flipY);
    }
    void setWindow(const arucohip_rectify_t& window) { rect_.setWindow(window); }
    const arucohip_rectify_t& getWindow() const { return rect_.getWindow(); }
    // texture onto B's plane in `frame`, in place; nothing where mask (CV_8UC1, the frame's size; empty: none) is 0, nothing at all when B
    // carries no pose
    void paint(cv::Mat& frame, const Board& B, const CameraParameters& CP, const cv::Mat& texture, int opacity = 255, const cv::Mat& mask = cv::Mat()) const {
        const int cn = frame.type() == CV_8UC3 ? 3 : 1, tcn = texture_channels_(texture);
        if (frame.type() != CV_8UC1 && frame.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "compositing: CV_8UC1 or CV_8UC3 frames", nullptr);
        if (!mask.empty() && (mask.type() != CV_8UC1 || mask.rows != frame.rows || mask.cols != frame.cols))
            arucohip_throw_(ARUCOHIP_E_INVALID, "compositing: the mask is CV_8UC1 of the frame's size", nullptr);
        float K[9], d[8];
        const bool hasK = mat_to_K_(CP.CameraMatrix, K);
        const int nd = mat_to_dist_(CP.Distorsion, d);
        const arucohip_board_t b = board_record_(B);
        const arucohip_texture_t tex = {texture.data, texture.cols, texture.rows, tcn, 0, (size_t)texture.step, 0, opacity, 0};
        std::vector<unsigned char> packed;   // the C call takes masks tightly packed
        for (int y = 0; y < mask.rows; y++) packed.insert(packed.end(), mask.data + (size_t)y * (size_t)mask.step, mask.data + (size_t)y * (size_t)mask.step + mask.cols);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_board_composite_batch(h, frame.data, 1, frame.cols, frame.rows, cn, (size_t)frame.step, (size_t)frame.step * frame.rows, 0, &b, 0,
                                                       hasK ? K : nullptr, nd ? d : nullptr, nd, &rect_.getWindow(), &tex, mask.empty() ? nullptr : packed.data(), 0,
                                                       nullptr, nullptr),
                        "BoardCompositor::paint", h);
    }
    // texture onto the plane of boards[i] in frames[i]; masks: empty, or one per frame
    void paint(std::vector<cv::Mat>& frames, const std::vector<Board>& boards, const CameraParameters& CP, const cv::Mat& texture, int opacity = 255,
               const std::vector<cv::Mat>& masks = std::vector<cv::Mat>()) const {
        if (frames.size() != boards.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardCompositor::paint: one board per frame", nullptr);
        if (!masks.empty() && masks.size() != frames.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "BoardCompositor::paint: no masks, or one per frame", nullptr);
        for (size_t i = 0; i < frames.size(); i++) paint(frames[i], boards[i], CP, texture, opacity, masks.empty() ? cv::Mat() : masks[i]);
    }

private:
    BoardRectifier rect_;
    static int texture_channels_(const cv::Mat& t) {
#if ARUCOHIP_HAVE_OPENCV
        if (!t.empty() && t.depth() == CV_8U) return t.channels();
#else   // the stand-in Mat has no 2- or 4-channel type: no alpha without OpenCV
        if (!t.empty() && (t.type() == CV_8UC1 || t.type() == CV_8UC3)) return (int)t.elemSize();
#endif
        arucohip_throw_(ARUCOHIP_E_INVALID, "compositing: an 8-bit texture", nullptr);
        return 0;
    }
};

// A triangle mesh in the object frame of a pose: what the reference's aruco_test_gl applications hand to OpenGL as glut solids.
// triangles are vertex indices, counter-clockwise seen from outside (right-handed); colors is empty (one colour for all) or holds
// B G R per triangle.
struct Mesh {
    std::vector<float> vertices;          // 3 per vertex
    std::vector<int32_t> triangles;       // 3 per triangle
    std::vector<unsigned char> colors;    // empty, or 3 per triangle
    size_t nverts() const { return vertices.size() / 3; }
    size_t ntris() const { return triangles.size() / 3; }
    // the unit cube standing on the pose's plane: [-0.5, 0.5]^2 x [0, 1], 8 vertices, 12 triangles
    static Mesh cube() {
        Mesh m;
        for (int i = 0; i < 8; i++) {
            m.vertices.push_back((i & 1) ? 0.5f : -0.5f), m.vertices.push_back((i & 2) ? 0.5f : -0.5f), m.vertices.push_back((i & 4) ? 1.f : 0.f);
        }
        static const int q[6][4] = {{0, 2, 3, 1}, {4, 5, 7, 6}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 4, 6, 2}, {1, 3, 7, 5}};
        for (int f = 0; f < 6; f++) m.quad_(q[f][0], q[f][1], q[f][2], q[f][3]);
        return m;
    }
    // a latitude / longitude sphere of the given radius about `center`: 2 + (stacks - 1) * slices vertices, 2 * slices * (stacks - 1) triangles
    static Mesh uvSphere(int stacks, int slices, float radius = 0.5f, float cx = 0.f, float cy = 0.f, float cz = 0.5f) {
        if (stacks < 2 || slices < 3) arucohip_throw_(ARUCOHIP_E_INVALID, "Mesh::uvSphere: at least 2 stacks and 3 slices", nullptr);
        const double pi = 3.14159265358979323846;
        Mesh m;
        auto add = [&](double x, double y, double z) {
            m.vertices.push_back((float)(x * radius + cx)), m.vertices.push_back((float)(y * radius + cy)), m.vertices.push_back((float)(z * radius + cz));
        };
        add(0, 0, 1);
        for (int i = 1; i < stacks; i++)
            for (int j = 0; j < slices; j++) {
                const double th = pi * i / stacks, ph = 2 * pi * j / slices;
                add(std::sin(th) * std::cos(ph), std::sin(th) * std::sin(ph), std::cos(th));
            }
        add(0, 0, -1);
        auto ring = [&](int i, int j) { return 1 + (i - 1) * slices + j % slices; };
        const int south = (int)m.nverts() - 1;
        for (int j = 0; j < slices; j++) {
            m.tri_(0, ring(1, j), ring(1, j + 1));
            for (int i = 1; i < stacks - 1; i++) m.quad_(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1), ring(i, j + 1));
            m.tri_(south, ring(stacks - 1, j + 1), ring(stacks - 1, j));
        }
        return m;
    }
    arucohip_mesh_t abi() const {
        arucohip_mesh_t a;
        std::memset(&a, 0, sizeof(a));
        a.vertices = vertices.data(), a.triangles = triangles.data(), a.colors = colors.empty() ? nullptr : colors.data();
        a.nverts = (int32_t)nverts(), a.ntris = (int32_t)ntris();
        return a;
    }

private:
    void tri_(int a, int b, int c) { triangles.push_back(a), triangles.push_back(b), triangles.push_back(c); }
    void quad_(int a, int b, int c, int d) { tri_(a, b, c), tri_(a, c, d); }
};

// Solid objects at marker and board poses (arucohip_render_markers_batch / arucohip_render_boards_batch on the process-wide handle):
// the frame goes up, the mesh is drawn flat-shaded with a depth test and the frame comes back. What aruco_test_gl, aruco_test_board_gl
// and aruco_test_board_gl_mask do through OpenGL; the pixel rule is the library's own (arucohip.h). 8-bit frames with 1 or 3 (B G R)
// channels. A caller that keeps its frames on the device calls the C ABI directly, a whole batch at a time, and copies nothing.
class MeshRenderer {
public:
    MeshRenderer() { arucohip_default_render(&style_); }
    arucohip_render_t& style() { return style_; }
    const arucohip_render_t& style() const { return style_; }
    // the mesh on every marker that carries a pose, in units of the marker's side; nothing where mask (CV_8UC1, the frame's size; empty: none) is 0
    void draw(cv::Mat& image, const std::vector<Marker>& markers, const CameraParameters& CP, const Mesh& mesh, const cv::Mat& mask = cv::Mat()) const {
        if (markers.empty()) return;
        std::vector<arucohip_marker_t> m(markers.size());
        for (size_t i = 0; i < markers.size(); i++) markers[i].to_abi(&m[i]);
        const int32_t n = (int32_t)m.size();
        Call_ c(image, CP, mesh, mask);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure(image.cols, image.rows);
        arucohip_throw_(arucohip_render_markers_batch(h, image.data, 1, image.cols, image.rows, c.cn, (size_t)image.step, (size_t)image.step * image.rows, 0,
                                                      m.data(), n, &n, 0, c.hasK ? c.K : nullptr, c.nd ? c.d : nullptr, c.nd, &c.mesh, &style_, c.mask(), 0),
                        "MeshRenderer::draw", h);
    }
    // the mesh at the board's pose, in the units the pose was solved in (style().scale sizes it); nothing at all when B carries no pose
    void draw(cv::Mat& image, const Board& B, const CameraParameters& CP, const Mesh& mesh, const cv::Mat& mask = cv::Mat()) const {
        const arucohip_board_t b = board_record_(B);
        Call_ c(image, CP, mesh, mask);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure(image.cols, image.rows);
        arucohip_throw_(arucohip_render_boards_batch(h, image.data, 1, image.cols, image.rows, c.cn, (size_t)image.step, (size_t)image.step * image.rows, 0, &b, 0,
                                                     c.hasK ? c.K : nullptr, c.nd ? c.d : nullptr, c.nd, &c.mesh, &style_, c.mask(), 0),
                        "MeshRenderer::draw (board)", h);
    }

private:
    arucohip_render_t style_;
    // the arguments both forms share
    struct Call_ {
        int cn, nd;
        bool hasK;
        float K[9], d[8];
        arucohip_mesh_t mesh;
        std::vector<unsigned char> packed;   // the C call takes masks tightly packed
        bool masked;
        Call_(const cv::Mat& image, const CameraParameters& CP, const Mesh& m, const cv::Mat& msk) : mesh(m.abi()), masked(!msk.empty()) {
            if (image.type() != CV_8UC1 && image.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "rendering: CV_8UC1 or CV_8UC3 frames", nullptr);
            if (masked && (msk.type() != CV_8UC1 || msk.rows != image.rows || msk.cols != image.cols))
                arucohip_throw_(ARUCOHIP_E_INVALID, "rendering: the mask is CV_8UC1 of the frame's size", nullptr);
            if (m.vertices.size() % 3 || m.triangles.size() % 3 || (!m.colors.empty() && m.colors.size() != m.triangles.size()))
                arucohip_throw_(ARUCOHIP_E_INVALID, "rendering: a mesh has 3 floats per vertex, 3 indices and no or 3 colour bytes per triangle", nullptr);
            cn = image.type() == CV_8UC3 ? 3 : 1;
            hasK = mat_to_K_(CP.CameraMatrix, K);
            nd = mat_to_dist_(CP.Distorsion, d);
            for (int y = 0; y < msk.rows; y++)
                packed.insert(packed.end(), msk.data + (size_t)y * (size_t)msk.step, msk.data + (size_t)y * (size_t)msk.step + msk.cols);
        }
        const unsigned char* mask() const { return masked ? packed.data() : nullptr; }
    };
};
#if ARUCOHIP_HAVE_OPENCV && defined(ARUCOHIP_SHIM_DEFINE_DRAWING)
// The reference's drawing names, defined through the device overlay. Off by default: an integration that keeps the reference's own
// src/marker.cpp / src/cvdrawingutils.{h,cpp} (or any other definition of these names) must not define the macro.
inline void Marker::draw(cv::Mat& in, cv::Scalar color, int lineWidth, bool writeId) const {
    if (size() != 4) return;
    DeviceDrawing::draw(in, std::vector<Marker>(1, *this), ARUCOHIP_DRAW_OUTLINE | (writeId ? ARUCOHIP_DRAW_IDS : 0), lineWidth, (unsigned char)color[0],
                        (unsigned char)color[1], (unsigned char)color[2]);
}
class CvDrawingUtils {
public:
    static void draw3dAxis(cv::Mat& Image, Marker& m, const CameraParameters& CP) { DeviceDrawing::draw3dAxis(Image, m, CP); }
    static void draw3dCube(cv::Mat& Image, Marker& m, const CameraParameters& CP, bool setYperpendicular = false) {
        DeviceDrawing::draw3dCube(Image, m, CP, setYperpendicular);
    }
    static void draw3dAxis(cv::Mat& Image, Board& B, const CameraParameters& CP) { DeviceDrawing::draw3dAxis(Image, B, CP); }
    static void draw3dCube(cv::Mat& Image, Board& B, const CameraParameters& CP, bool setYperpendicular = false) {
        DeviceDrawing::draw3dCube(Image, B, CP, setYperpendicular);
    }
};
#endif

// ---- marker-id decoders (markerdetector.h:248 setMakerDetectorFunction). On the accelerated path the decoders run on the
// device; the static functions below are the tokens a caller passes to MarkerDetector::setMakerDetectorFunction.
class FiducidalMarkers {
public:
    // arucofidmarkers.h:84 — the default decoder (5x5 Hamming markers)
    static int detect(const cv::Mat&, int&) {
        arucohip_throw_(ARUCOHIP_E_UNSUPPORTED, "FiducidalMarkers::detect runs on the device; pass it to setMakerDetectorFunction", nullptr);
        return -1;
    }
    // arucofidmarkers.h:82-130 / .cpp:214-430 on the device (arucohip_fiducial_*), through the process-wide handle.
    // createMarkerImage: writeIdWaterMark is accepted and ignored, the "#id" text is not drawn.
    static cv::Mat createMarkerImage(int id, int size, bool writeIdWaterMark = true, bool locked = false) {
        (void)writeIdWaterMark;
        const int side = arucohip_fiducial_marker_side(size, locked ? 1 : 0);
        if (!side || id < 0 || id >= 1024) arucohip_throw_(ARUCOHIP_E_INVALID, "createMarkerImage: 0 <= id < 1024, 7 <= size, side <= 16383", nullptr);
        cv::Mat img(side, side, CV_8UC1);
        const int32_t id32 = id;
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_fiducial_marker_images(h, &id32, 1, size, locked ? 1 : 0, img.data, img.step, 0, 0), "createMarkerImage", h);
        return img;
    }
    static cv::Mat getMarkerMat(int id) {   // 5 x 5 CV_8UC1 of 0 / 1
        unsigned char cells[25];
        arucohip_throw_(arucohip_fiducial_marker_mat(id, cells), "getMarkerMat: invalid marker id", nullptr);
        cv::Mat m(5, 5, CV_8UC1);
        for (int y = 0; y < 5; y++)
            for (int x = 0; x < 5; x++) m.at<unsigned char>(y, x) = cells[5 * y + x];
        return m;
    }
    // The ids come from cv::theRNG() as in the reference: consecutive calls continue one stream. The panel form resizes TInfo.objPoints
    // and assigns TInfo.ids; the other two append to what TInfo held.
    static cv::Mat createBoardImage(cv::Size gridSize, int MarkerSize, int MarkerDistance, BoardConfiguration& TInfo,
                                    const std::vector<int>& excludedIds = std::vector<int>()) {
        return board_(0, gridSize, MarkerSize, MarkerDistance, TInfo, true, excludedIds);
    }
    static cv::Mat createBoardImage_ChessBoard(cv::Size gridSize, int MarkerSize, BoardConfiguration& TInfo, bool setDataCentered = true,
                                               const std::vector<int>& excludedIds = std::vector<int>()) {
        return board_(1, gridSize, MarkerSize, 0, TInfo, setDataCentered, excludedIds);
    }
    static cv::Mat createBoardImage_Frame(cv::Size gridSize, int MarkerSize, int MarkerDistance, BoardConfiguration& TInfo, bool setDataCentered = true,
                                          const std::vector<int>& excludedIds = std::vector<int>()) {
        return board_(2, gridSize, MarkerSize, MarkerDistance, TInfo, setDataCentered, excludedIds);
    }

private:
    static cv::Mat board_(int type, cv::Size grid, int size, int dist, BoardConfiguration& TInfo, bool centered, const std::vector<int>& excluded) {
        int w = 0, hgt = 0, drawn = 0, nm = 0;
        arucohip_throw_(arucohip_fiducial_board_size(type, grid.width, grid.height, size, dist, &w, &hgt, &drawn, &nm), "createBoardImage", nullptr);
        std::vector<int32_t> ex(excluded.begin(), excluded.end()), ids((size_t)drawn);
        uint64_t state = (uint64_t)cv::theRNG().state;
        arucohip_throw_(arucohip_fiducial_shuffle_ids(&state, drawn, ex.data(), (int)ex.size(), ids.data()),
                        "createBoardImage: number of possible markers is exceeded", nullptr);
        cv::theRNG().state = state;
        cv::Mat img(hgt, w, CV_8UC1);
        std::vector<float> obj((size_t)nm * 12);
        {
            SharedHandle_& sh = SharedHandle_::get();
            std::lock_guard<std::mutex> lock(sh.mu);
            arucohip_handle* h = sh.ensure();
            arucohip_throw_(arucohip_fiducial_board_image(h, type, grid.width, grid.height, size, dist, centered ? 1 : 0, ids.data(), drawn, img.data,
                                                          img.step, 0, obj.data()),
                            "createBoardImage", h);
        }
        TInfo.mInfoType = BoardConfiguration::PIX;
        if (type == 0) TInfo.ids.clear(), TInfo.objPoints.clear();
        for (int i = 0; i < nm; i++) {
            TInfo.ids.push_back(ids[i]);
            std::vector<cv::Point3f> c(4);
            for (int k = 0; k < 4; k++) c[k] = cv::Point3f(obj[12 * i + 3 * k], obj[12 * i + 3 * k + 1], obj[12 * i + 3 * k + 2]);
            TInfo.objPoints.push_back(c);
        }
        return img;
    }
};

// highlyreliablemarkers.h:50-140 / .cpp:120-260: an n x n code in its four rotations with their ids. Small host arithmetic.
class MarkerCode {
public:
    explicit MarkerCode(unsigned int n = 0) : _n(n) {
        for (int r = 0; r < 4; r++) _bits[r].assign((size_t)n * n, false), _ids[r] = 0;
    }
    // MarkerCode::set (:149-182): an n x n CV_8U matrix, non-zero = 1
    void set(const cv::Mat& code) {
        if (code.rows != (int)_n || code.cols != (int)_n) arucohip_throw_(ARUCOHIP_E_INVALID, "MarkerCode::set: the code must be n x n", nullptr);
        uint64_t c = 0;
        for (unsigned int y = 0; y < _n; y++)
            for (unsigned int x = 0; x < _n; x++)
                if (code.at<unsigned char>((int)y, (int)x)) c |= 1ull << (y * _n + x);
        set_code_(c);
    }
    void fromString(const std::string& s) {
        uint64_t c = 0;
        for (size_t i = 0; i < s.size() && i < (size_t)_n * _n; i++)
            if (s[i] == '1') c |= 1ull << i;
        set_code_(c);
    }
    std::string toString() const {
        std::string s(size(), '0');
        for (unsigned int i = 0; i < size(); i++)
            if (get(i)) s[i] = '1';
        return s;
    }
    unsigned int n() const { return _n; }
    unsigned int size() const { return _n * _n; }
    bool get(unsigned int pos) const { return _bits[0][pos]; }
    // sum of 2 << pos over the 1 bits of rotation rot. For n >= 6 the reference's int shift passes 32 bits (undefined); here the bits
    // past 32 are dropped.
    unsigned int getId(unsigned int rot = 0) const { return _ids[rot]; }
    const std::vector<bool>& getRotation(unsigned int rot) const { return _bits[rot]; }
    // :184-194: min over rotations 1..3 of the Hamming distance to rotation 0
    unsigned int selfDistance(unsigned int& minRot) const {
        unsigned int res = size();
        for (unsigned int i = 1; i < 4; i++) {
            const unsigned int d = hamming_(_bits[0], _bits[i]);
            if (d < res) minRot = i, res = d;
        }
        return res;
    }
    unsigned int selfDistance() const {
        unsigned int r = 0;
        return selfDistance(r);
    }
    // :198-208: min over the rotations of m of the Hamming distance to this code's rotation 0
    unsigned int distance(const MarkerCode& m, unsigned int& minRot) const {
        unsigned int res = size();
        for (unsigned int i = 0; i < 4; i++) {
            const unsigned int d = hamming_(_bits[0], m.getRotation(i));
            if (d < res) minRot = i, res = d;
        }
        return res;
    }
    unsigned int distance(const MarkerCode& m) const {
        unsigned int r = 0;
        return distance(m, r);
    }
    // :234-260: pixSize rounded up to a multiple of n + 2, black border, white = bit 1
    cv::Mat getImg(unsigned int pixSize) const {
        const unsigned int nrows = _n + 2;
        if (pixSize % nrows != 0) pixSize = pixSize + nrows - pixSize % nrows;
        const unsigned int cell = pixSize / nrows;
        cv::Mat img = cv::Mat::zeros((int)pixSize, (int)pixSize, CV_8UC1);
        for (unsigned int i = 0; i < _n; i++)
            for (unsigned int j = 0; j < _n; j++)
                if (_bits[0][i * _n + j])
                    for (unsigned int k = 0; k < cell; k++)
                        for (unsigned int l = 0; l < cell; l++) img.at<unsigned char>((int)((i + 1) * cell + k), (int)((j + 1) * cell + l)) = 255;
        return img;
    }
    // rotation 0 in arucohip_set_dictionary's layout (bit y * n + x)
    uint64_t code_() const {
        uint64_t c = 0;
        for (unsigned int i = 0; i < size(); i++)
            if (_bits[0][i]) c |= 1ull << i;
        return c;
    }

private:
    static unsigned int hamming_(const std::vector<bool>& a, const std::vector<bool>& b) {
        unsigned int r = 0;
        for (size_t i = 0; i < a.size(); i++) r += a[i] != b[i];
        return r;
    }
    void set_code_(uint64_t c) {
        for (int r = 0; r < 4; r++) _bits[r].assign((size_t)_n * _n, false), _ids[r] = 0;
        for (unsigned int y = 0; y < _n; y++)
            for (unsigned int x = 0; x < _n; x++) {
                const bool v = (c >> (y * _n + x)) & 1;
                for (int r = 0; r < 4; r++) {
                    unsigned int ry = y, rx = x;
                    if (r == 1) ry = x, rx = _n - y - 1;
                    else if (r == 2) ry = _n - y - 1, rx = _n - x - 1;
                    else if (r == 3) ry = _n - x - 1, rx = y;
                    const unsigned int pos = ry * _n + rx;
                    _bits[r][pos] = v;
                    if (v) _ids[r] |= (unsigned int)(2ull << pos);
                }
            }
    }
    unsigned int _n;
    std::vector<bool> _bits[4];
    unsigned int _ids[4];
};

// highlyreliablemarkers.h:150-190; fromFile / toFile: the reference's dictionary files (src/serialization.cpp:123-150:
// nmarkers, markersize, tau0, marker_<i>: "<n*n bits>")
class Dictionary : public std::vector<MarkerCode> {
public:
    int tau0 = 0;
    bool fromFile(const std::string& filename) {
        std::ifstream f(filename.c_str());
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, "Dictionary::fromFile: cannot open file", nullptr);
        clear();
        unsigned int n = 0;
        size_t nmarkers = 0;
        std::vector<std::pair<size_t, std::string> > codes;
        std::string line;
        while (std::getline(f, line)) {
            size_t c = line.find(':');
            if (c == std::string::npos || line[0] == '%') continue;
            std::string key = line.substr(0, c), val = line.substr(c + 1);
            key.erase(0, key.find_first_not_of(" \t"));
            val.erase(0, val.find_first_not_of(" \t\""));
            val.erase(val.find_last_not_of(" \t\"\r") + 1);
            if (key == "nmarkers") nmarkers = (size_t)std::atol(val.c_str());
            else if (key == "markersize") n = (unsigned int)std::atol(val.c_str());
            else if (key == "tau0") tau0 = std::atoi(val.c_str());
            else if (key.compare(0, 7, "marker_") == 0) codes.push_back(std::make_pair((size_t)std::atol(key.c_str() + 7), val));
        }
        if (n == 0 || codes.size() != nmarkers) arucohip_throw_(ARUCOHIP_E_INVALID, "Dictionary::fromFile: malformed dictionary", nullptr);
        resize(nmarkers, MarkerCode(n));
        for (size_t i = 0; i < codes.size(); i++) {
            if (codes[i].first >= nmarkers || codes[i].second.size() != (size_t)n * n)
                arucohip_throw_(ARUCOHIP_E_INVALID, "Dictionary::fromFile: malformed marker", nullptr);
            (*this)[codes[i].first].fromString(codes[i].second);
        }
        return true;
    }
    // :268-274 (serialization.cpp:123-133): the file fromFile reads back
    bool toFile(const std::string& filename) {
        if (empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "Dictionary::toFile: empty dictionary", nullptr);
        std::ofstream f(filename.c_str());
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + filename).c_str(), nullptr);
        f << "%YAML:1.0\nnmarkers: " << size() << "\nmarkersize: " << (*this)[0].n() << "\ntau0: " << tau0 << "\n";
        for (size_t i = 0; i < size(); i++) f << "marker_" << i << ": \"" << (*this)[i].toString() << "\"\n";
        if (!f) arucohip_throw_(ARUCOHIP_E_INVALID, ("cannot write " + filename).c_str(), nullptr);
        return true;
    }
    // :277-289: min over the markers of MarkerCode::distance; m.size() when empty
    unsigned int distance(const MarkerCode& m, unsigned int& minMarker, unsigned int& minRot) {
        unsigned int res = m.size();
        for (unsigned int i = 0; i < size(); i++) {
            unsigned int r = 0;
            const unsigned int d = (*this)[i].distance(m, r);
            if (d < res) minMarker = i, minRot = r, res = d;
        }
        return res;
    }
    unsigned int distance(const MarkerCode& m) {
        unsigned int a = 0, b = 0;
        return distance(m, a, b);
    }
    // :293-308
    unsigned int minimunDistance() {
        if (empty()) return 0;
        unsigned int best = (*this)[0].size();
        for (size_t i = 0; i < size(); i++) {
            best = std::min(best, (*this)[i].selfDistance());
            for (size_t j = i + 1; j < size(); j++) best = std::min(best, (*this)[i].distance((*this)[j]));
        }
        return best;
    }
};

// highlyreliablemarkers.h:196-260: static dictionary + decoder token, dictionary and board generation
class HighlyReliableMarkers {
public:
    static bool loadDictionary(Dictionary D, float correctionDistanceRate = 1) {  // highlyreliablemarkers.cpp:311-322
        if (D.size() == 0) return false;
        State_& s = state_();
        s.D = D, s.rate = correctionDistanceRate, s.version++;
        return true;
    }
    static bool loadDictionary(const std::string& filename, float correctionDistance = 1) {
        Dictionary D;
        D.fromFile(filename);
        return loadDictionary(D, correctionDistance);
    }
    static int detect(const cv::Mat&, int&) {
        arucohip_throw_(ARUCOHIP_E_UNSUPPORTED, "HighlyReliableMarkers::detect runs on the device; pass it to setMakerDetectorFunction", nullptr);
        return -1;
    }
    // :567-608 on the device (arucohip_hrm_create_dictionary). The reference continues the caller's glibc rand() state; this one takes
    // its seed from one std::rand() call. The three-argument form equals the reference run right after srand(seed).
    static Dictionary createDicitionary(size_t dictSize, size_t n) { return createDicitionary(dictSize, n, (unsigned int)std::rand()); }
    static Dictionary createDicitionary(size_t dictSize, size_t n, unsigned int seed) {
        if (n < 3 || n > 8 || dictSize < 1 || dictSize > 4096)
            arucohip_throw_(ARUCOHIP_E_INVALID, "createDicitionary: n must be 3..8 and dictSize 1..4096", nullptr);
        std::vector<uint64_t> codes(dictSize);
        int tau = 0;
        SharedHandle_& sh = SharedHandle_::get();
        {
            std::lock_guard<std::mutex> lock(sh.mu);
            arucohip_handle* h = sh.ensure();
            arucohip_throw_(arucohip_hrm_create_dictionary(h, (int)n, (int)dictSize, seed, codes.data(), &tau, nullptr), "createDicitionary", h);
        }
        Dictionary D;
        for (size_t i = 0; i < dictSize; i++) {
            MarkerCode m((unsigned int)n);
            std::string bits((size_t)n * n, '0');
            for (size_t b = 0; b < bits.size(); b++)
                if ((codes[i] >> b) & 1) bits[b] = '1';
            m.fromString(bits);
            D.push_back(m);
        }
        D.tau0 = tau;
        return D;
    }
    // :498-565 on the device (arucohip_hrm_board_image): BC gets PIX, and the markers' ids (getId()) and corners appended, as in the
    // reference. The ids are undefined there for n >= 6: cv::Exception here.
    static cv::Mat createBoardImage(cv::Size gridSize, const Dictionary& D, BoardConfiguration& BC, bool chromatic = false) {
        if (D.empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "createBoardImage: empty dictionary", nullptr);
        const int n = (int)D[0].n();
        int w = 0, hgt = 0, ch = 0;
        arucohip_throw_(arucohip_hrm_board_size(n, gridSize.width, gridSize.height, chromatic ? 1 : 0, &w, &hgt, &ch), "createBoardImage", nullptr);
        const int nb = gridSize.width * gridSize.height;
        std::vector<uint64_t> codes(D.size());
        for (size_t i = 0; i < D.size(); i++) codes[i] = D[i].code_();
        cv::Mat img(hgt, w, chromatic ? CV_8UC3 : CV_8UC1);
        std::vector<int32_t> ids((size_t)nb);
        std::vector<float> obj((size_t)nb * 12);
        SharedHandle_& sh = SharedHandle_::get();
        {
            std::lock_guard<std::mutex> lock(sh.mu);
            arucohip_handle* h = sh.ensure();
            arucohip_throw_(arucohip_hrm_board_image(h, n, (int)codes.size(), codes.data(), gridSize.width, gridSize.height, chromatic ? 1 : 0,
                                                     img.data, img.step, 0, ids.data(), obj.data()),
                            "createBoardImage", h);
        }
        BC.mInfoType = BoardConfiguration::PIX;
        for (int i = 0; i < nb; i++) {
            BC.ids.push_back(ids[i]);
            std::vector<cv::Point3f> MI(4);
            for (int k = 0; k < 4; k++) MI[k] = cv::Point3f(obj[12 * i + 3 * k], obj[12 * i + 3 * k + 1], obj[12 * i + 3 * k + 2]);
            BC.objPoints.push_back(MI);
        }
        return img;
    }
    struct State_ {
        Dictionary D;
        float rate = 1;
        int version = 0;
    };
    static State_& state_() {
        static State_ s;
        return s;
    }
};

class MarkerDetector {
public:
    // markerdetector.h:45-62: a candidate to be a marker = the marker (corners, id) + its contour + its position in the contour list.
    // (Private in the reference although refineCandidateLines, a public member, takes one; public here so that a caller can build one.)
    class MarkerCandidate : public Marker {
    public:
        MarkerCandidate() : idx(-1) {}
        MarkerCandidate(const Marker& M) : Marker(M), idx(-1) {}
        std::vector<cv::Point> contour;   // all the points of its contour
        int idx;                          // index position in the global contour list
    };
    enum ThresholdMethods { FIXED_THRES, ADPT_THRES, CANNY };
    enum CornerRefinementMethod { NONE, HARRIS, SUBPIX, LINES };

    explicit MarkerDetector(int device = 0) : h_(nullptr), device_(device), cap_w_(0), cap_h_(0) { arucohip_default_params(&p_); }
    ~MarkerDetector() { arucohip_destroy(h_); }
    MarkerDetector(const MarkerDetector&) = delete;
    MarkerDetector& operator=(const MarkerDetector&) = delete;

    // markerdetector.h:102-103
    void detect(const cv::Mat& input, std::vector<Marker>& detectedMarkers, cv::Mat camMatrix = cv::Mat(), cv::Mat distCoeff = cv::Mat(),
                float markerSizeMeters = -1, bool setYPerpendicular = false) {
        // markerdetector.cpp:303-310: 8-bit gray frames are used as they are, 3-channel frames are BGR and converted (on the device)
        if (input.type() != CV_8UC1 && input.type() != CV_8UC3)
            arucohip_throw_(ARUCOHIP_E_INVALID, "detect: 8-bit gray (CV_8UC1) or BGR (CV_8UC3) frames", nullptr);
        ensure_(input.cols, input.rows);
        if (hrm_ && hrm_version_ != HighlyReliableMarkers::state_().version) apply_decoder_();
        float K[9], d[8];
        bool hasK = mat_to_K_(camMatrix, K);
        int nd = mat_to_dist_(distCoeff, d);
        std::vector<arucohip_marker_t>& out = out_;   // the detector's own result buffer: a frame loop allocates nothing per call
        if (out.size() < 256) out.resize(256);
        int n = 0, rc;
        for (int attempt = 0;; attempt++) {
            rc = input.type() == CV_8UC3
                     ? arucohip_detect_bgr(h_, input.data, input.cols, input.rows, input.step, hasK ? K : nullptr, nd ? d : nullptr, nd, markerSizeMeters,
                                           setYPerpendicular ? 1 : 0, out.data(), (int)out.size(), &n)
                     : arucohip_detect(h_, input.data, input.cols, input.rows, input.step, hasK ? K : nullptr, nd ? d : nullptr, nd, markerSizeMeters,
                                       setYPerpendicular ? 1 : 0, out.data(), (int)out.size(), &n);
            // a cluttered frame can outgrow the device lists; the reference has no such limit, so the lists are doubled and the
            // frame is detected again instead of failing
            if (rc != ARUCOHIP_E_OVERFLOW || attempt >= 5) break;
            grow_++;
            recreate_();
        }
        arucohip_throw_(rc, "MarkerDetector::detect", h_);
        detectedMarkers.clear();
        for (int i = 0; i < n; i++) detectedMarkers.push_back(Marker::from_abi(out[i]));
        frame_size_ = cv::Size(input.cols, input.rows);
        thres_valid_ = false, cand_valid_ = false;
    }
    // markerdetector.h:116-120
    void detect(const cv::Mat& input, std::vector<Marker>& detectedMarkers, const CameraParameters& camParams, float markerSizeMeters = -1,
                bool setYPerpendicular = false) {
        detect(input, detectedMarkers, camParams.CameraMatrix, camParams.Distorsion, markerSizeMeters, setYPerpendicular);
    }
    // A camera-native host frame: GRAY8 and the Y plane of NV12 are grey frames as they lie; every other format is converted to grey on the
    // device (arucohip_convert_batch), and the grey image then takes the path of detect(cv::Mat).
    void detect(const RawFrame& input, std::vector<Marker>& detectedMarkers, const CameraParameters& camParams = CameraParameters(),
                float markerSizeMeters = -1, bool setYPerpendicular = false) {
        arucohip_frame_format_t fmt;
        fmt.format = (int32_t)input.format, fmt.bits = input.bits, fmt.chroma_offset = input.chromaOffset;
        if (!input.data || !arucohip_frame_min_stride(&fmt, input.width, input.height, input.step))
            arucohip_throw_(ARUCOHIP_E_INVALID, "detect: RawFrame with an invalid format, size, step or chromaOffset", nullptr);
        cv::Mat grey;
        if (input.format == PixelFormat::GRAY8 || input.format == PixelFormat::NV12) {
            grey = cv::Mat(input.height, input.width, CV_8UC1, const_cast<void*>(input.data), input.step);
        } else {
            ensure_(input.width, input.height);
            convert_frame_(h_, input, grey, 1);
        }
        detect(grey, detectedMarkers, camParams.CameraMatrix, camParams.Distorsion, markerSizeMeters, setYPerpendicular);
    }

#if ARUCOHIP_HAVE_OPENCV
    // With the real OpenCV the reference takes cv::InputArray (markerdetector.h:102): anything that is not already a cv::Mat
    // (std::vector<uchar>, cv::Mat_, cv::UMat ...) comes through getMat(). This branch cannot be compiled in the build container
    // (no OpenCV there): DESIGN.md lists it as untested.
    template <class A, class = typename std::enable_if<!std::is_convertible<const A&, const cv::Mat&>::value>::type>
    void detect(const A& input, std::vector<Marker>& detectedMarkers, cv::Mat camMatrix = cv::Mat(), cv::Mat distCoeff = cv::Mat(),
                float markerSizeMeters = -1, bool setYPerpendicular = false) {
        detect(cv::_InputArray(input).getMat(), detectedMarkers, camMatrix, distCoeff, markerSizeMeters, setYPerpendicular);
    }
#endif

    // markerdetector.h:78
    typedef int (*MarkerdetectorFunc)(const cv::Mat& in, int& nRotations);
    // markerdetector.h:243-245. The library's two decoders select the device kernels; any other function is called on the
    // host with the canonical patch the device warped (contract: markerdetector.h:65-77), the pipeline continues on the device.
    void setMakerDetectorFunction(MarkerdetectorFunc markerdetector_func) {
        // a null function changes nothing: the detector keeps the decoder it had (the check comes before any member is touched)
        if (!markerdetector_func) arucohip_throw_(ARUCOHIP_E_INVALID, "setMakerDetectorFunction: null function", nullptr);
        user_fn_ = nullptr, hrm_ = false;
        if (markerdetector_func == &HighlyReliableMarkers::detect)
            hrm_ = true;
        else if (markerdetector_func != &FiducidalMarkers::detect)
            user_fn_ = markerdetector_func;
        p_.decoder_kind = user_fn_ ? ARUCOHIP_DECODER_USER : hrm_ ? ARUCOHIP_DECODER_HRM : ARUCOHIP_DECODER_FIDUCIAL_5X5;   // part of the parameter set from now on
        hrm_version_ = -1;
        if (h_) apply_decoder_();
    }
    void setThresholdMethod(ThresholdMethods m) { p_.thres_method = (int)m, push_(); }
    ThresholdMethods getThresholdMethod() const { return (ThresholdMethods)p_.thres_method; }
    void setThresholdParams(double param1, double param2) { p_.thres_param1 = param1, p_.thres_param2 = param2, push_(); }
    void setThresholdParamRange(size_t r1 = 0, size_t = 0) { p_.thres_param1_range = (int)r1, recreate_(); }
    void getThresholdParams(double& param1, double& param2) const { param1 = p_.thres_param1, param2 = p_.thres_param2; }
    void enableLockedCornersMethod(bool enable) {  // markerdetector.cpp:291-295
        p_.use_locked_corners = enable;
        if (enable) p_.corner_method = SUBPIX;
        push_();
    }
    // MarkerDetector::pyrDown(level) of ArUco 1.2 (this snapshot of the reference keeps the call as a no-op, PortingManual.md): threshold, contours
    // and quads run on the frame reduced `level` times (0..3), everything else on the frame itself; arucohip_set_pyr_down
    void pyrDown(unsigned int level) {
        if (level > 3) arucohip_throw_(ARUCOHIP_E_INVALID, "pyrDown: level outside 0..3", nullptr);
        if (h_) arucohip_throw_(arucohip_set_pyr_down(h_, (int)level), "pyrDown", h_);
        pyr_ = (int)level;
    }
    const cv::Mat& getThresholdedImage() {  // markerdetector.h:183; with pyrDown(level) the reduced image
        if (!thres_valid_ && h_ && frame_size_.width > 0) {
            int tw = frame_size_.width, th = frame_size_.height;
            for (int l = 0; l < arucohip_get_pyr_down(h_); l++) tw = (tw + 1) / 2, th = (th + 1) / 2;
            thres_ = cv::Mat(th, tw, CV_8UC1);
            arucohip_throw_(arucohip_get_thresholded(h_, 0, thres_.data), "getThresholdedImage", h_);
            thres_valid_ = true;
        }
        return thres_;
    }
    void setCornerRefinementMethod(CornerRefinementMethod m) { p_.corner_method = (int)m, push_(); }
    CornerRefinementMethod getCornerRefinementMethod() const { return (CornerRefinementMethod)p_.corner_method; }
    void setMinMaxSize(float min = 0.03f, float max = 0.5f) {  // CV_Assert ranges: markerdetector.cpp:1031-1038
        arucohip_params_t q = p_;
        q.min_size = min, q.max_size = max;
        check_(q);
        p_ = q, push_();
    }
    void getMinMaxSize(float& min, float& max) { min = p_.min_size, max = p_.max_size; }
    void setDesiredSpeed(int val) {  // markerdetector.cpp:265-285
        if (val < 0) val = 0;
        else if (val > 3) val = 2;
        speed_ = val;
        if (val == 0) p_.warp_size = 56, p_.corner_method = SUBPIX;
        else if (val == 1 || val == 2) p_.warp_size = 28, p_.corner_method = NONE;
        push_();
    }
    int getDesiredSpeed() const { return speed_; }
    void setWarpSize(int val) {  // CV_Assert(val >= 10): markerdetector.cpp:1047-1051
        arucohip_params_t q = p_;
        q.warp_size = val;
        check_(q);
        p_ = q, push_();
    }
    int getWarpSize() const { return p_.warp_size; }
    const std::vector<std::vector<cv::Point2f> >& getCandidates() {  // markerdetector.h:266
        if (!cand_valid_ && h_) {
            std::vector<float> q(512 * 8);
            int n = 0;
            arucohip_throw_(arucohip_get_candidates(h_, 0, q.data(), 512, &n), "getCandidates", h_);
            candidates_.assign(n, std::vector<cv::Point2f>(4));
            for (int i = 0; i < n; i++)
                for (int k = 0; k < 4; k++) candidates_[i][k] = cv::Point2f(q[i * 8 + 2 * k], q[i * 8 + 2 * k + 1]);
            cand_valid_ = true;
        }
        return candidates_;
    }
    // stage entry points (markerdetector.h:255-280)
    void thresHold(int method, const cv::Mat& grey, cv::Mat& thresImg, double param1 = -1, double param2 = -1) {
        if (grey.type() != CV_8UC1) arucohip_throw_(ARUCOHIP_E_INVALID, "thresHold: grey.type() == CV_8UC1", nullptr);  // :644
        ensure_(grey.cols, grey.rows);
        thresImg = cv::Mat(grey.rows, grey.cols, CV_8UC1);
        arucohip_throw_(arucohip_threshold(h_, method, grey.data, grey.cols, grey.rows, grey.step, param1, param2, thresImg.data), "thresHold", h_);
    }
    void detectRectangles(const cv::Mat& thresImg, std::vector<std::vector<cv::Point2f> >& candidates) {
        ensure_(thresImg.cols, thresImg.rows);
        std::vector<float> q(512 * 8);
        int n = 0;
        arucohip_throw_(arucohip_detect_rectangles(h_, thresImg.data, thresImg.cols, thresImg.rows, thresImg.step, q.data(), 512, &n), "detectRectangles", h_);
        candidates.assign(n, std::vector<cv::Point2f>(4));
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 4; k++) candidates[i][k] = cv::Point2f(q[i * 8 + 2 * k], q[i * 8 + 2 * k + 1]);
    }
    void warp(const cv::Mat& in, cv::Mat& out, cv::Size size, std::vector<cv::Point2f> points) {
        if (points.size() != 4) arucohip_throw_(ARUCOHIP_E_INVALID, "warp: points.size() == 4", nullptr);  // :685
        ensure_(in.cols, in.rows);
        float q[8];
        for (int k = 0; k < 4; k++) q[2 * k] = points[k].x, q[2 * k + 1] = points[k].y;
        out = cv::Mat(size.height, size.width, CV_8UC1);
        arucohip_throw_(arucohip_warp(h_, in.data, in.cols, in.rows, in.step, q, size.width, out.data), "warp", h_);
    }
    // markerdetector.h:280 / markerdetector.cpp:931-997: the LINES corner refinement of one candidate, on the device
    // (arucohip_refine_candidate_lines): the four corners become the intersections of the least-squares lines through the contour's sides;
    // with both matrices non-empty the contour is undistorted first and the corners are distorted again.
    void refineCandidateLines(MarkerCandidate& candidate, const cv::Mat& camMatrix, const cv::Mat& distCoeff) {
        if (candidate.size() != 4 || candidate.contour.empty())
            arucohip_throw_(ARUCOHIP_E_INVALID, "refineCandidateLines: a candidate has 4 corners and a contour", nullptr);
        ensure_(std::max(cap_w_, 64), std::max(cap_h_, 64));
        float K[9], d[8], c[8];
        const bool hasK = mat_to_K_(camMatrix, K);
        const int nd = mat_to_dist_(distCoeff, d);
        const bool undist = hasK && nd > 0;   // :958 / :990: both matrices or neither
        std::vector<int32_t> xy(2 * candidate.contour.size());
        for (size_t i = 0; i < candidate.contour.size(); i++) xy[2 * i] = candidate.contour[i].x, xy[2 * i + 1] = candidate.contour[i].y;
        for (int k = 0; k < 4; k++) c[2 * k] = candidate[k].x, c[2 * k + 1] = candidate[k].y;
        arucohip_throw_(arucohip_refine_candidate_lines(h_, xy.data(), (int)candidate.contour.size(), c, undist ? K : nullptr, undist ? d : nullptr, undist ? nd : 0),
                        "refineCandidateLines", h_);
        for (int k = 0; k < 4; k++) candidate[k] = cv::Point2f(c[2 * k], c[2 * k + 1]);
    }
    // Marker::calculateExtrinsics for a whole vector at once (batched device solvePnP)
    void calculateExtrinsics(std::vector<Marker>& markers, float markerSize, cv::Mat camMatrix, cv::Mat distCoeff = cv::Mat(), bool setYPerpendicular = true) {
        if (markers.empty()) return;
        ensure_(std::max(cap_w_, 64), std::max(cap_h_, 64));
        float K[9], d[8];
        if (!mat_to_K_(camMatrix, K)) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraMatrix is empty", nullptr);
        int nd = mat_to_dist_(distCoeff, d);
        std::vector<arucohip_marker_t> m(markers.size());
        for (size_t i = 0; i < markers.size(); i++) markers[i].to_abi(&m[i]);
        arucohip_throw_(arucohip_calculate_extrinsics(h_, m.data(), (int)m.size(), K, nd ? d : nullptr, nd, markerSize, setYPerpendicular), "calculateExtrinsics", h_);
        for (size_t i = 0; i < markers.size(); i++) markers[i] = Marker::from_abi(m[i]);
    }
    arucohip_handle* handle(int w = 640, int h = 480) {
        ensure_(std::max(w, cap_w_), std::max(h, cap_h_));
        return h_;
    }

private:
    void check_(const arucohip_params_t& q) {
        arucohip_handle* tmp = h_;
        if (!tmp) ensure_(640, 480), tmp = h_;
        arucohip_params_t saved;
        arucohip_get_params(tmp, &saved);
        int rc = arucohip_set_params(tmp, &q);
        if (rc != ARUCOHIP_OK) {
            arucohip_set_params(tmp, &saved);
            arucohip_throw_(rc, "MarkerDetector parameter", tmp);
        }
    }
    void push_() {
        if (h_) arucohip_throw_(arucohip_set_params(h_, &p_), "MarkerDetector parameter", h_);
    }
    void recreate_() {
        if (!h_) return;
        int w = cap_w_, hh = cap_h_;
        arucohip_destroy(h_);
        h_ = nullptr, cap_w_ = cap_h_ = 0;
        ensure_(w, hh);
    }
    void ensure_(int w, int hh) {
        if (h_ && w <= cap_w_ && hh <= cap_h_) return;   // device arrays are sized per dimension
        w = std::max(std::max(w, cap_w_), 32), hh = std::max(std::max(hh, cap_h_), 32);   // a handle is at least 32 x 32; frames may be smaller
        arucohip_destroy(h_);
        h_ = nullptr;
        arucohip_limits_t lim;
        arucohip_default_limits(&lim, w, hh, 1);
        lim.max_thres_planes = std::max(1, 2 * p_.thres_param1_range + 1);
        // the reference has no list limits: after a device list overflow detect() retries with larger lists (grow_)
        for (int g = 0; g < grow_; g++) {
            lim.triggers_per_frame = std::min(lim.triggers_per_frame * 2, 1 << 22);
            lim.contours_per_frame = std::min(lim.contours_per_frame * 2, 1 << 18);
            lim.points_per_frame = std::min(lim.points_per_frame * 2, 1 << 24);
            lim.long_walks_per_plane = std::min(lim.long_walks_per_plane * 2, 1 << 16);
        }
        lim.candidates_per_frame = 512, lim.markers_per_frame = 256;
        arucohip_throw_(arucohip_create_ex(&p_, device_, &lim, &h_), "arucohip_create", nullptr);
        cap_w_ = w, cap_h_ = hh;
        if (pyr_) arucohip_throw_(arucohip_set_pyr_down(h_, pyr_), "pyrDown", h_);
        hrm_version_ = -1;
        if (hrm_ || user_fn_) apply_decoder_();
    }
    // HighlyReliableMarkers' static dictionary -> the handle (arucohip_set_dictionary), or back to the fiducial decoder
    void apply_decoder_() {
        if (hrm_) {
            const HighlyReliableMarkers::State_& s = HighlyReliableMarkers::state_();
            if (s.D.empty()) arucohip_throw_(ARUCOHIP_E_INVALID, "HighlyReliableMarkers: no dictionary loaded", nullptr);
            std::vector<uint64_t> codes(s.D.size(), 0);
            for (size_t i = 0; i < s.D.size(); i++)
                for (unsigned int b = 0; b < s.D[i].size(); b++)
                    if (s.D[i].get(b)) codes[i] |= 1ull << b;
            arucohip_throw_(arucohip_set_dictionary(h_, (int)s.D[0].n(), (int)codes.size(), codes.data(), s.D.tau0, s.rate), "loadDictionary", h_);
            hrm_version_ = s.version;
        }
        arucohip_throw_(arucohip_set_decoder_callback(h_, user_fn_ ? &user_trampoline_ : nullptr, reinterpret_cast<void*>(user_fn_)), "setMakerDetectorFunction", h_);
        push_();
    }
    // the C ABI's callback -> the reference's function type: a cv::Mat header over the patch, nRotations by reference
    static int user_trampoline_(void* user, uint8_t* patch, int size, int* n_rotations) {
        MarkerdetectorFunc fn = reinterpret_cast<MarkerdetectorFunc>(user);
        cv::Mat in(size, size, CV_8UC1, patch);
        int nrot = *n_rotations;
        const int id = fn(in, nrot);
        *n_rotations = nrot;
        return id;
    }
    MarkerdetectorFunc user_fn_ = nullptr;
    std::vector<arucohip_marker_t> out_;
    arucohip_handle* h_;
    int device_, cap_w_, cap_h_;
    int grow_ = 0;   // doublings of the device list limits after overflows
    int pyr_ = 0;    // pyrDown level, set again on every handle ensure_ creates
    arucohip_params_t p_;
    int speed_ = 0;
    bool hrm_ = false;
    int hrm_version_ = -1;
    cv::Size frame_size_;
    cv::Mat thres_;
    bool thres_valid_ = false, cand_valid_ = false;
    std::vector<std::vector<cv::Point2f> > candidates_;
};

// Frames sharded over the GPUs of the node behind one call (arucohip_mgpu_*). No reference counterpart: the
// reference's frame loop (utils/aruco_test.cpp:140-160) calls one MarkerDetector per frame; with this helper the loop hands
// over up to devices x framesPerDevice frames at once, frame f is detected on device f mod G and the markers come back in
// frame order.
class MultiGpuDetector {
public:
    MultiGpuDetector(const std::vector<int>& devices, int maxWidth, int maxHeight, int framesPerDevice, bool gatherOverXgmi = false) : m_(nullptr) {
        arucohip_throw_(arucohip_mgpu_create(nullptr, devices.empty() ? nullptr : devices.data(), devices.empty() ? arucohip_mgpu_device_count() : (int)devices.size(),
                                             maxWidth, maxHeight, framesPerDevice, 128, gatherOverXgmi ? ARUCOHIP_MGPU_GATHER_PEER : ARUCOHIP_MGPU_GATHER_HOST, &m_),
                        "arucohip_mgpu_create", nullptr);
    }
    ~MultiGpuDetector() { arucohip_mgpu_destroy(m_); }
    MultiGpuDetector(const MultiGpuDetector&) = delete;
    MultiGpuDetector& operator=(const MultiGpuDetector&) = delete;
    int devices() const { return arucohip_mgpu_size(m_); }
    // equally sized 8-bit gray frames; same camera arguments as MarkerDetector::detect
    void detect(const std::vector<cv::Mat>& frames, std::vector<std::vector<Marker> >& detectedMarkers, cv::Mat camMatrix = cv::Mat(),
                cv::Mat distCoeff = cv::Mat(), float markerSizeMeters = -1, bool setYPerpendicular = false) {
        detectedMarkers.assign(frames.size(), std::vector<Marker>());
        if (frames.empty()) return;
        const int w = frames[0].cols, h = frames[0].rows;
        std::vector<unsigned char> packed((size_t)frames.size() * w * h);
        for (size_t f = 0; f < frames.size(); f++) {
            if (frames[f].type() != CV_8UC1 || frames[f].cols != w || frames[f].rows != h)
                arucohip_throw_(ARUCOHIP_E_INVALID, "MultiGpuDetector::detect: equally sized CV_8UC1 frames", nullptr);
            for (int r = 0; r < h; r++) std::memcpy(packed.data() + (f * h + r) * (size_t)w, frames[f].data + (size_t)r * frames[f].step, (size_t)w);
        }
        float K[9], d[8];
        const bool hasK = mat_to_K_(camMatrix, K);
        const int nd = mat_to_dist_(distCoeff, d);
        std::vector<arucohip_marker_t> out(frames.size() * 128);
        std::vector<int32_t> n(frames.size(), 0);
        const int rc = arucohip_mgpu_detect_batch(m_, packed.data(), (int)frames.size(), w, h, (size_t)w, (size_t)w * h, hasK ? K : nullptr, nd ? d : nullptr, nd,
                                                  markerSizeMeters, setYPerpendicular ? 1 : 0, out.data(), 128, n.data());
        if (rc != ARUCOHIP_OK) throw cv::Exception(rc == ARUCOHIP_E_INVALID ? -215 : -2, std::string("MultiGpuDetector::detect: ") + arucohip_mgpu_last_error_string(m_)
#if ARUCOHIP_HAVE_OPENCV
                                                   , "arucohip", __FILE__, __LINE__
#endif
        );
        for (size_t f = 0; f < frames.size(); f++)
            for (int i = 0; i < n[f]; i++) detectedMarkers[f].push_back(Marker::from_abi(out[f * 128 + i]));
    }

private:
    arucohip_mgpu* m_;
};

class BoardDetector {
public:
    explicit BoardDetector(bool setYPerpendicular = false) : _setYPerpendicular(setYPerpendicular), _areParamsSet(false), _markerSize(-1), repj_err_thres(-1) {}
    void setParams(const BoardConfiguration& bc, const CameraParameters& cp, float markerSizeMeters = -1) {
        _camParams = cp, _markerSize = markerSizeMeters, _bconf = bc, _areParamsSet = true;
    }
    void setParams(const BoardConfiguration& bc) { _bconf = bc, _areParamsSet = true; }
    // boarddetector.cpp:66-77
    float detect(const cv::Mat& im) {
        _mdetector.detect(im, _vmarkers);
        if (_camParams.isValid())
            return detect(_vmarkers, _bconf, _boardDetected, _camParams.CameraMatrix, _camParams.Distorsion, _markerSize);
        return detect(_vmarkers, _bconf, _boardDetected);
    }
    float detect(const std::vector<Marker>& detectedMarkers, const BoardConfiguration& BConf, Board& Bdetected, const CameraParameters& cp,
                 float markerSizeMeters = -1) {
        return detect(detectedMarkers, BConf, Bdetected, cp.CameraMatrix, cp.Distorsion, markerSizeMeters);
    }
    // boarddetector.cpp:90-205
    float detect(const std::vector<Marker>& detectedMarkers, const BoardConfiguration& BConf, Board& Bdetected, cv::Mat camMatrix = cv::Mat(),
                 cv::Mat distCoeff = cv::Mat(), float markerSizeMeters = -1) {
        float K[9], d[8];
        bool hasK = mat_to_K_(camMatrix, K);
        int nd = mat_to_dist_(distCoeff, d);
        std::vector<arucohip_marker_t> in(std::max<size_t>(detectedMarkers.size(), 1)), out(std::max<size_t>(detectedMarkers.size(), 1));
        for (size_t i = 0; i < detectedMarkers.size(); i++) detectedMarkers[i].to_abi(&in[i]);
        std::vector<int32_t> ids(BConf.ids.begin(), BConf.ids.end());
        std::vector<float> obj;
        for (size_t i = 0; i < BConf.objPoints.size(); i++)
            for (int p = 0; p < 4 && p < (int)BConf.objPoints[i].size(); p++)
                obj.push_back(BConf.objPoints[i][p].x), obj.push_back(BConf.objPoints[i][p].y), obj.push_back(BConf.objPoints[i][p].z);
        arucohip_board_t b;
        float prob = 0;
        arucohip_handle* h = _mdetector.handle();
        int rc = arucohip_board_detect(h, in.data(), (int)detectedMarkers.size(), ids.data(), obj.data(), (int)ids.size(), BConf.mInfoType,
                                       hasK ? K : nullptr, nd ? d : nullptr, nd, markerSizeMeters, repj_err_thres, _setYPerpendicular ? 1 : 0,
                                       out.data(), &b, &prob);
        arucohip_throw_(rc, "BoardDetector::detect", h);
        Bdetected.clear();
        for (int i = 0; i < b.n_markers; i++) Bdetected.push_back(Marker::from_abi(out[i]));
        Bdetected.conf = BConf;
        if (b.has_pose) {
            Bdetected.Rvec = cv::Mat_<double>(3, 1), Bdetected.Tvec = cv::Mat_<double>(3, 1);
            for (int k = 0; k < 3; k++) Bdetected.Rvec(k) = b.rvec[k], Bdetected.Tvec(k) = b.tvec[k];
        }
        return prob;
    }
    static Board detect(const cv::Mat& Image, const BoardConfiguration& bc, const CameraParameters& cp, float markerSizeMeters = -1) {
        BoardDetector BD;
        BD.setParams(bc, cp, markerSizeMeters);
        BD.detect(Image);
        return BD.getDetectedBoard();
    }
    // No counterpart in the reference (OpenCV's aruco module: refineDetectedMarkers). The board's markers that the decoder rejected in the
    // last detect(im) are taken back from that frame's rejected candidates on the device (arucohip_board_recover_batch): a candidate within
    // maxCornerDist pixels of where the board's pose puts the marker, showing it in all but maxCellErrors cells. Replaces the detector's
    // marker vector and board; returns the number of markers recovered.
    int recoverMarkers(const BoardConfiguration& BConf, const CameraParameters& cp, float markerSizeMeters = -1, float maxCornerDist = 10,
                       int maxCellErrors = 3) {
        float K[9], d[8];
        bool hasK = mat_to_K_(cp.CameraMatrix, K);
        int nd = mat_to_dist_(cp.Distorsion, d);
        std::vector<int32_t> ids(BConf.ids.begin(), BConf.ids.end());
        std::vector<float> obj;
        for (size_t i = 0; i < BConf.objPoints.size(); i++)
            for (int p = 0; p < 4 && p < (int)BConf.objPoints[i].size(); p++)
                obj.push_back(BConf.objPoints[i][p].x), obj.push_back(BConf.objPoints[i][p].y), obj.push_back(BConf.objPoints[i][p].z);
        arucohip_recover_t o;
        arucohip_default_recover(&o);
        o.max_corner_dist = maxCornerDist, o.max_cell_errors = maxCellErrors, o.pose_markers = markerSizeMeters > 0 ? 1 : 0;
        const int cap = 512;
        std::vector<arucohip_marker_t> out(cap);
        int32_t n = 0, recovered = 0;
        arucohip_handle* h = _mdetector.handle();
        int rc = arucohip_board_recover_batch(h, 1, ids.data(), obj.data(), (int)ids.size(), BConf.mInfoType, hasK ? K : nullptr, nd ? d : nullptr, nd,
                                              markerSizeMeters, repj_err_thres, _setYPerpendicular ? 1 : 0, &o, out.data(), cap, &n, 0, &recovered,
                                              nullptr, nullptr);
        arucohip_throw_(rc, "BoardDetector::recoverMarkers", h);
        _vmarkers.clear();
        for (int i = 0; i < n && i < cap; i++) _vmarkers.push_back(Marker::from_abi(out[i]));
        detect(_vmarkers, BConf, _boardDetected, cp.CameraMatrix, cp.Distorsion, markerSizeMeters);
        return recovered;
    }
    // No counterpart in this snapshot of the reference (its later versions ship a marker mapper). The 3-D layout of a rigid marker set
    // (a cube, markers around a room) from frames that show several of its markers each, solved on the device (arucohip_board_map):
    // a BoardConfiguration in metres in the frame of the first id, for detect() above. frames[f]: the markers detected in frame f. mapped
    // (may be NULL) gets one flag per id; an id that no frame connects to the first one has mapped = false and zero corners. rms (may be
    // NULL): the reprojection error in pixels.
    BoardConfiguration mapBoard(const std::vector<std::vector<Marker> >& frames, const std::vector<int>& ids, const CameraParameters& cp,
                                float markerSizeMeters, std::vector<bool>* mapped = nullptr, double* rms = nullptr) {
        std::vector<int32_t> of, oi;
        std::vector<float> oc;
        for (size_t f = 0; f < frames.size(); f++)
            for (size_t i = 0; i < frames[f].size(); i++) {
                if (frames[f][i].size() != 4) continue;
                of.push_back((int32_t)f), oi.push_back(frames[f][i].id);
                for (int k = 0; k < 4; k++) oc.push_back(frames[f][i][k].x), oc.push_back(frames[f][i][k].y);
            }
        return map_(false, (int)frames.size(), &of, &oi, &oc, ids, cp, markerSizeMeters, 2, mapped, rms);
    }
    // The same on the device-resident markers of the first nframes frames of the last batch the detector's handle ran
    // (getMarkerDetector().handle(): arucohip_detect_batch, or the one frame of detect(im)).
    BoardConfiguration mapBoardLastBatch(int nframes, const std::vector<int>& ids, const CameraParameters& cp, float markerSizeMeters, int minMarkers = 2,
                                         std::vector<bool>* mapped = nullptr, double* rms = nullptr) {
        return map_(true, nframes, nullptr, nullptr, nullptr, ids, cp, markerSizeMeters, minMarkers, mapped, rms);
    }
    Board& getDetectedBoard() { return _boardDetected; }
    MarkerDetector& getMarkerDetector() { return _mdetector; }
    std::vector<Marker>& getDetectedMarkers() { return _vmarkers; }
    void setYPerpendicular(bool enable) { _setYPerpendicular = enable; }
    bool isYPerpendicular() { return _setYPerpendicular; }   // boarddetector.h:128
    void set_repj_err_thres(float Repj_err_thres) { repj_err_thres = Repj_err_thres; }
    float get_repj_err_thres() const { return repj_err_thres; }

private:
    BoardConfiguration map_(bool batch, int nframes, const std::vector<int32_t>* of, const std::vector<int32_t>* oi, const std::vector<float>* oc,
                            const std::vector<int>& ids, const CameraParameters& cp, float markerSizeMeters, int minMarkers, std::vector<bool>* mapped,
                            double* rms) {
        float K[9], d[8];
        const bool hasK = mat_to_K_(cp.CameraMatrix, K);
        const int nd = mat_to_dist_(cp.Distorsion, d);
        const size_t nb = ids.size();
        std::vector<int32_t> bid(ids.begin(), ids.end()), flag(std::max<size_t>(nb, 1));
        std::vector<float> obj(std::max<size_t>(nb, 1) * 12);
        std::vector<double> rv(std::max<size_t>(nb, 1) * 3), tv(std::max<size_t>(nb, 1) * 3);
        arucohip_handle* h = _mdetector.handle();
        const int rc = batch ? arucohip_board_map_batch(h, nframes, bid.data(), (int)nb, hasK ? K : nullptr, nd ? d : nullptr, nd, markerSizeMeters,
                                                        minMarkers, obj.data(), rv.data(), tv.data(), flag.data(), nullptr, nullptr, nullptr, nullptr,
                                                        rms, nullptr)
                             : arucohip_board_map(h, of->data(), oi->data(), oc->data(), (int)of->size(), 0, nframes, bid.data(), (int)nb,
                                                  hasK ? K : nullptr, nd ? d : nullptr, nd, markerSizeMeters, obj.data(), rv.data(), tv.data(),
                                                  flag.data(), nullptr, nullptr, nullptr, nullptr, rms, nullptr);
        arucohip_throw_(rc, "BoardDetector::mapBoard", h);
        BoardConfiguration bc;
        bc.mInfoType = BoardConfiguration::METERS;
        bc.ids = ids;
        if (mapped) mapped->assign(nb, false);
        for (size_t i = 0; i < nb; i++) {
            std::vector<cv::Point3f> c(4);
            for (int k = 0; k < 4; k++) c[k] = cv::Point3f(obj[12 * i + 3 * k], obj[12 * i + 3 * k + 1], obj[12 * i + 3 * k + 2]);
            bc.objPoints.push_back(c);
            if (mapped) (*mapped)[i] = flag[i] != 0;
        }
        return bc;
    }
    bool _setYPerpendicular, _areParamsSet;
    BoardConfiguration _bconf;
    Board _boardDetected;
    float _markerSize;
    CameraParameters _camParams;
    MarkerDetector _mdetector;
    std::vector<Marker> _vmarkers;
    float repj_err_thres;
};

// Several cameras on one frame, exposed together (no counterpart in this snapshot of the reference; cv::stereoCalibrate answers the
// first question for two cameras). cameras[c] holds camera c's fixed intrinsics; Rvec[c] / Tvec[c] (3x1 double) its transform rig ->
// camera and calibrated[c] whether calibrate() reached it; camera 0 is the rig frame. View v = instant * cameras.size() + camera: an
// interleaved stream is a batch as it stands. Solved on the device (arucohip_rig_calibrate* / arucohip_rig_pose*, include/arucohip.h).
class CameraRig {
public:
    std::vector<CameraParameters> cameras;
    std::vector<cv::Mat_<double> > Rvec, Tvec;
    std::vector<bool> calibrated;
    std::vector<double> cameraRms;   // of the last calibrate, pixels
    double rms;
    int minMarkers;                  // member markers a view must hold to count

    CameraRig() : rms(0), minMarkers(1) {}
    explicit CameraRig(const std::vector<CameraParameters>& cams) : cameras(cams), rms(0), minMarkers(1) {}

    // The cameras' transforms from the markers of every view (views[v]: the markers detected in view v), and the board's pose in the rig
    // frame at every instant (a Board without Rvec / Tvec for an instant that was not used).
    std::vector<Board> calibrate(MarkerDetector& detector, const std::vector<std::vector<Marker> >& views, const BoardConfiguration& bc, float markerSizeMeters = -1) {
        return run_(detector.handle(), true, &views, 0, bc, markerSizeMeters);
    }
    // The same on the device-resident markers of the first nframes frames of a handle's last batch: frame f is view f, ncams must equal
    // cameras.size(). A MarkerDetector's own handle holds one frame, which is no whole instant; a stream of several cameras goes through
    // arucohip_detect_batch on a handle of the caller's, created with room for the batch, and that handle is passed here.
    std::vector<Board> calibrate(arucohip_handle* h, const BoardConfiguration& bc, float markerSizeMeters, int ncams, int nframes) {
        if (ncams != (int)cameras.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraRig::calibrate: ncams differs from the cameras given", nullptr);
        return run_(h, true, nullptr, nframes, bc, markerSizeMeters);
    }
    std::vector<Board> calibrate(MarkerDetector& detector, const BoardConfiguration& bc, float markerSizeMeters, int ncams, int nframes) {
        return calibrate(detector.handle(), bc, markerSizeMeters, ncams, nframes);
    }
    // The board's pose in the rig frame at every instant, from every calibrated camera that sees part of it.
    std::vector<Board> detect(MarkerDetector& detector, const std::vector<std::vector<Marker> >& views, const BoardConfiguration& bc, float markerSizeMeters = -1) {
        return run_(detector.handle(), false, &views, 0, bc, markerSizeMeters);
    }
    std::vector<Board> detect(arucohip_handle* h, const BoardConfiguration& bc, float markerSizeMeters, int nframes) {
        return run_(h, false, nullptr, nframes, bc, markerSizeMeters);
    }
    std::vector<Board> detect(MarkerDetector& detector, const BoardConfiguration& bc, float markerSizeMeters, int nframes) {
        return detect(detector.handle(), bc, markerSizeMeters, nframes);
    }

private:
    std::vector<Board> run_(arucohip_handle* h, bool calib, const std::vector<std::vector<Marker> >* views, int nframes, const BoardConfiguration& bc,
                            float markerSizeMeters) {
        const int nc = (int)cameras.size();
        std::vector<arucohip_rig_camera_t> cams(std::max(nc, 1));
        for (int c = 0; c < nc; c++) {
            arucohip_rig_camera_t& rc = cams[c];
            std::memset(&rc, 0, sizeof(rc));
            float d[8];
            if (!mat_to_K_(cameras[c].CameraMatrix, rc.K)) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraRig: a camera matrix is empty", nullptr);
            rc.ndist = mat_to_dist_(cameras[c].Distorsion, d);
            for (int k = 0; k < 5 && k < rc.ndist; k++) rc.dist[k] = d[k];
            if (!calib && c < (int)calibrated.size() && calibrated[c] && c < (int)Rvec.size() && c < (int)Tvec.size() && !Rvec[c].empty() && !Tvec[c].empty()) {
                rc.calibrated = 1;
                for (int k = 0; k < 3; k++) rc.rvec[k] = Rvec[c](k), rc.tvec[k] = Tvec[c](k);
            }
        }
        std::vector<int32_t> ov, oi, ids(bc.ids.begin(), bc.ids.end());
        std::vector<float> oc, obj;
        for (size_t i = 0; i < bc.objPoints.size(); i++)
            for (int p = 0; p < 4 && p < (int)bc.objPoints[i].size(); p++)
                obj.push_back(bc.objPoints[i][p].x), obj.push_back(bc.objPoints[i][p].y), obj.push_back(bc.objPoints[i][p].z);
        if (views) {
            nframes = (int)views->size();
            for (size_t v = 0; v < views->size(); v++)
                for (size_t i = 0; i < (*views)[v].size(); i++) {
                    const Marker& m = (*views)[v][i];
                    if (m.size() != 4) continue;
                    ov.push_back((int32_t)v), oi.push_back(m.id);
                    for (int k = 0; k < 4; k++) oc.push_back(m[k].x), oc.push_back(m[k].y);
                }
            if (nc > 0 && nframes % nc != 0) arucohip_throw_(ARUCOHIP_E_INVALID, "CameraRig: the views are not whole instants", nullptr);
        }
        const int ninstants = nc > 0 ? nframes / nc : 0;
        std::vector<arucohip_board_t> out(std::max(ninstants, 1));
        std::vector<int32_t> used(std::max(ninstants, 1));
        std::vector<double> brv(std::max(ninstants, 1) * 3), btv(std::max(ninstants, 1) * 3), crms(std::max(nc, 1));
        int rc;
        if (calib)
            rc = views ? arucohip_rig_calibrate(h, ov.data(), oi.data(), oc.data(), (int)ov.size(), 0, ninstants, cams.data(), nc, ids.data(), obj.data(),
                                                (int)ids.size(), bc.mInfoType, markerSizeMeters, minMarkers, used.data(), brv.data(), btv.data(), crms.data(),
                                                &rms, nullptr)
                       : arucohip_rig_calibrate_batch(h, nframes, cams.data(), nc, ids.data(), obj.data(), (int)ids.size(), bc.mInfoType, markerSizeMeters,
                                                      minMarkers, used.data(), brv.data(), btv.data(), crms.data(), &rms, nullptr);
        else
            rc = views ? arucohip_rig_pose(h, ov.data(), oi.data(), oc.data(), (int)ov.size(), 0, ninstants, cams.data(), nc, ids.data(), obj.data(),
                                           (int)ids.size(), bc.mInfoType, markerSizeMeters, minMarkers, out.data(), nullptr)
                       : arucohip_rig_pose_batch(h, nframes, cams.data(), nc, ids.data(), obj.data(), (int)ids.size(), bc.mInfoType, markerSizeMeters,
                                                 minMarkers, out.data(), nullptr);
        arucohip_throw_(rc, calib ? "CameraRig::calibrate" : "CameraRig::detect", h);
        if (calib) {
            Rvec.assign(nc, cv::Mat_<double>()), Tvec.assign(nc, cv::Mat_<double>()), calibrated.assign(nc, false);
            cameraRms.assign(crms.begin(), crms.begin() + nc);
            for (int c = 0; c < nc; c++) {
                calibrated[c] = cams[c].calibrated != 0;
                Rvec[c] = cv::Mat_<double>(3, 1), Tvec[c] = cv::Mat_<double>(3, 1);
                for (int k = 0; k < 3; k++) Rvec[c](k) = cams[c].rvec[k], Tvec[c](k) = cams[c].tvec[k];
            }
        }
        std::vector<Board> boards(ninstants);
        for (int t = 0; t < ninstants; t++) {
            boards[t].conf = bc;
            if (!(calib ? used[t] != 0 : out[t].has_pose != 0)) continue;
            boards[t].Rvec = cv::Mat_<double>(3, 1), boards[t].Tvec = cv::Mat_<double>(3, 1);
            for (int k = 0; k < 3; k++)
                boards[t].Rvec(k) = calib ? brv[3 * t + k] : out[t].rvec[k], boards[t].Tvec(k) = calib ? btv[3 * t + k] : out[t].tvec[k];
        }
        return boards;
    }
};

// A camera with a fisheye lens (cv::fisheye's equidistant model; no counterpart in the reference): K (3x3), D (k1..k4) and the image
// size. The detector's corners, or the frames, are mapped once to an ideal pinhole camera (idealCamera(): Knew, no distortion), with
// which every other class of this header then works unchanged. Knew is K unless newCameraMatrix holds a 3x3 matrix; maxAngle <= 0 is
// 1.4 rad (arucohip_fisheye_*, include/arucohip.h).
class FisheyeCamera {
public:
    cv::Mat_<double> K, D;
    cv::Size size;
    cv::Mat_<double> newCameraMatrix;
    float maxAngle;
    double rms;   // of the last calibrate, pixels

    FisheyeCamera() : maxAngle(0), rms(0) {}
    FisheyeCamera(const double k[9], const double d[4], cv::Size sz) : K(3, 3), D(1, 4), size(sz), maxAngle(0), rms(0) {
        for (int i = 0; i < 9; i++) K(i / 3, i % 3) = k[i];
        for (int i = 0; i < 4; i++) D(0, i) = d[i];
    }
    // the pinhole camera the undistorted markers and frames belong to
    CameraParameters idealCamera() const {
        float kn[9];
        knew_(kn);
        const float none[4] = {0.f, 0.f, 0.f, 0.f};
        return CameraParameters(kn, none, 4, size);
    }
    // The markers of the detector's last frame where they lie on the device, mapped in place to the ideal camera and returned (without
    // poses: BoardDetector::detect or MarkerDetector::calculateExtrinsics with idealCamera() give them). A marker with a corner beyond
    // maxAngle is left out. The next detect() starts afresh.
    std::vector<Marker> undistortMarkers(MarkerDetector& detector) {
        std::vector<std::vector<Marker> > out = undistortMarkers(detector.handle(), 1);
        return out[0];
    }
    // The same on the first nframes frames of the last batch of a handle of the caller's (arucohip_detect_batch): one list per frame.
    std::vector<std::vector<Marker> > undistortMarkers(arucohip_handle* h, int nframes, int cap = 128) {
        const arucohip_fisheye_t m = model_();
        float kn[9];
        knew_(kn);
        std::vector<arucohip_marker_t> buf((size_t)std::max(nframes, 1) * cap);
        std::vector<int32_t> n(std::max(nframes, 1));
        arucohip_throw_(arucohip_fisheye_undistort_markers_batch(h, nframes, &m, 1, kn, maxAngle, buf.data(), cap, n.data(), 0, nullptr),
                        "FisheyeCamera::undistortMarkers", h);
        std::vector<std::vector<Marker> > out(nframes);
        for (int f = 0; f < nframes; f++)
            for (int i = 0; i < n[f] && i < cap; i++) out[f].push_back(Marker::from_abi(buf[(size_t)f * cap + i]));
        return out;
    }
    // A frame (CV_8UC1 or CV_8UC3) as the ideal camera sees it, for the paths that read pixels around the markers (CharucoBoard, marker
    // recovery, drawing): detect on the result with idealCamera().
    void undistortImage(const cv::Mat& src, cv::Mat& dst) const {
        if (src.type() != CV_8UC1 && src.type() != CV_8UC3) arucohip_throw_(ARUCOHIP_E_INVALID, "FisheyeCamera::undistortImage: CV_8UC1 or CV_8UC3 frames", nullptr);
        const arucohip_fisheye_t m = model_();
        float kn[9];
        knew_(kn);
        const int cn = src.type() == CV_8UC3 ? 3 : 1;
        cv::Mat out(src.rows, src.cols, src.type());
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure(src.cols, src.rows);
        arucohip_throw_(arucohip_fisheye_undistort(h, src.data, 1, src.cols, src.rows, src.step, (size_t)src.rows * src.step, cn, 0, &m, kn, maxAngle, out.data, 0),
                        "FisheyeCamera::undistortImage", h);
        dst = out;
    }
    // K and D from planar views (one list of object and image points per view), as cv::fisheye::calibrate is called: flags are
    // ARUCOHIP_FISHEYE_*; with USE_INTRINSIC_GUESS the current K and D are the start. Returns the RMS reprojection error; rvecs / tvecs
    // (3x1 double per view) may be NULL.
    double calibrate(const std::vector<std::vector<cv::Point3f> >& objPointsV, const std::vector<std::vector<cv::Point2f> >& imgPointsV, cv::Size imageSize,
                     int flags = 0, std::vector<cv::Mat>* rvecs = nullptr, std::vector<cv::Mat>* tvecs = nullptr) {
        if (objPointsV.size() != imgPointsV.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "FisheyeCamera::calibrate: object and image point lists differ", nullptr);
        const int nv = (int)objPointsV.size();
        std::vector<float> obj, img;
        std::vector<int32_t> np;
        for (int v = 0; v < nv; v++) {
            if (objPointsV[v].size() != imgPointsV[v].size()) arucohip_throw_(ARUCOHIP_E_INVALID, "FisheyeCamera::calibrate: a view's point counts differ", nullptr);
            np.push_back((int32_t)objPointsV[v].size());
            for (const cv::Point3f& p : objPointsV[v]) obj.push_back(p.x), obj.push_back(p.y), obj.push_back(p.z);
            for (const cv::Point2f& p : imgPointsV[v]) img.push_back(p.x), img.push_back(p.y);
        }
        arucohip_fisheye_t m;
        std::memset(&m, 0, sizeof(m));
        if (!K.empty() && !D.empty()) m = model_();
        std::vector<double> rv((size_t)std::max(nv, 1) * 3), tv((size_t)std::max(nv, 1) * 3);
        {
            SharedHandle_& sh = SharedHandle_::get();
            std::lock_guard<std::mutex> lock(sh.mu);
            arucohip_handle* h = sh.ensure();
            arucohip_throw_(arucohip_fisheye_calibrate(h, obj.data(), img.data(), np.data(), nv, 0, imageSize.width, imageSize.height, flags, &m, rv.data(),
                                                       tv.data(), nullptr, &rms),
                            "FisheyeCamera::calibrate", h);
        }
        K = cv::Mat_<double>(3, 3), D = cv::Mat_<double>(1, 4), size = imageSize;
        for (int i = 0; i < 9; i++) K(i / 3, i % 3) = m.K[i];
        for (int i = 0; i < 4; i++) D(0, i) = m.D[i];
        for (int v = 0; v < nv && rvecs && tvecs; v++) {
            if (v == 0) rvecs->clear(), tvecs->clear();
            cv::Mat r(3, 1, CV_64FC1), t(3, 1, CV_64FC1);
            for (int k = 0; k < 3; k++) r.at<double>(k, 0) = rv[3 * v + k], t.at<double>(k, 0) = tv[3 * v + k];
            rvecs->push_back(r), tvecs->push_back(t);
        }
        return rms;
    }

private:
    arucohip_fisheye_t model_() const {
        if (K.empty() || D.empty() || K.total() != 9 || D.total() != 4) arucohip_throw_(ARUCOHIP_E_INVALID, "FisheyeCamera: K (3x3) and D (4) are not set", nullptr);
        arucohip_fisheye_t m;
        for (int i = 0; i < 9; i++) m.K[i] = K(i / 3, i % 3);
        for (int i = 0; i < 4; i++) m.D[i] = D(i);
        return m;
    }
    void knew_(float kn[9]) const {
        const cv::Mat_<double>& src = (!newCameraMatrix.empty() && newCameraMatrix.total() == 9) ? newCameraMatrix : K;
        if (src.empty() || src.total() != 9) arucohip_throw_(ARUCOHIP_E_INVALID, "FisheyeCamera: K (3x3) is not set", nullptr);
        for (int i = 0; i < 9; i++) kn[i] = (float)src(i / 3, i % 3);
    }
};

// A chessboard whose white squares carry the markers (OpenCV's aruco module: CharucoBoard, interpolateCornersCharuco,
// estimatePoseCharucoBoard, calibrateCameraCharuco; no counterpart in the reference). The calibration points are the chessboard's inner
// corners: the markers of the detector's last frame say which corner is which, and each corner is refined in the frame
// (arucohip_charuco_corners_batch, include/arucohip.h). Corners are numbered row by row; one that was not found is left out.
class CharucoBoard {
public:
    arucohip_charuco_t layout;
    std::vector<int> ids;                       // marker k (row-major order of the white squares) shows ids[k]
    std::vector<int> cornerIds;                 // of the last detectCorners: the number of every found corner ...
    std::vector<cv::Point2f> corners;           // ... and where it is in the frame
    std::vector<arucohip_charuco_corner_t> records;   // every corner's record of the last detectCorners
    cv::Mat_<double> Rvec, Tvec;                // of the last estimatePose that gave a pose

    CharucoBoard() { layout.squares_x = layout.squares_y = layout.square_px = layout.marker_px = 0; }
    static CharucoBoard create(int squaresX, int squaresY, int squarePx, int markerPx, const std::vector<int>& markerIds) {
        CharucoBoard b;
        b.layout.squares_x = squaresX, b.layout.squares_y = squaresY, b.layout.square_px = squarePx, b.layout.marker_px = markerPx;
        int nm = 0;
        arucohip_throw_(arucohip_charuco_board_size(&b.layout, nullptr, nullptr, &nm, nullptr), "CharucoBoard::create: layout outside the limits", nullptr);
        if ((int)markerIds.size() != nm) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::create: one id per white square", nullptr);
        b.ids = markerIds;
        return b;
    }
    cv::Size size() const {
        int w = 0, h = 0;
        arucohip_throw_(arucohip_charuco_board_size(&layout, &w, &h, nullptr, nullptr), "CharucoBoard::size", nullptr);
        return cv::Size(w, h);
    }
    int cornerCount() const {
        int n = 0;
        arucohip_throw_(arucohip_charuco_board_size(&layout, nullptr, nullptr, nullptr, &n), "CharucoBoard::cornerCount", nullptr);
        return n;
    }
    // the board image, painted on the device; with `conf` the markers as a BoardConfiguration (PIX) for BoardDetector
    cv::Mat image(BoardConfiguration* conf = nullptr, bool centered = true) const {
        const cv::Size sz = size();
        cv::Mat img(sz.height, sz.width, CV_8UC1);
        std::vector<int32_t> id32(ids.begin(), ids.end());
        std::vector<float> obj(id32.size() * 12);
        SharedHandle_& sh = SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        arucohip_throw_(arucohip_charuco_board_image(h, &layout, centered ? 1 : 0, id32.data(), (int)id32.size(), img.data, img.step, 0, obj.data(), nullptr),
                        "CharucoBoard::image", h);
        if (conf) {
            conf->mInfoType = BoardConfiguration::PIX;
            conf->ids.assign(ids.begin(), ids.end());
            conf->objPoints.clear();
            for (size_t k = 0; k < id32.size(); k++) {
                std::vector<cv::Point3f> q(4);
                for (int c = 0; c < 4; c++) q[c].x = obj[12 * k + 3 * c], q[c].y = obj[12 * k + 3 * c + 1], q[c].z = obj[12 * k + 3 * c + 2];
                conf->objPoints.push_back(q);
            }
        }
        return img;
    }
    // the inner corners of `frame`, the gray frame the detector's last detect() saw; returns how many were found
    int detectCorners(MarkerDetector& detector, const cv::Mat& frame, int minMarkers = 2, int maxWin = 5) {
        if (frame.type() != CV_8UC1) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::detectCorners: the 8-bit gray frame of the last detect()", nullptr);
        arucohip_charuco_opt_t o;
        o.min_markers = minMarkers, o.max_win = maxWin;
        std::vector<int32_t> id32(ids.begin(), ids.end());
        records.assign((size_t)cornerCount(), arucohip_charuco_corner_t());
        int32_t n = 0;
        arucohip_handle* h = detector.handle();
        detector_ = &detector;
        arucohip_throw_(arucohip_charuco_corners_batch(h, &layout, id32.data(), (int)id32.size(), frame.data, 1, frame.cols, frame.rows, frame.step,
                                                       (size_t)frame.rows * frame.step, 0, &o, records.data(), &n, 0),
                        "CharucoBoard::detectCorners", h);
        cornerIds.clear(), corners.clear();
        for (size_t c = 0; c < records.size(); c++)
            if (records[c].found) {
                cv::Point2f p;
                p.x = records[c].x, p.y = records[c].y;
                cornerIds.push_back((int)c), corners.push_back(p);
            }
        return n;
    }
    // the board's pose from the corners of the last detectCorners; squareSize: the side of a square in the caller's unit (<= 0: board pixels)
    bool estimatePose(const CameraParameters& cp, float squareSize, bool setYPerpendicular = false, int minCorners = 4) {
        if (!detector_) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::estimatePose: no detectCorners before", nullptr);
        float K[9], d[8];
        const bool hasK = mat_to_K_(cp.CameraMatrix, K);
        const int nd = mat_to_dist_(cp.Distorsion, d);
        arucohip_handle* h = detector_->handle();
        arucohip_throw_(arucohip_charuco_pose_batch(h, 1, hasK ? K : nullptr, nd ? d : nullptr, nd, squareSize, minCorners, setYPerpendicular ? 1 : 0, &pose),
                        "CharucoBoard::estimatePose", h);
        if (pose.has_pose) {
            Rvec = cv::Mat_<double>(3, 1), Tvec = cv::Mat_<double>(3, 1);
            for (int k = 0; k < 3; k++) Rvec(k) = pose.rvec[k], Tvec(k) = pose.tvec[k];
        }
        return pose.has_pose != 0;
    }
    arucohip_board_t pose = arucohip_board_t();   // the last estimatePose, as the library returned it
    // cv::calibrateCamera over views of this board: allIds[v] / allCorners[v] as detectCorners left cornerIds / corners for view v
    double calibrate(const std::vector<std::vector<int> >& allIds, const std::vector<std::vector<cv::Point2f> >& allCorners, cv::Size imageSize,
                     float squareSize, cv::Mat& cameraMatrix, cv::Mat& distCoeffs, std::vector<cv::Mat>* rvecs = nullptr, std::vector<cv::Mat>* tvecs = nullptr,
                     int flags = 0) const {
        if (allIds.size() != allCorners.size()) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::calibrate: id and corner lists differ", nullptr);
        const int ncx = layout.squares_x - 1, nc = cornerCount();
        const double scale = squareSize > 0 ? (double)squareSize / (double)layout.square_px : 1.0;
        std::vector<std::vector<cv::Point3f> > obj(allIds.size());
        for (size_t v = 0; v < allIds.size(); v++) {
            if (allIds[v].size() != allCorners[v].size()) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::calibrate: a view's counts differ", nullptr);
            for (size_t i = 0; i < allIds[v].size(); i++) {
                const int c = allIds[v][i];
                if (c < 0 || c >= nc) arucohip_throw_(ARUCOHIP_E_INVALID, "CharucoBoard::calibrate: a corner number outside the board", nullptr);
                cv::Point3f p;
                p.x = (float)((float)((c % ncx + 1) * layout.square_px) * scale), p.y = (float)((float)((c / ncx + 1) * layout.square_px) * scale), p.z = 0.f;
                obj[v].push_back(p);
            }
        }
        std::vector<cv::Mat> rv, tv;
        return calibrateCamera(obj, allCorners, imageSize, cameraMatrix, distCoeffs, rvecs ? *rvecs : rv, tvecs ? *tvecs : tv, flags);
    }

private:
    MarkerDetector* detector_ = nullptr;
};

}  // namespace aruco

#if !ARUCOHIP_HAVE_OPENCV
namespace cv {
// the reference's apps spell it cv::undistort; without OpenCV the name resolves to the device implementation
inline void undistort(const Mat& src, Mat& dst, const Mat& cameraMatrix, const Mat& distCoeffs) { aruco::undistort(src, dst, cameraMatrix, distCoeffs); }
enum { CALIB_USE_INTRINSIC_GUESS = 1, CALIB_FIX_ASPECT_RATIO = 2, CALIB_FIX_PRINCIPAL_POINT = 4, CALIB_ZERO_TANGENT_DIST = 8,
       CALIB_FIX_FOCAL_LENGTH = 16, CALIB_FIX_K1 = 32, CALIB_FIX_K2 = 64, CALIB_FIX_K3 = 128 };
inline double calibrateCamera(const std::vector<std::vector<Point3f> >& objPointsV, const std::vector<std::vector<Point2f> >& imgPointsV, Size imageSize,
                              Mat& cameraMatrix, Mat& distCoeffs, std::vector<Mat>& rvecs, std::vector<Mat>& tvecs, int flags = 0) {
    return aruco::calibrateCamera(objPointsV, imgPointsV, imageSize, cameraMatrix, distCoeffs, rvecs, tvecs, flags);
}
}  // namespace cv
#endif

// ---- ChromaticMask / EMClassifier (src/chromaticmask.h:38-114) at global scope, as the reference declares them. The fit runs on the
// device (arucohip_em_fit / arucohip_chromatic_*); a ChromaticMask owns a small handle of its own for its device and stream.
class EMClassifier {
public:
    // the device fit discretises to the reference's default of 200 samples; another nelements is not supported
    EMClassifier(unsigned int nelements = 200) : _threshProb(0.0001) {
        if (nelements != 200) aruco::arucohip_throw_(ARUCOHIP_E_UNSUPPORTED, "EMClassifier: nelements other than 200", nullptr);
        for (int i = 0; i < 256; i++) _prob[i] = 0.5, _inside[i] = 0.5 > _threshProb;
    }
    void addSample(unsigned char s) { _samples.push_back(s); }
    void clearSamples() { _samples.clear(); }
    void train() {
        uint32_t hist[256] = {0};
        for (unsigned char s : _samples) hist[s]++;
        uint8_t inside[256];
        for (int i = 0; i < 256; i++) inside[i] = _inside[i];
        int trained = 0;
        aruco::SharedHandle_& sh = aruco::SharedHandle_::get();
        std::lock_guard<std::mutex> lock(sh.mu);
        arucohip_handle* h = sh.ensure();
        aruco::arucohip_throw_(arucohip_em_fit(h, hist, _threshProb, _prob, inside, &trained), "EMClassifier::train", h);
        for (int i = 0; i < 256; i++) _inside[i] = inside[i] != 0;
    }
    bool classify(unsigned char s) { return _inside[s]; }
    double getProb(unsigned char s) { return _prob[s]; }
    unsigned int numsamples() { return (unsigned int)_samples.size(); }
    void setProb(double p) { _threshProb = p; }

private:
    std::vector<unsigned char> _samples;
    bool _inside[256];
    double _prob[256];
    double _threshProb;
};

class ChromaticMask {
public:
    ChromaticMask() : _isValid(false) {}

    void setParams(unsigned int mc, unsigned int nc, double threshProb, aruco::CameraParameters CP, aruco::BoardConfiguration /*BC*/,
                   std::vector<cv::Point3f> corners) {
        if (corners.size() != 4) aruco::arucohip_throw_(ARUCOHIP_E_INVALID, "ChromaticMask::setParams: 4 corners", nullptr);
        float K[9], d[8], c[12];
        if (!aruco::mat_to_K_(CP.CameraMatrix, K)) aruco::arucohip_throw_(ARUCOHIP_E_INVALID, "ChromaticMask::setParams: camera matrix is empty", nullptr);
        const int nd = aruco::mat_to_dist_(CP.Distorsion, d);
        for (int i = 0; i < 4; i++) c[3 * i] = corners[i].x, c[3 * i + 1] = corners[i].y, c[3 * i + 2] = corners[i].z;
        std::shared_ptr<State> st(new State());
        const char* e = std::getenv("ARUCOHIP_DEVICE");
        aruco::arucohip_throw_(arucohip_create(nullptr, e ? std::atoi(e) : 0, 32, 32, 1, &st->h), "arucohip_create", nullptr);
        aruco::arucohip_throw_(arucohip_chromatic_create(st->h, (int)mc, (int)nc, threshProb, K, nd ? d : nullptr, nd, CP.CamSize.width,
                                                         CP.CamSize.height, c, &st->m),
                               "ChromaticMask::setParams", st->h);
        _st = st, _size = CP.CamSize, _isValid = false;
    }
    void setParams(unsigned int mc, unsigned int nc, double threshProb, aruco::CameraParameters CP, aruco::BoardConfiguration BC,
                   float markersize = -1.) {
        if (BC.mInfoType != aruco::BoardConfiguration::METERS && markersize == -1) {
            std::fprintf(stderr, "Invalid markersize in ChromaticMask::setParams\n");
            return;
        }
        if (BC.objPoints.size() == 0) {
            std::fprintf(stderr, "Invalid BoardConfiguration size in ChromaticMask::setParams\n");
            return;
        }
        std::vector<float> obj;
        for (const std::vector<cv::Point3f>& m : BC.objPoints)
            for (int j = 0; j < 4; j++) obj.push_back(m[j].x), obj.push_back(m[j].y), obj.push_back(m[j].z);
        float c[12];
        aruco::arucohip_throw_(arucohip_chromatic_board_corners(obj.data(), (int)BC.objPoints.size(), BC.mInfoType, markersize, c),
                               "ChromaticMask::setParams", nullptr);
        std::vector<cv::Point3f> corners;
        for (int i = 0; i < 4; i++) corners.push_back(cv::Point3f(c[3 * i], c[3 * i + 1], c[3 * i + 2]));
        setParams(mc, nc, threshProb, CP, BC, corners);
    }

    void calculateGridImage(const aruco::Board& board) {
        double r[3], t[3];
        pose_(board, r, t);
        aruco::arucohip_throw_(arucohip_chromatic_grid(st_(), r, t), "ChromaticMask::calculateGridImage", _st->h);
    }
    cv::Mat getCellMap() { return fetch_(arucohip_chromatic_get_cell_map); }
    cv::Mat getMask() { return fetch_(arucohip_chromatic_get_mask); }

    void train(const cv::Mat& in, const aruco::Board& board) {
        double r[3], t[3];
        pose_(board, r, t);
        check_(in);
        aruco::arucohip_throw_(arucohip_chromatic_train(st_(), in.data, 0, (size_t)in.step, r, t), "ChromaticMask::train", _st->h);
        _isValid = true;
    }
    void classify(const cv::Mat& in, const aruco::Board& board) { classify_(in, board, 1); }
    void classify2(const cv::Mat& in, const aruco::Board& board) { classify_(in, board, 2); }
    void update(const cv::Mat& in) {
        check_(in);
        aruco::arucohip_throw_(arucohip_chromatic_update(st_(), in.data, 0, (size_t)in.step), "ChromaticMask::update", _st->h);
    }

    bool isValid() { return _isValid; }
    void resetMask() { aruco::arucohip_throw_(arucohip_chromatic_reset_mask(st_()), "ChromaticMask::resetMask", _st->h); }

private:
    struct State {
        arucohip_handle* h = nullptr;
        arucohip_chromatic* m = nullptr;
        ~State() {
            arucohip_chromatic_destroy(m);
            arucohip_destroy(h);
        }
    };
    std::shared_ptr<State> _st;
    cv::Size _size;
    bool _isValid;

    arucohip_chromatic* st_() {
        if (!_st) aruco::arucohip_throw_(ARUCOHIP_E_INVALID, "ChromaticMask: setParams has not been called", nullptr);
        return _st->m;
    }
    static void pose_(const aruco::Board& b, double r[3], double t[3]) {
        if (b.Rvec.empty() || b.Tvec.empty()) aruco::arucohip_throw_(ARUCOHIP_E_INVALID, "ChromaticMask: the board has no pose", nullptr);
        for (int k = 0; k < 3; k++) r[k] = b.Rvec(k), t[k] = b.Tvec(k);
    }
    void check_(const cv::Mat& in) const {
        if (in.type() != CV_8UC1 || in.cols != _size.width || in.rows != _size.height)
            aruco::arucohip_throw_(ARUCOHIP_E_INVALID, "ChromaticMask: one 8-bit plane of CamSize", nullptr);
    }
    void classify_(const cv::Mat& in, const aruco::Board& board, int method) {
        double r[3], t[3];
        pose_(board, r, t);
        check_(in);
        aruco::arucohip_throw_(arucohip_chromatic_classify(st_(), in.data, 0, (size_t)in.step, r, t, method), "ChromaticMask::classify", _st->h);
    }
    cv::Mat fetch_(int (*get)(arucohip_chromatic*, uint8_t*, int)) {
        cv::Mat out(_size.height, _size.width, CV_8UC1);
        aruco::arucohip_throw_(get(st_(), out.data, 0), "ChromaticMask::getMask", _st->h);
        return out;
    }
};
