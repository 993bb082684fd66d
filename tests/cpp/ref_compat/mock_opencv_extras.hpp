// The few OpenCV calls the reference's generator utilities make beside the shim's classes (utils/aruco_create_board.cpp,
// aruco_selectoptimalmarkers.cpp, aruco_board_pix2meters.cpp), for builds against tests/cpp/mock_opencv: cv::getTickCount, cv::norm and
// the arithmetic on Point3f, CV_32SC1. board.h and arucofidmarkers.h include it only where the OpenCV on the include path is that mock
// (no CV_VERSION); a real OpenCV has all of them. Bodies are the minimum that links.
#pragma once
#include <cmath>

#include <opencv2/core.hpp>

#ifndef CV_32SC1
#define CV_32SC1 CV_MAKETYPE(4, 1)
#endif

namespace cv {
template <class T> Point3_<T> operator-(const Point3_<T>& a, const Point3_<T>& b) { return Point3_<T>(a.x - b.x, a.y - b.y, a.z - b.z); }
template <class T> Point3_<T>& operator*=(Point3_<T>& a, float b) {
    a.x = (T)(a.x * b), a.y = (T)(a.y * b), a.z = (T)(a.z * b);
    return a;
}
template <class T> double norm(const Point3_<T>& p) { return std::sqrt((double)p.x * p.x + (double)p.y * p.y + (double)p.z * p.z); }
inline long long getTickCount() { return 0; }
}  // namespace cv
