// What "arucofidmarkers.h" resolves to when a caller of the reference is built against the MI355X path: aruco::FiducidalMarkers comes
// from the shim (utils/aruco_create_marker.cpp, aruco_create_board.cpp and aruco_selectoptimalmarkers.cpp include it by this name).
#pragma once
#include "aruco_hip_shim.hpp"
#if ARUCOHIP_HAVE_OPENCV && !defined(CV_VERSION)
#include "mock_opencv_extras.hpp"
#endif
