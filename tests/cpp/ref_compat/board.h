// What "board.h" resolves to when a caller of the reference is built against the MI355X path: aruco::BoardConfiguration and aruco::Board
// come from the shim (utils/aruco_create_board.cpp and aruco_board_pix2meters.cpp include it by this name and rely on it for <iostream>).
#pragma once
#include <iostream>

#include "aruco_hip_shim.hpp"
#if ARUCOHIP_HAVE_OPENCV && !defined(CV_VERSION)
#include "mock_opencv_extras.hpp"
#endif
