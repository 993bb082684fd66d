// The border filter's rectangle (markerdetector.cpp:433-434). Host-only and free of HIP types: tests/cpp/border_rect_check.cpp prints it
// with the host compiler, make_detect_params (capi.hip) hands it to finalize_kernel.
#pragma once
#include <algorithm>
#include <cmath>

// [r[0], r[2]) x [r[1], r[3]) of a W x H frame: Rect(Point(size) * t, Point(size) * (1 - t)). Point * float multiplies in float and rounds
// with cvRound (half to even); Rect(pt1, pt2) sorts the two points with min / max, so t > 0.5 gives a rectangle too and t = 0.5 an empty one
inline void border_rect(float border_dist, int W, int H, int r[4]) {
    const int x1 = (int)lrintf((float)W * border_dist), y1 = (int)lrintf((float)H * border_dist);
    const int x2 = (int)lrintf((float)W * (1.0f - border_dist)), y2 = (int)lrintf((float)H * (1.0f - border_dist));
    r[0] = std::min(x1, x2), r[1] = std::min(y1, y2), r[2] = std::max(x1, x2), r[3] = std::max(y1, y2);
}
