// border_rect (aruco_amd/csrc/border_rect.h), the border filter's rectangle, printed for a table of frame sizes and border distances:
// one line "W H t x0 y0 x1 y1" each, t with nine significant digits. tests/test_tail_cpu.py compares the lines with the plain
// restatement of markerdetector.cpp:433-434. Host C++ only.
#include <stdio.h>
#include <stdlib.h>

#include "../../aruco_amd/csrc/border_rect.h"

int main(int argc, char** argv) {
    // arguments: W H t triples; the test passes its own table, so the two sides cannot drift apart
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: border_rect_check W H t [W H t ...]\n");
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const int W = atoi(argv[i]), H = atoi(argv[i + 1]);
        const float t = strtof(argv[i + 2], nullptr);
        int r[4];
        border_rect(t, W, H, r);
        printf("%d %d %.9g %d %d %d %d\n", W, H, (double)t, r[0], r[1], r[2], r[3]);
    }
    return 0;
}
