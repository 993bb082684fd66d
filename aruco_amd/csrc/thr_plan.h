// Which threshold kernel runs on each plane of a launch (k_threshold.hip executes the plan; the kernel families are indexed there).
// Host-only and free of HIP types: tests/cpp/thr_plan_check.cpp walks it on the CPU. Every condition the kernels rely on lives here
// once. The one that must never drift: a plane of the strip kernel stores through ThrArgs::thres without a test, so the byte image may
// only be left out when no plane runs it - `no_bytes` is derived from the planes' families, not from a second copy of their conditions.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/arucohip.h"

namespace ah {

enum ThrFamily { THR_STRIP, THR_WIDE, THR_EO };
constexpr int THR_WSTRIP = 1024;   // pixels per wave and row of the wide / eo kernels

struct ThrPlanePlan {
    ThrFamily family;
    int R;             // block radius b/2 (the kernels' template argument); 0 with the FIXED method
    bool p16, fast;    // strip kernel: its P16 / FAST template arguments
    int seg;           // wide / eo kernel: rows per wave (16, 32 or 128)
};

struct ThrPlan {
    ThrPlanePlan plane[16];
    int strips;        // wide / eo kernel: strips per row
    bool no_bytes;     // the byte image is left out: thres = null and edge = buf.thres_edge for every plane, else for none
    bool bitmap_pass;  // some plane's kernel (the strip kernel) wrote no non-empty-tile bitmap: launch_tile_bitmap follows
};

struct ThrPlanIn {
    int W, H;
    size_t row_stride, frame_stride;   // of the gray frames
    uintptr_t gray, thres;             // addresses of the gray frames and of buf.thres: their alignment counts
    int method, nthr;                  // ARUCOHIP_THRES_FIXED, else adaptive; planes per frame (<= 16)
    const int* block;                  // [nthr] adaptive block sizes, odd, 3..31
    int idelta, nframes;               // adaptive: floor(C)
    bool has_edge, lazy;               // buf.thres_edge exists; the caller does not need the byte image now
};

// dword loads and stores: width, strides and base address are multiples of 4
inline bool thr_fast(int W, size_t row_stride, size_t frame_stride, uintptr_t gray) {
    return ((W | (int)(row_stride & 3) | (int)(frame_stride & 3) | (int)(gray & 3)) & 3) == 0;
}
// 16-byte loads and stores of the 16-pixel-per-lane kernels: ... multiples of 16, the byte image too, and at least one full lane
inline bool thr_fast16(int W, size_t row_stride, size_t frame_stride, uintptr_t gray, uintptr_t thres) {
    return W >= 16 && ((W | (int)(row_stride & 15) | (int)(frame_stride & 15) | (int)(gray & 15) | (int)(thres & 15)) & 15) == 0;
}
inline ThrPlan thr_plan(const ThrPlanIn& in) {
    ThrPlan pl{};
    const bool fast = thr_fast(in.W, in.row_stride, in.frame_stride, in.gray);
    const bool fast16 = thr_fast16(in.W, in.row_stride, in.frame_stride, in.gray, in.thres);
    pl.strips = (in.W + THR_WSTRIP - 1) / THR_WSTRIP;
    // Rows per wave of the 16-pixel-per-lane kernels. A wave walks down its segment row by row: a launch of few frames gets shorter
    // segments so that it still spreads over the chip (one 640x480 frame: 4 waves of 128 rows took 91 us; 2R extra rows per segment are
    // re-read, which only small launches can afford). 128 rows are the best of the sweep in profiles/r02_threshold_sweep.txt.
    const long waves128 = (long)pl.strips * ((in.H + 127) / 128) * in.nframes;
    const int seg = waves128 >= 512 ? 128 : waves128 * 4 >= 512 ? 32 : 16;
    for (int t = 0; t < in.nthr; t++) {
        ThrPlanePlan& q = pl.plane[t];
        q.family = THR_STRIP, q.fast = fast;
        if (in.method != ARUCOHIP_THRES_FIXED) {
            // the packed 16-bit compare holds (255 + |C| + 1) * b^2 + b^2/2 in a signed half
            const long n = (long)in.block[t] * in.block[t];
            const bool half = (256 + labs((long)in.idelta)) * n + n / 2 < 32768;
            q.R = in.block[t] / 2;
            if (q.R <= 4 && fast16 && half)   // the eo kernel is the 7x7 form of the wide one; its folded constants want a moderate C
                q.family = q.R == 3 && abs(in.idelta) <= 200 ? THR_EO : THR_WIDE, q.seg = seg;
            else
                q.p16 = fast && q.R <= 5 && half;
        }
        if (q.family == THR_STRIP) pl.bitmap_pass = true;
    }
    pl.no_bytes = in.lazy && in.method == ARUCOHIP_THRES_ADPT && in.has_edge && !pl.bitmap_pass;
    return pl;
}

}  // namespace ah
