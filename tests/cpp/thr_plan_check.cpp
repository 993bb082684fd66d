// Walks thr_plan() (aruco_amd/csrc/thr_plan.h) over a grid of launches on the CPU and checks, at every point, the conditions the
// threshold kernels rely on. The first one is the reason this file exists: the strip kernel stores through ThrArgs::thres without a
// test, so a plan that leaves the byte image out while a plane runs the strip kernel is a store through a null-based pointer on the
// device. The conditions are restated here from the kernels' requirements, in arithmetic of their own (no tolerance: they are rules).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../aruco_amd/csrc/thr_plan.h"

static long failures = 0;
#define CHECK(cond)                                                                                                                    \
    do {                                                                                                                               \
        if (!(cond) && failures++ < 20)                                                                                                \
            fprintf(stderr, "FAIL %s: W %d H %d stride %zu gray+%d thres+%d method %d block %d C %d frames %d planes %d lazy %d edge %d plane %d\n", \
                    #cond, in.W, in.H, in.row_stride, (int)(in.gray & 15), (int)(in.thres & 15), in.method, blocks[0], in.idelta, in.nframes,  \
                    in.nthr, (int)in.lazy, (int)in.has_edge, t);                                                                     \
    } while (0)

// One plane on a 272 x 140 frame with everything 16-byte aligned, lazy: only the block size, C and the launch's size choose the kernel.
static ah::ThrPlan plan_of(int block, double C, int W = 272, int H = 140, int frames = 3) {
    static int blocks[1];
    blocks[0] = block;
    ah::ThrPlanIn in;
    in.W = W, in.H = H, in.row_stride = (size_t)W, in.frame_stride = (size_t)W * H;
    in.gray = 0x10000u, in.thres = 0x800000u;
    in.method = ARUCOHIP_THRES_ADPT, in.nthr = 1, in.block = blocks, in.idelta = (int)floor(C), in.nframes = frames, in.has_edge = true, in.lazy = true;
    return ah::thr_plan(in);
}

// The exact boundaries of the plan, as literals: the last C at which the packed 16-bit compare holds for a block size
// ((256 + |C|) b^2 + b^2 / 2 < 32768), the last C the eo kernel's folded constants take, and the launch sizes at which the segment height changes.
static long boundaries() {
    long bad = 0;
#define EXPECT(cond)                                      \
    do {                                                  \
        if (!(cond)) bad++, fprintf(stderr, "FAIL boundary: %s\n", #cond); \
    } while (0)
    for (int sgn = -1; sgn <= 1; sgn += 2) {
        // 9x9: 404 * 81 + 40 = 32764, 405 * 81 + 40 = 32845
        EXPECT(plan_of(9, sgn * 148).plane[0].family == ah::THR_WIDE && plan_of(9, sgn * 148).no_bytes);
        EXPECT(plan_of(9, sgn * 149).plane[0].family == ah::THR_STRIP && !plan_of(9, sgn * 149).plane[0].p16 && !plan_of(9, sgn * 149).no_bytes);
        // 11x11 never runs the 16-pixel kernels; its strip kernel packs up to 270 * 121 + 60 = 32730 (271 * 121 + 60 = 32851)
        EXPECT(plan_of(11, sgn * 14).plane[0].family == ah::THR_STRIP && plan_of(11, sgn * 14).plane[0].p16);
        EXPECT(plan_of(11, sgn * 15).plane[0].family == ah::THR_STRIP && !plan_of(11, sgn * 15).plane[0].p16);
        // 7x7: eo up to |C| = 200, wide up to 412 (668 * 49 + 24 = 32756, 669 * 49 + 24 = 32805), then the strip kernel in 32 bits
        EXPECT(plan_of(7, sgn * 200).plane[0].family == ah::THR_EO);
        EXPECT(plan_of(7, sgn * 201).plane[0].family == ah::THR_WIDE);
        EXPECT(plan_of(7, sgn * 412).plane[0].family == ah::THR_WIDE);
        EXPECT(plan_of(7, sgn * 413).plane[0].family == ah::THR_STRIP && !plan_of(7, sgn * 413).plane[0].p16 && plan_of(7, sgn * 413).plane[0].fast);
    }
    EXPECT(plan_of(7, -200.5).plane[0].family == ah::THR_WIDE);   // floor(-200.5) = -201
    EXPECT(plan_of(7, 200.5).plane[0].family == ah::THR_EO);      // floor(200.5) = 200
    // rows per wave: waves128 = strips * ceil(H / 128) * frames; 48 x 129 has 2 per frame, 48 x 128 one
    EXPECT(plan_of(7, 7, 48, 128, 127).plane[0].seg == 16);
    EXPECT(plan_of(7, 7, 48, 128, 128).plane[0].seg == 32);
    EXPECT(plan_of(7, 7, 48, 128, 511).plane[0].seg == 32);
    EXPECT(plan_of(7, 7, 48, 128, 512).plane[0].seg == 128);
    EXPECT(plan_of(7, 7, 48, 129, 63).plane[0].seg == 16 && plan_of(7, 7, 48, 129, 64).plane[0].seg == 32);
    EXPECT(plan_of(7, 7, 48, 129, 255).plane[0].seg == 32 && plan_of(7, 7, 48, 129, 256).plane[0].seg == 128);
    EXPECT(plan_of(5, 7, 2064, 136, 86).plane[0].seg == 128 && plan_of(5, 7, 2064, 136, 86).strips == 3);   // 3 * 2 * 86 = 516
    EXPECT(plan_of(5, 7, 2064, 136, 85).plane[0].seg == 32);                                                 // 510
#undef EXPECT
    return bad;
}

int main() {
    const int widths[] = {1, 4, 15, 16, 20, 640, 1024, 1920, 4112}, heights[] = {1, 8, 480, 1080}, pads[] = {0, 4, 16}, offs[] = {0, 4, 1};
    const int deltas[] = {-250, -201, -200, -149, -148, 0, 7, 148, 149, 200, 201, 250}, frames[] = {1, 4, 1024};
    const int methods[] = {ARUCOHIP_THRES_ADPT, ARUCOHIP_THRES_FIXED}, planes[] = {1, 3};
    long points = 0, lazy_points = 0, count[3] = {0, 0, 0};
    for (int W : widths) for (int H : heights) for (int pad : pads) for (int goff : offs) for (int toff : offs)
    for (int b = 3; b <= 31; b += 2) for (int C : deltas) for (int F : frames) for (int nthr : planes)
    for (int lazy = 0; lazy < 2; lazy++) for (int edge = 0; edge < 2; edge++) for (int method : methods) {
        const int blocks[3] = {b, 34 - b, 7};   // three planes: a small and a large block next to each other
        ah::ThrPlanIn in;
        in.W = W, in.H = H, in.row_stride = (size_t)(W + pad), in.frame_stride = in.row_stride * H;
        in.gray = 0x10000u + goff, in.thres = 0x800000u + toff;
        in.method = method, in.nthr = nthr, in.block = blocks, in.idelta = C, in.nframes = F, in.has_edge = edge, in.lazy = lazy;
        const ah::ThrPlan pl = ah::thr_plan(in);
        points++, lazy_points += pl.no_bytes;

        const bool fast = W % 4 == 0 && in.row_stride % 4 == 0 && in.frame_stride % 4 == 0 && in.gray % 4 == 0;
        const bool fast16 = W >= 16 && W % 16 == 0 && in.row_stride % 16 == 0 && in.frame_stride % 16 == 0 && in.gray % 16 == 0 && in.thres % 16 == 0;
        const int absC = C < 0 ? -C : C;
        const long waves128 = (long)((W + 1023) / 1024) * ((H + 127) / 128) * F;
        bool any_strip = false;
        int t = 0;
        for (; t < nthr; t++) {
            const ah::ThrPlanePlan& q = pl.plane[t];
            const long n = (long)blocks[t] * blocks[t], lim = (256 + absC) * n + n / 2;
            count[q.family]++;
            if (q.family == ah::THR_STRIP) {
                any_strip = true;
                CHECK(!pl.no_bytes);   // the null-store condition
                if (q.p16) CHECK(q.R <= 5 && lim < 32768 && fast);
                if (q.fast) CHECK(fast);
                CHECK(q.R == (method == ARUCOHIP_THRES_FIXED ? 0 : blocks[t] / 2));
            } else {
                CHECK(q.family == ah::THR_WIDE || q.family == ah::THR_EO);
                CHECK(method == ARUCOHIP_THRES_ADPT && q.R == blocks[t] / 2);
                CHECK(q.R <= 4 && fast16 && lim < 32768);
                if (q.family == ah::THR_EO) CHECK(q.R == 3 && absC <= 200);
                CHECK(q.seg == (waves128 >= 512 ? 128 : waves128 * 4 >= 512 ? 32 : 16));
                CHECK(pl.strips == (W + 1023) / 1024);
            }
        }
        t = -1;
        CHECK(pl.bitmap_pass == any_strip);
        if (method == ARUCOHIP_THRES_FIXED) CHECK(!pl.no_bytes);
        if (pl.no_bytes) CHECK(lazy && edge && method == ARUCOHIP_THRES_ADPT);
    }
    printf("thr_plan: %ld points, %ld without the byte image, planes strip %ld wide %ld eo %ld, %ld failures\n", points, lazy_points, count[0], count[1],
           count[2], failures);
    // the grid reaches every family and both answers about the byte image, or the checks above were vacuous
    if (!lazy_points || lazy_points == points || !count[0] || !count[1] || !count[2]) return 2;
    if (boundaries()) return 1;
    return failures ? 1 : 0;
}
