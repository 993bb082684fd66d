// Fisheye lenses (equidistant model, fisheye_device.h): detected corners and whole frames are mapped once from the fisheye image to the
// image of an ideal pinhole camera Knew; every pinhole solver of the library then runs unchanged with K = Knew and no distortion.
//   - fisheye_points_kernel: n pixel pairs in either direction, one lane per point, double arithmetic, one rounding to float;
//   - fisheye_markers_kernel: the resident marker lists of a batch in place, one wave per frame; markers with an invalid corner leave
//     the list, which closes up in order;
//   - fisheye_map_kernel: the remap table of a frame in the CV_16SC2 form remap_linear_kernel (k_undistort.hip) reads, one thread per
//     destination pixel.
#include "fisheye_device.h"
#include "internal.h"

namespace ah {

struct FisheyePointsArgs {
    FisheyeCam cam;
    const float* src;   // [n][2]
    float* dst;         // [n][2]
    uint8_t* valid;     // [n], undistort only
    int n, undistort;
};

__global__ __launch_bounds__(256) void fisheye_points_kernel(FisheyePointsArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double u = (double)a.src[2 * i], v = (double)a.src[2 * i + 1];
    double ou = 0, ov = 0;
    if (a.undistort) {
        double xn, yn;
        const bool ok = fisheye_unproject(a.cam, u, v, &xn, &yn);
        if (ok) fisheye_ideal_pixel(a.cam, xn, yn, &ou, &ov);
        a.valid[i] = ok ? 1 : 0;
    } else {
        double X, Y, Z, th;
        fisheye_ideal_ray(a.cam, u, v, &X, &Y, &Z);
        fisheye_project(a.cam, X, Y, Z, &ou, &ov, &th);
    }
    a.dst[2 * i] = (float)ou, a.dst[2 * i + 1] = (float)ov;
}

struct FisheyeMarkersArgs {
    const FisheyeCam* cams;   // [nmodels]
    int nmodels, first, nframes, cap_markers;   // first: the batch index of this worker's frame 0
    arucohip_marker_t* markers;   // [nframes][cap_markers]
    int32_t* nmarkers;            // [nframes]
    int32_t* dropped;             // [nframes]
};

// One wave per frame, one lane per marker, 64 markers at a time: every lane holds its marker in registers before any lane stores, and
// a marker only moves towards the front, so the list closes up in place.
__global__ __launch_bounds__(WAVE) void fisheye_markers_kernel(FisheyeMarkersArgs a) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= a.nframes) return;
    const int n_in = a.nmarkers[f];
    if (n_in < 0) {
        if (lane == 0) a.dropped[f] = 0;
        return;
    }
    const int n = min(n_in, a.cap_markers);
    const FisheyeCam cam = a.cams[(a.first + f) % a.nmodels];
    arucohip_marker_t* list = a.markers + (size_t)f * a.cap_markers;
    int kept = 0;
    for (int base = 0; base < n; base += WAVE) {
        const int i = base + lane;
        arucohip_marker_t m;
        bool ok = i < n;
        if (ok) {
            m = list[i];
            for (int c = 0; c < 4; c++) {
                double xn, yn, u, v;
                if (!fisheye_unproject(cam, (double)m.corners[2 * c], (double)m.corners[2 * c + 1], &xn, &yn)) {
                    ok = false;
                    break;
                }
                fisheye_ideal_pixel(cam, xn, yn, &u, &v);
                m.corners[2 * c] = (float)u, m.corners[2 * c + 1] = (float)v;
            }
            // a pose the batch computed came from the wrong camera model
            m.has_pose = 0, m.ssize = -1.f;
        }
        const unsigned long long keep = __ballot(ok);
        if (ok) list[kept + __popcll(keep & ((1ull << lane) - 1ull))] = m;
        kept += __popcll(keep);
    }
    if (lane == 0) a.nmarkers[f] = kept, a.dropped[f] = n - kept;
}

struct FisheyeMapArgs {
    FisheyeCam cam;
    int width, height;
    short2* xy;
    uint16_t* fxy;
};

__global__ __launch_bounds__(256) void fisheye_map_kernel(FisheyeMapArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t pix = (size_t)y * a.width + x;
    double X, Y, Z, u, v, th;
    fisheye_ideal_ray(a.cam, (double)x, (double)y, &X, &Y, &Z);
    fisheye_project(a.cam, X, Y, Z, &u, &v, &th);
    if (!(th <= a.cam.max_angle)) {   // beyond the lens: a source position outside every frame (constant 0)
        a.xy[pix] = make_short2((short)-32768, (short)-32768);
        a.fxy[pix] = 0;
        return;
    }
    // round half to even, kept inside what the 16-bit integer part holds
    const double lo = -32768.0 * 32, hi = 32767.0 * 32 + 31;
    const int iu = __double2int_rn(fmax(lo, fmin(hi, u * 32)));
    const int iv = __double2int_rn(fmax(lo, fmin(hi, v * 32)));
    a.xy[pix] = make_short2((short)(iu >> 5), (short)(iv >> 5));
    a.fxy[pix] = (uint16_t)((iv & 31) * 32 + (iu & 31));
}

void launch_fisheye_points(hipStream_t s, const FisheyeCam& cam, const float* src, int n, int undistort, float* dst, uint8_t* valid) {
    FisheyePointsArgs a{cam, src, dst, valid, n, undistort};
    hipLaunchKernelGGL(fisheye_points_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

void launch_fisheye_markers(hipStream_t s, const FisheyeCam* cams, int nmodels, int first, int nframes, const Buffers& b, int32_t* dropped) {
    FisheyeMarkersArgs a{cams, nmodels, first, nframes, b.cap_markers, b.markers, b.nmarkers, dropped};
    hipLaunchKernelGGL(fisheye_markers_kernel, dim3(nframes), dim3(WAVE), 0, s, a);
}

void launch_fisheye_map(hipStream_t s, const FisheyeCam& cam, int W, int H, short2* xy, uint16_t* fxy) {
    FisheyeMapArgs a{cam, W, H, xy, fxy};
    hipLaunchKernelGGL(fisheye_map_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, a);
}

}  // namespace ah
