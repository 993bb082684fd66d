// Host side of plane rectification (k_rectify.hip): argument checks, the window of a board, staging of host arguments, the launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the arguments both entry points share, as the caller gave them
struct Call {
    Images src;
    int w, ch;
    const float *K, *dist;
    int ndist;
    Images dst;
    int ow;
};
Call make_call(const uint8_t* src, int n, int w, int h, int ch, size_t row, size_t frame, int src_on_device, const float* K, const float* dist, int ndist,
               uint8_t* dst, int ow, int oh, size_t drow, size_t dframe, int dst_on_device) {
    return {images(src, n, h, (size_t)w * ch, row, frame, src_on_device), w, ch, K, dist, ndist,
            images(dst, n, oh, (size_t)ow * ch, drow, dframe, dst_on_device), ow};
}

int check_call(arucohip_handle* h, const Call& c, bool need_K) {
    if (!c.src.p) return fail(h, ARUCOHIP_E_INVALID, "rectify: src (the frames) is NULL");
    if (!c.dst.p) return fail(h, ARUCOHIP_E_INVALID, "rectify: dst is NULL");
    if (c.src.n < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: nframes is below 1");
    if (c.w < 1 || c.src.rows < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: width / height is below 1");
    if (c.ch != 1 && c.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "rectify: channels must be 1 or 3");
    if (const int rc = check_plane_camera(h, "rectify", need_K, c.K, c.dist, c.ndist)) return rc;
    if (c.ow < 1 || c.dst.rows < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: out_width / out_height is below 1");
    if (c.ow > 16383 || c.dst.rows > 16383) return fail(h, ARUCOHIP_E_INVALID, "rectify: out_width / out_height is above 16383");
    if (const int rc = check_strides(h, "rectify", "", c.src)) return rc;
    if (const int rc = check_strides(h, "rectify", "dst_", c.dst)) return rc;
    return check_disjoint(h, "rectify", "dst", c.dst, "src", c.src);
}

// The one layout of a call in the handle's arena: the plane maps it uploads or computes (n_maps frames; 0: the caller's are on the
// device), the staged host frames and the images a host caller gets, tightly packed.
struct Scratch {
    PlaneMaps m;
    size_t src_at, dst_at;
};
int carve(arucohip_handle* h, const Call& c, int n_maps, Scratch* sc) {
    return carve_scratch(h, h, [&](Carver& cv) {
        carve_plane_maps(cv, n_maps, &sc->m);
        sc->src_at = cv.take_at(c.src.on_device ? 0 : c.src.packed_bytes());
        sc->dst_at = cv.take_at(c.dst.on_device ? 0 : c.dst.packed_bytes());
    });
}

// The resampling of a checked call with device maps: host frames go up, host images come back. Queues only; the caller synchronises.
int warp(arucohip_handle* h, const Call& c, const Scratch& sc, const double* maps, const int32_t* valid) {
    DevImages src, dst;
    if (const int rc = stage_input(h, h->stream, c.src, h->scratch, sc.src_at, &src)) return rc;
    if (const int rc = stage_output(h, c.dst, h->scratch, sc.dst_at, &dst)) return rc;
    PlaneWarp a;
    std::memset(&a, 0, sizeof(a));
    a.src = src.p, a.row_stride = src.row, a.frame_stride = src.frame;
    a.dst = dst.p, a.dst_row_stride = dst.row, a.dst_frame_stride = dst.frame;
    a.width = c.w, a.height = c.src.rows, a.out_width = c.ow, a.out_height = c.dst.rows;
    a.maps = maps, a.valid = valid;
    a.fx = c.K ? (double)c.K[0] : 1.0, a.fy = c.K ? (double)c.K[4] : 1.0, a.cx = c.K ? (double)c.K[2] : 0.0, a.cy = c.K ? (double)c.K[5] : 0.0;
    for (int i = 0; i < c.ndist; i++) a.k[i] = (double)c.dist[i];
    launch_plane_warp(h->stream, a, c.ch, c.ndist > 0, c.src.n);
    HIPCHK(h, hipGetLastError());
    return unstage(h, h->stream, c.dst, dst);
}

}  // namespace

extern "C" {

int arucohip_warp_plane_batch(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, int channels, size_t row_stride,
                              size_t frame_stride, int src_on_device, const double* maps, const int32_t* valid, int maps_on_device,
                              const float* K, const float* dist, int ndist, uint8_t* dst, int out_width, int out_height,
                              size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = make_call(src, nframes, width, height, channels, row_stride, frame_stride, src_on_device, K, dist, ndist, dst, out_width, out_height,
                             dst_row_stride, dst_frame_stride, dst_on_device);
    if (!maps) return fail(h, ARUCOHIP_E_INVALID, "rectify: maps is NULL");
    if (const int rc = check_call(h, c, false)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    Scratch sc;
    if (const int rc = carve(h, c, maps_on_device ? 0 : nframes, &sc)) return rc;
    if (const int rc = stage_plane_maps(h, sc.m, nframes, maps_on_device, &maps, &valid)) return rc;
    if (const int rc = warp(h, c, sc, maps, valid)) return rc;
    if (!src_on_device || !maps_on_device || !dst_on_device) HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_rectify_board_window(const float* obj, int nboard, int info_type, float marker_size, float px_per_unit, float margin, int flip_y,
                                  arucohip_rectify_t* win) {
    if (!obj || !win || nboard < 1 || !(px_per_unit > 0) || !std::isfinite(px_per_unit) || !std::isfinite(margin)) return ARUCOHIP_E_INVALID;
    const BoardDef bd = {nullptr, obj, nboard, info_type, marker_size, 0.f};
    const double unit = board_mpp(bd), ppu = px_per_unit, step = 1.0 / ppu, m = margin;
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    for (int i = 0; i < nboard * 4; i++)
        for (int k = 0; k < 2; k++) {
            const double v = (double)obj[3 * i + k] * unit;
            lo[k] = std::min(lo[k], v), hi[k] = std::max(hi[k], v);
        }
    int size[2];
    for (int k = 0; k < 2; k++) {
        const double px = (hi[k] - lo[k] + 2 * m) * ppu;   // an extent a rounding above a whole number of pixels is that number
        if (!(px > 0) || !(px <= 16383)) return ARUCOHIP_E_INVALID;
        size[k] = (int)std::max(1.0, std::ceil(px - 1e-6 * px));
    }
    win->out_width = size[0], win->out_height = size[1];
    win->x0 = (float)(lo[0] - m + step / 2), win->ux = (float)step, win->uy = 0.f;
    win->vx = 0.f;
    win->y0 = flip_y ? (float)(hi[1] + m - step / 2) : (float)(lo[1] - m + step / 2);
    win->vy = flip_y ? (float)-step : (float)step;
    return ARUCOHIP_OK;
}

int arucohip_board_rectify_batch(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, int channels,
                                 size_t row_stride, size_t frame_stride, int frames_on_device, const arucohip_board_t* boards,
                                 int boards_on_device, const float* K, const float* dist, int ndist, const arucohip_rectify_t* win,
                                 uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device, int32_t* status,
                                 double* maps_out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!boards) return fail(h, ARUCOHIP_E_INVALID, "rectify: boards is NULL");
    if (!win) return fail(h, ARUCOHIP_E_INVALID, "rectify: win (the window) is NULL");
    const Call c = make_call(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, K, dist, ndist, dst, win->out_width,
                             win->out_height, dst_row_stride, dst_frame_stride, dst_on_device);
    if (const int rc = check_call(h, c, true)) return rc;
    if (!window_spans_plane(*win))
        return fail(h, ARUCOHIP_E_INVALID, "rectify: the window's u and v steps are parallel, zero or not finite");
    HIPCHK(h, hipSetDevice(h->device));
    Scratch sc;
    if (const int rc = carve(h, c, nframes, &sc)) return rc;
    if (const int rc = plane_maps_of_boards(h, sc.m, launch_plane_maps, boards, boards_on_device, nframes, *win)) return rc;
    if (const int rc = warp(h, c, sc, sc.m.maps, sc.m.valid)) return rc;
    if (const int rc = read_plane_maps(h, sc.m, nframes, status, maps_out)) return rc;
    if (!frames_on_device || !boards_on_device || !dst_on_device || status || maps_out) HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

}  // extern "C"
