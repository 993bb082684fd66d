// Host side of plane rectification (k_rectify.hip): argument checks, the window of a board, staging of host arguments, the launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the arguments both entry points share, as the caller gave them
struct Call {
    const uint8_t* src;
    int n, w, h, ch;
    size_t row, frame;
    int src_on_device;
    const float *K, *dist;
    int ndist;
    uint8_t* dst;
    int ow, oh;
    size_t drow, dframe;
    int dst_on_device;
    size_t src_row_bytes() const { return (size_t)w * ch; }
    size_t dst_row_bytes() const { return (size_t)ow * ch; }
    size_t src_extent() const { return (size_t)(n - 1) * frame + (size_t)(h - 1) * row + src_row_bytes(); }
    size_t dst_extent() const { return (size_t)(n - 1) * dframe + (size_t)(oh - 1) * drow + dst_row_bytes(); }
};

int check_call(arucohip_handle* h, const Call& c, bool need_K) {
    if (!c.src) return fail(h, ARUCOHIP_E_INVALID, "rectify: src (the frames) is NULL");
    if (!c.dst) return fail(h, ARUCOHIP_E_INVALID, "rectify: dst is NULL");
    if (c.n < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: nframes is below 1");
    if (c.w < 1 || c.h < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: width / height is below 1");
    if (c.ch != 1 && c.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "rectify: channels must be 1 or 3");
    if (need_K && !c.K) return fail(h, ARUCOHIP_E_INVALID, "rectify: K is NULL (the board call needs the camera)");
    if (!(c.ndist == 0 || c.ndist == 4 || c.ndist == 5 || c.ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "rectify: ndist must be 0, 4, 5 or 8");
    if (c.ndist > 0 && !c.dist) return fail(h, ARUCOHIP_E_INVALID, "rectify: dist is NULL with ndist > 0");
    if (c.ndist > 0 && !c.K) return fail(h, ARUCOHIP_E_INVALID, "rectify: dist without K");
    if (c.ow < 1 || c.oh < 1) return fail(h, ARUCOHIP_E_INVALID, "rectify: out_width / out_height is below 1");
    if (c.ow > 16383 || c.oh > 16383) return fail(h, ARUCOHIP_E_INVALID, "rectify: out_width / out_height is above 16383");
    if (c.row < c.src_row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "rectify: row_stride is smaller than width * channels");
    if (c.n > 1 && c.frame < (size_t)(c.h - 1) * c.row + c.src_row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "rectify: frame_stride is smaller than a frame");
    if (c.drow < c.dst_row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "rectify: dst_row_stride is smaller than out_width * channels");
    if (c.n > 1 && c.dframe < (size_t)(c.oh - 1) * c.drow + c.dst_row_bytes())
        return fail(h, ARUCOHIP_E_INVALID, "rectify: dst_frame_stride is smaller than an image");
    // host and device addresses share one space, so one comparison serves every combination
    const uintptr_t s0 = (uintptr_t)c.src, d0 = (uintptr_t)c.dst;
    if (s0 < d0 + c.dst_extent() && d0 < s0 + c.src_extent()) return fail(h, ARUCOHIP_E_INVALID, "rectify: dst overlaps src");
    return ARUCOHIP_OK;
}

// one call's scratch in d_rectify
struct Scratch {
    double* maps;
    int32_t* valid;
    arucohip_board_t* boards;
};
size_t scratch_layout(uint8_t* base, int n, Scratch* s) {
    Carver cv{base};
    s->maps = cv.take<double>((size_t)n * 9);
    s->valid = cv.take<int32_t>((size_t)n);
    s->boards = cv.take<arucohip_board_t>((size_t)n);
    return cv.at;
}
int reserve_scratch(arucohip_handle* h, int n, Scratch* s) {
    HIPCHK(h, h->d_rectify.reserve(scratch_layout(nullptr, n, s)));
    scratch_layout(h->d_rectify, n, s);
    return ARUCOHIP_OK;
}

// The resampling of a checked call with device maps: host frames go up, host images come back. Queues only; the caller synchronises.
int warp(arucohip_handle* h, const Call& c, const double* maps, const int32_t* valid) {
    const size_t src_bytes = c.src_on_device ? 0 : ((size_t)c.n * c.h * c.src_row_bytes() + 255) & ~(size_t)255;
    const size_t dst_bytes = c.dst_on_device ? 0 : (size_t)c.n * c.oh * c.dst_row_bytes();
    HIPCHK(h, h->d_rectify_frames.reserve(src_bytes + dst_bytes));
    PlaneWarp a;
    std::memset(&a, 0, sizeof(a));
    a.src = c.src, a.row_stride = c.row, a.frame_stride = c.frame;
    if (!c.src_on_device) {
        if (const int rc = copy_rows(h, const_cast<uint8_t*>(c.src), c.row, c.frame, c.src_row_bytes(), c.h, c.n, h->d_rectify_frames, true)) return rc;
        a.src = h->d_rectify_frames, a.row_stride = c.src_row_bytes(), a.frame_stride = (size_t)c.h * c.src_row_bytes();
    }
    a.dst = c.dst, a.dst_row_stride = c.drow, a.dst_frame_stride = c.dframe;
    if (!c.dst_on_device) a.dst = h->d_rectify_frames + src_bytes, a.dst_row_stride = c.dst_row_bytes(), a.dst_frame_stride = (size_t)c.oh * c.dst_row_bytes();
    a.width = c.w, a.height = c.h, a.out_width = c.ow, a.out_height = c.oh;
    a.maps = maps, a.valid = valid;
    a.fx = c.K ? (double)c.K[0] : 1.0, a.fy = c.K ? (double)c.K[4] : 1.0, a.cx = c.K ? (double)c.K[2] : 0.0, a.cy = c.K ? (double)c.K[5] : 0.0;
    for (int i = 0; i < c.ndist; i++) a.k[i] = (double)c.dist[i];
    launch_plane_warp(h->stream, a, c.ch, c.ndist > 0, c.n);
    HIPCHK(h, hipGetLastError());
    if (!c.dst_on_device) return copy_rows(h, c.dst, c.drow, c.dframe, c.dst_row_bytes(), c.oh, c.n, a.dst, false);
    return ARUCOHIP_OK;
}

}  // namespace

extern "C" {

int arucohip_warp_plane_batch(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, int channels, size_t row_stride,
                              size_t frame_stride, int src_on_device, const double* maps, const int32_t* valid, int maps_on_device,
                              const float* K, const float* dist, int ndist, uint8_t* dst, int out_width, int out_height,
                              size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = {src, nframes, width, height, channels, row_stride, frame_stride, src_on_device, K, dist, ndist,
                    dst, out_width, out_height, dst_row_stride, dst_frame_stride, dst_on_device};
    if (!maps) return fail(h, ARUCOHIP_E_INVALID, "rectify: maps is NULL");
    if (const int rc = check_call(h, c, false)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (!maps_on_device) {
        Scratch sc;
        if (const int rc = reserve_scratch(h, nframes, &sc)) return rc;
        HIPCHK(h, hipMemcpyAsync(sc.maps, maps, (size_t)nframes * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        maps = sc.maps;
        if (valid) {
            HIPCHK(h, hipMemcpyAsync(sc.valid, valid, (size_t)nframes * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            valid = sc.valid;
        }
    }
    if (const int rc = warp(h, c, maps, valid)) return rc;
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
    const Call c = {frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, K, dist, ndist,
                    dst, win->out_width, win->out_height, dst_row_stride, dst_frame_stride, dst_on_device};
    if (const int rc = check_call(h, c, true)) return rc;
    if (!window_spans_plane(*win))
        return fail(h, ARUCOHIP_E_INVALID, "rectify: the window's u and v steps are parallel, zero or not finite");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    Scratch sc;
    if (const int rc = reserve_scratch(h, nframes, &sc)) return rc;
    if (!boards_on_device) {
        HIPCHK(h, hipMemcpyAsync(sc.boards, boards, (size_t)nframes * sizeof(arucohip_board_t), hipMemcpyHostToDevice, s));
        boards = sc.boards;
    }
    launch_plane_maps(s, boards, nframes, *win, sc.maps, sc.valid);
    HIPCHK(h, hipGetLastError());
    if (const int rc = warp(h, c, sc.maps, sc.valid)) return rc;
    if (status) HIPCHK(h, hipMemcpyAsync(status, sc.valid, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (maps_out) HIPCHK(h, hipMemcpyAsync(maps_out, sc.maps, (size_t)nframes * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (!frames_on_device || !boards_on_device || !dst_on_device || status || maps_out) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
