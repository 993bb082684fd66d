// Host side of the overlay pass (k_overlay.hip): argument checks, staging of host arguments, the chunked build + raster launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the frames of a call, drawn into in place
struct Frames {
    Images im;
    int w, ch;
};
Frames make_frames(uint8_t* p, int n, int w, int h, int ch, size_t row, size_t frame, int on_device) {
    return {images(p, n, h, (size_t)w * ch, row, frame, on_device), w, ch};
}

int check_frames(arucohip_handle* h, const Frames& f) {
    if (!f.im.p || f.im.n < 1 || f.w < 1 || f.im.rows < 1) return fail(h, ARUCOHIP_E_INVALID, "draw: NULL frames, or nframes / width / height below 1");
    if (f.ch != 1 && f.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "draw: channels must be 1 or 3");
    if (const int rc = check_strides(h, "draw", "", f.im)) return rc;
    if (f.w > h->lim.max_width || f.im.rows > h->lim.max_height) return fail(h, ARUCOHIP_E_UNSUPPORTED, "draw: width / height exceed the handle's limits");
    return ARUCOHIP_OK;
}

int check_camera(arucohip_handle* h, bool need_K, const float* K, const float* dist, int ndist, CamModel* cam) {
    if (need_K && !K) return fail(h, ARUCOHIP_E_INVALID, "draw: K is required for ARUCOHIP_DRAW_AXIS / ARUCOHIP_DRAW_CUBE");
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0, 4, 5 or 8");
    if (ndist > 0 && !dist) return fail(h, ARUCOHIP_E_INVALID, "draw: dist is NULL with ndist > 0");
    fill_cam(cam, K, dist, ndist, 0.f, 0);
    return ARUCOHIP_OK;
}

// The common part: `slots` marker slots per frame (1 for boards). src / counts: device pointers, or host arrays of `elem` bytes per slot
// that are staged behind the primitive lists in the handle's arena, with host frames behind them, tightly packed.
// build(frames0, nframes, src, counts, recs, prims) enqueues the build kernel of one chunk.
template <typename Build>
int draw(arucohip_handle* h, const Frames& f, const void* src, size_t elem, int slots, const int32_t* counts, int src_on_device, Build build) {
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // the scratch holds the primitive lists of a chunk of frames: at most 64 MiB (and 65535 frames, the grid's z limit), at least one frame
    const size_t per_frame = (size_t)slots * (OV_REC_BYTES + OV_PRIM_BYTES);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)f.im.n, 65535, ((size_t)64 << 20) / per_frame}));
    const size_t src_bytes = src_on_device ? 0 : (size_t)f.im.n * slots * elem, cnt_bytes = (src_on_device || !counts) ? 0 : (size_t)f.im.n * sizeof(int32_t);
    uint8_t *recs, *prims, *d_src, *d_counts;
    size_t frames_at;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            recs = cv.take<uint8_t>((size_t)chunk * slots * OV_REC_BYTES);
            prims = cv.take<uint8_t>((size_t)chunk * slots * OV_PRIM_BYTES);
            d_src = cv.take<uint8_t>(src_bytes);
            d_counts = cv.take<uint8_t>(cnt_bytes);
            frames_at = cv.take_at(f.im.on_device ? 0 : f.im.packed_bytes());
        }))
        return rc;
    if (!src_on_device) {
        HIPCHK(h, hipMemcpyAsync(d_src, src, src_bytes, hipMemcpyHostToDevice, s));
        src = d_src;
        if (counts) {
            HIPCHK(h, hipMemcpyAsync(d_counts, counts, cnt_bytes, hipMemcpyHostToDevice, s));
            counts = (const int32_t*)d_counts;
        }
    }
    DevImages dev;
    if (const int rc = stage_input(h, s, f.im, h->scratch, frames_at, &dev)) return rc;
    for (int f0 = 0; f0 < f.im.n; f0 += chunk) {
        const int nf = std::min(chunk, f.im.n - f0);
        build(s, nf, (const uint8_t*)src + (size_t)f0 * slots * elem, counts ? counts + f0 : nullptr, recs, prims);
        HIPCHK(h, hipGetLastError());
        launch_overlay_raster(s, dev.p + (size_t)f0 * dev.frame, nf, f.w, f.im.rows, f.ch, dev.row, dev.frame, recs, prims, slots);
        HIPCHK(h, hipGetLastError());
    }
    if (const int rc = unstage(h, s, f.im, dev)) return rc;
    if (!f.im.on_device || !src_on_device) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // namespace

extern "C" {

int arucohip_draw_markers_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                size_t frame_stride, int frames_on_device, const arucohip_marker_t* markers, int cap, const int32_t* counts,
                                int markers_on_device, const float* K, const float* dist, int ndist, const arucohip_overlay_t* style) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Frames f = make_frames(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device);
    int rc = check_frames(h, f);
    if (rc) return rc;
    if (!markers || !counts || cap < 1) return fail(h, ARUCOHIP_E_INVALID, "draw_markers: NULL markers / counts, or cap below 1");
    if (cap > 65535) return fail(h, ARUCOHIP_E_UNSUPPORTED, "draw_markers: cap exceeds 65535");
    const arucohip_overlay_t def = {ARUCOHIP_DRAW_OUTLINE | ARUCOHIP_DRAW_IDS, 1, {0, 0, 255, 0}};
    const arucohip_overlay_t st = style ? *style : def;
    if (st.line_width < 1 || st.line_width > 7) return fail(h, ARUCOHIP_E_INVALID, "draw_markers: line_width must be 1..7");
    CamModel cam;
    if ((rc = check_camera(h, (st.flags & (ARUCOHIP_DRAW_AXIS | ARUCOHIP_DRAW_CUBE)) != 0, K, dist, ndist, &cam))) return rc;
    const uint32_t color = (uint32_t)st.color[0] | (uint32_t)st.color[1] << 8 | (uint32_t)st.color[2] << 16;
    return draw(h, f, markers, sizeof(arucohip_marker_t), cap, counts, markers_on_device,
                [&](hipStream_t s, int nf, const void* src, const int32_t* cnt, void* recs, void* prims) {
                    launch_overlay_build_markers(s, (const arucohip_marker_t*)src, cnt, nf, cap, cam, st.flags, st.line_width, color, recs, prims);
                });
}

int arucohip_draw_boards_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                               size_t frame_stride, int frames_on_device, const arucohip_board_t* boards, int boards_on_device, float marker_size,
                               const float* K, const float* dist, int ndist, int flags) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Frames f = make_frames(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device);
    int rc = check_frames(h, f);
    if (rc) return rc;
    if (!boards) return fail(h, ARUCOHIP_E_INVALID, "draw_boards: NULL boards");
    if (!(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "draw_boards: marker_size must be positive");
    CamModel cam;
    if ((rc = check_camera(h, true, K, dist, ndist, &cam))) return rc;
    return draw(h, f, boards, sizeof(arucohip_board_t), 1, nullptr, boards_on_device,
                [&](hipStream_t s, int nf, const void* src, const int32_t*, void* recs, void* prims) {
                    launch_overlay_build_boards(s, (const arucohip_board_t*)src, nf, cam, flags, marker_size, recs, prims);
                });
}

}  // extern "C"
