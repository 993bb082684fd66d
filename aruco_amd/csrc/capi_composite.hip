// Host side of plane compositing (k_composite.hip): argument checks, staging of host arguments, the launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the arguments both entry points share, as the caller gave them
struct Call {
    Images frames;
    int w, ch;
    const arucohip_texture_t* tex;
    const float *K, *dist;
    int ndist;
    Images tex_images, masks;   // tex_images: empty while tex is NULL; masks.p NULL: none
    // nothing of the call lives on the host, so nothing has to be waited for
    bool resident() const { return frames.on_device && tex->on_device && (!masks.p || masks.on_device); }
};
Call make_call(uint8_t* frames, int n, int w, int h, int ch, size_t row, size_t frame, int frames_on_device, const arucohip_texture_t* tex, const float* K,
               const float* dist, int ndist, const uint8_t* masks, int masks_on_device) {
    Call c = {images(frames, n, h, (size_t)w * ch, row, frame, frames_on_device), w, ch, tex, K, dist, ndist, {},
              images(masks, n, h, (size_t)w, (size_t)w, (size_t)w * h, masks_on_device)};
    if (tex)   // tex->frame_stride 0: one texture for every frame
        c.tex_images = images(tex->data, tex->frame_stride ? n : 1, tex->height, (size_t)tex->width * tex->channels, tex->row_stride, tex->frame_stride,
                              tex->on_device);
    return c;
}

int check_call(arucohip_handle* h, const Call& c, bool need_K) {
    if (!c.frames.p) return fail(h, ARUCOHIP_E_INVALID, "composite: frames is NULL");
    if (!c.tex) return fail(h, ARUCOHIP_E_INVALID, "composite: tex (the texture) is NULL");
    if (!c.tex->data) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->data is NULL");
    if (c.frames.n < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: nframes is below 1");
    if (c.w < 1 || c.frames.rows < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: width / height is below 1");
    if (c.w > 16383 || c.frames.rows > 16383) return fail(h, ARUCOHIP_E_INVALID, "composite: width / height is above 16383");
    if (c.ch != 1 && c.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "composite: channels must be 1 or 3");
    if (c.tex->channels != c.ch && c.tex->channels != c.ch + 1)
        return fail(h, ARUCOHIP_E_INVALID, "composite: tex->channels must be channels, or channels + 1 with alpha");
    if (c.tex->opacity < 0 || c.tex->opacity > 255) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->opacity is outside 0..255");
    if (c.tex->width < 1 || c.tex->height < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->width / tex->height is below 1");
    if (c.tex->width > 16383 || c.tex->height > 16383) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->width / tex->height is above 16383");
    if (const int rc = check_plane_camera(h, "composite", need_K, c.K, c.dist, c.ndist)) return rc;
    if (const int rc = check_strides(h, "composite", "", c.frames)) return rc;
    if (const int rc = check_strides(h, "composite", "tex->", c.tex_images)) return rc;
    if (const int rc = check_disjoint(h, "composite", "the texture", c.tex_images, "the frames", c.frames)) return rc;
    return c.masks.p ? check_disjoint(h, "composite", "masks", c.masks, "the frames", c.frames) : ARUCOHIP_OK;
}

// The one layout of a call in the handle's arena: the plane maps it uploads or computes (n_maps frames; 0: the caller's are on the
// device) and the staged host frames, textures and masks, tightly packed.
struct Scratch {
    PlaneMaps m;
    size_t frames_at, tex_at, masks_at;
};
int carve(arucohip_handle* h, const Call& c, int n_maps, Scratch* sc) {
    return carve_scratch(h, h, [&](Carver& cv) {
        carve_plane_maps(cv, n_maps, &sc->m);
        sc->frames_at = cv.take_at(c.frames.on_device ? 0 : c.frames.packed_bytes());
        sc->tex_at = cv.take_at(c.tex->on_device ? 0 : c.tex_images.packed_bytes());
        sc->masks_at = cv.take_at(c.masks.p && !c.masks.on_device ? c.masks.packed_bytes() : 0);
    });
}

// The painting of a checked call with device maps: host frames, textures and masks go up and host frames come back. Queues only; the
// caller synchronises.
int paint(arucohip_handle* h, const Call& c, const Scratch& sc, const double* maps, const int32_t* valid) {
    const arucohip_texture_t& t = *c.tex;
    DevImages frames, tex, masks = {nullptr, 0, 0};
    if (const int rc = stage_input(h, h->stream, c.frames, h->scratch, sc.frames_at, &frames)) return rc;
    if (const int rc = stage_input(h, h->stream, c.tex_images, h->scratch, sc.tex_at, &tex)) return rc;
    if (c.masks.p)
        if (const int rc = stage_input(h, h->stream, c.masks, h->scratch, sc.masks_at, &masks)) return rc;
    PlaneComposite a;
    std::memset(&a, 0, sizeof(a));
    a.frames = frames.p, a.row_stride = frames.row, a.frame_stride = frames.frame;
    a.tex = tex.p, a.tex_row_stride = tex.row, a.tex_frame_stride = t.frame_stride ? tex.frame : 0;
    a.masks = masks.p;
    a.width = c.w, a.height = c.frames.rows, a.tex_width = t.width, a.tex_height = t.height, a.opacity = t.opacity;
    a.maps = maps, a.valid = valid;
    a.K[0] = a.K[4] = a.K[8] = 1.f;   // no camera: the ray of pixel (u, v) is (u, v)
    for (int i = 0; c.K && i < 9; i++) a.K[i] = c.K[i];
    for (int i = 0; i < c.ndist; i++) a.k[i] = (double)c.dist[i];
    launch_plane_composite(h->stream, a, c.ch, t.channels == c.ch + 1, c.ndist > 0, c.frames.n);
    HIPCHK(h, hipGetLastError());
    return unstage(h, h->stream, c.frames, frames);
}

}  // namespace

extern "C" {

int arucohip_composite_plane_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                   size_t frame_stride, int frames_on_device, const arucohip_texture_t* tex, const double* maps,
                                   const int32_t* valid, int maps_on_device, const float* K, const float* dist, int ndist, const uint8_t* masks,
                                   int masks_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = make_call(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, tex, K, dist, ndist, masks, masks_on_device);
    if (!maps) return fail(h, ARUCOHIP_E_INVALID, "composite: maps is NULL");
    if (const int rc = check_call(h, c, false)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    Scratch sc;
    if (const int rc = carve(h, c, maps_on_device ? 0 : nframes, &sc)) return rc;
    if (const int rc = stage_plane_maps(h, sc.m, nframes, maps_on_device, &maps, &valid)) return rc;
    if (const int rc = paint(h, c, sc, maps, valid)) return rc;
    if (!c.resident() || !maps_on_device) HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_board_composite_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                   size_t frame_stride, int frames_on_device, const arucohip_board_t* boards, int boards_on_device,
                                   const float* K, const float* dist, int ndist, const arucohip_rectify_t* win, const arucohip_texture_t* tex,
                                   const uint8_t* masks, int masks_on_device, int32_t* status, double* maps_out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!boards) return fail(h, ARUCOHIP_E_INVALID, "composite: boards is NULL");
    if (!win) return fail(h, ARUCOHIP_E_INVALID, "composite: win (the window) is NULL");
    const Call c = make_call(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, tex, K, dist, ndist, masks, masks_on_device);
    if (const int rc = check_call(h, c, true)) return rc;
    if (win->out_width != tex->width || win->out_height != tex->height)
        return fail(h, ARUCOHIP_E_INVALID, "composite: the window's out_width / out_height differ from the texture's size");
    if (!window_spans_plane(*win)) return fail(h, ARUCOHIP_E_INVALID, "composite: the window's u and v steps are parallel, zero or not finite");
    HIPCHK(h, hipSetDevice(h->device));
    Scratch sc;
    if (const int rc = carve(h, c, nframes, &sc)) return rc;
    if (const int rc = plane_maps_of_boards(h, sc.m, launch_plane_inverse_maps, boards, boards_on_device, nframes, *win)) return rc;
    if (const int rc = paint(h, c, sc, sc.m.maps, sc.m.valid)) return rc;
    if (const int rc = read_plane_maps(h, sc.m, nframes, status, maps_out)) return rc;
    if (!c.resident() || !boards_on_device || status || maps_out) HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

}  // extern "C"
