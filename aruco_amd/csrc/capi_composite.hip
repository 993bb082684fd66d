// Host side of plane compositing (k_composite.hip): argument checks, staging of host arguments, the launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the arguments both entry points share, as the caller gave them
struct Call {
    uint8_t* frames;
    int n, w, h, ch;
    size_t row, frame;
    int frames_on_device;
    const arucohip_texture_t* tex;
    const float *K, *dist;
    int ndist;
    const uint8_t* masks;
    int masks_on_device;
    size_t row_bytes() const { return (size_t)w * ch; }
    size_t extent() const { return (size_t)(n - 1) * frame + (size_t)(h - 1) * row + row_bytes(); }
    int textures() const { return tex->frame_stride ? n : 1; }
    size_t tex_row_bytes() const { return (size_t)tex->width * tex->channels; }
    size_t tex_extent() const { return (size_t)(textures() - 1) * tex->frame_stride + (size_t)(tex->height - 1) * tex->row_stride + tex_row_bytes(); }
    size_t mask_bytes() const { return (size_t)n * h * w; }
    // nothing of the call lives on the host, so nothing has to be waited for
    bool resident() const { return frames_on_device && tex->on_device && (!masks || masks_on_device); }
};

int check_call(arucohip_handle* h, const Call& c, bool need_K) {
    if (!c.frames) return fail(h, ARUCOHIP_E_INVALID, "composite: frames is NULL");
    if (!c.tex) return fail(h, ARUCOHIP_E_INVALID, "composite: tex (the texture) is NULL");
    if (!c.tex->data) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->data is NULL");
    if (c.n < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: nframes is below 1");
    if (c.w < 1 || c.h < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: width / height is below 1");
    if (c.w > 16383 || c.h > 16383) return fail(h, ARUCOHIP_E_INVALID, "composite: width / height is above 16383");
    if (c.ch != 1 && c.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "composite: channels must be 1 or 3");
    if (c.tex->channels != c.ch && c.tex->channels != c.ch + 1)
        return fail(h, ARUCOHIP_E_INVALID, "composite: tex->channels must be channels, or channels + 1 with alpha");
    if (c.tex->opacity < 0 || c.tex->opacity > 255) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->opacity is outside 0..255");
    if (c.tex->width < 1 || c.tex->height < 1) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->width / tex->height is below 1");
    if (c.tex->width > 16383 || c.tex->height > 16383) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->width / tex->height is above 16383");
    if (need_K && !c.K) return fail(h, ARUCOHIP_E_INVALID, "composite: K is NULL (the board call needs the camera)");
    if (!(c.ndist == 0 || c.ndist == 4 || c.ndist == 5 || c.ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "composite: ndist must be 0, 4, 5 or 8");
    if (c.ndist > 0 && !c.dist) return fail(h, ARUCOHIP_E_INVALID, "composite: dist is NULL with ndist > 0");
    if (c.ndist > 0 && !c.K) return fail(h, ARUCOHIP_E_INVALID, "composite: dist without K");
    if (c.row < c.row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "composite: row_stride is smaller than width * channels");
    if (c.n > 1 && c.frame < (size_t)(c.h - 1) * c.row + c.row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "composite: frame_stride is smaller than a frame");
    if (c.tex->row_stride < c.tex_row_bytes()) return fail(h, ARUCOHIP_E_INVALID, "composite: tex->row_stride is smaller than tex->width * tex->channels");
    if (c.textures() > 1 && c.tex->frame_stride < (size_t)(c.tex->height - 1) * c.tex->row_stride + c.tex_row_bytes())
        return fail(h, ARUCOHIP_E_INVALID, "composite: tex->frame_stride is neither 0 nor a texture");
    // host and device addresses share one space, so one comparison serves every combination
    const uintptr_t f0 = (uintptr_t)c.frames, t0 = (uintptr_t)c.tex->data, m0 = (uintptr_t)c.masks;
    if (t0 < f0 + c.extent() && f0 < t0 + c.tex_extent()) return fail(h, ARUCOHIP_E_INVALID, "composite: the texture overlaps the frames");
    if (c.masks && m0 < f0 + c.extent() && f0 < m0 + c.mask_bytes()) return fail(h, ARUCOHIP_E_INVALID, "composite: masks overlaps the frames");
    return ARUCOHIP_OK;
}

// one call's scratch in d_composite
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
    HIPCHK(h, h->d_composite.reserve(scratch_layout(nullptr, n, s)));
    scratch_layout(h->d_composite, n, s);
    return ARUCOHIP_OK;
}

// what of a call's frames, textures and masks lives on the host, staged tightly packed in d_composite_frames
struct Staged {
    uint8_t *frames, *tex, *masks;
};
size_t staged_layout(uint8_t* base, const Call& c, Staged* s) {
    Carver cv{base};
    s->frames = cv.take<uint8_t>(c.frames_on_device ? 0 : (size_t)c.n * c.h * c.row_bytes());
    s->tex = cv.take<uint8_t>(c.tex->on_device ? 0 : (size_t)c.textures() * c.tex->height * c.tex_row_bytes());
    s->masks = cv.take<uint8_t>(!c.masks || c.masks_on_device ? 0 : c.mask_bytes());
    return cv.at;
}

// The painting of a checked call with device maps: host frames, textures and masks go up, host frames come back. Queues only; the
// caller synchronises.
int paint(arucohip_handle* h, const Call& c, const double* maps, const int32_t* valid) {
    Staged st;
    HIPCHK(h, h->d_composite_frames.reserve(staged_layout(nullptr, c, &st)));
    staged_layout(h->d_composite_frames, c, &st);
    const arucohip_texture_t& t = *c.tex;
    PlaneComposite a;
    std::memset(&a, 0, sizeof(a));
    a.frames = c.frames, a.row_stride = c.row, a.frame_stride = c.frame;
    if (!c.frames_on_device) {
        if (const int rc = copy_rows(h, c.frames, c.row, c.frame, c.row_bytes(), c.h, c.n, st.frames, true)) return rc;
        a.frames = st.frames, a.row_stride = c.row_bytes(), a.frame_stride = (size_t)c.h * c.row_bytes();
    }
    a.tex = t.data, a.tex_row_stride = t.row_stride, a.tex_frame_stride = t.frame_stride;
    if (!t.on_device) {
        if (const int rc = copy_rows(h, const_cast<uint8_t*>(t.data), t.row_stride, t.frame_stride, c.tex_row_bytes(), t.height, c.textures(), st.tex, true))
            return rc;
        a.tex = st.tex, a.tex_row_stride = c.tex_row_bytes(), a.tex_frame_stride = t.frame_stride ? (size_t)t.height * c.tex_row_bytes() : 0;
    }
    a.masks = c.masks;
    if (c.masks && !c.masks_on_device) {
        HIPCHK(h, hipMemcpyAsync(st.masks, c.masks, c.mask_bytes(), hipMemcpyHostToDevice, h->stream));
        a.masks = st.masks;
    }
    a.width = c.w, a.height = c.h, a.tex_width = t.width, a.tex_height = t.height, a.opacity = t.opacity;
    a.maps = maps, a.valid = valid;
    a.K[0] = a.K[4] = a.K[8] = 1.f;   // no camera: the ray of pixel (u, v) is (u, v)
    for (int i = 0; c.K && i < 9; i++) a.K[i] = c.K[i];
    for (int i = 0; i < c.ndist; i++) a.k[i] = (double)c.dist[i];
    launch_plane_composite(h->stream, a, c.ch, t.channels == c.ch + 1, c.ndist > 0, c.n);
    HIPCHK(h, hipGetLastError());
    if (!c.frames_on_device) return copy_rows(h, c.frames, c.row, c.frame, c.row_bytes(), c.h, c.n, a.frames, false);
    return ARUCOHIP_OK;
}

}  // namespace

extern "C" {

int arucohip_composite_plane_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                   size_t frame_stride, int frames_on_device, const arucohip_texture_t* tex, const double* maps,
                                   const int32_t* valid, int maps_on_device, const float* K, const float* dist, int ndist, const uint8_t* masks,
                                   int masks_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = {frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, tex, K, dist, ndist, masks, masks_on_device};
    if (!maps) return fail(h, ARUCOHIP_E_INVALID, "composite: maps is NULL");
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
    if (const int rc = paint(h, c, maps, valid)) return rc;
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
    const Call c = {frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, tex, K, dist, ndist, masks, masks_on_device};
    if (const int rc = check_call(h, c, true)) return rc;
    if (win->out_width != tex->width || win->out_height != tex->height)
        return fail(h, ARUCOHIP_E_INVALID, "composite: the window's out_width / out_height differ from the texture's size");
    if (!window_spans_plane(*win)) return fail(h, ARUCOHIP_E_INVALID, "composite: the window's u and v steps are parallel, zero or not finite");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    Scratch sc;
    if (const int rc = reserve_scratch(h, nframes, &sc)) return rc;
    if (!boards_on_device) {
        HIPCHK(h, hipMemcpyAsync(sc.boards, boards, (size_t)nframes * sizeof(arucohip_board_t), hipMemcpyHostToDevice, s));
        boards = sc.boards;
    }
    launch_plane_inverse_maps(s, boards, nframes, *win, sc.maps, sc.valid);
    HIPCHK(h, hipGetLastError());
    if (const int rc = paint(h, c, sc.maps, sc.valid)) return rc;
    if (status) HIPCHK(h, hipMemcpyAsync(status, sc.valid, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (maps_out) HIPCHK(h, hipMemcpyAsync(maps_out, sc.maps, (size_t)nframes * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (!c.resident() || !boards_on_device || status || maps_out) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
