// Host side of mesh rendering (k_render.hip): argument checks, staging of host arguments, the chunked instance + build + raster launches.
#include <hip/hip_runtime.h>

#include <cstring>

#include "handle.h"

namespace {

// the arguments both entry points share, as the caller gave them
struct Call {
    Images frames;
    int w, ch;
    const float *K, *dist;
    int ndist;
    const arucohip_mesh_t* mesh;
    arucohip_render_t style;
    Images masks;   // masks.p NULL: none
};
Call make_call(uint8_t* frames, int n, int w, int h, int ch, size_t row, size_t frame, int frames_on_device, const float* K, const float* dist, int ndist,
               const arucohip_mesh_t* mesh, const arucohip_render_t* style, const uint8_t* masks, int masks_on_device) {
    Call c = {images(frames, n, h, (size_t)w * ch, row, frame, frames_on_device), w, ch, K, dist, ndist, mesh, {},
              images(masks, n, h, (size_t)w, (size_t)w, (size_t)w * h, masks_on_device)};
    if (style)
        c.style = *style;
    else
        arucohip_default_render(&c.style);
    return c;
}

// a flat array of the caller's as an image batch of one row, for the overlap test
Images flat(const void* p, size_t bytes, int on_device) { return images(p, 1, 1, bytes, bytes, bytes, on_device); }

// every refusal, before anything runs; *rs: the style as the kernels take it
int check_call(arucohip_handle* h, const Call& c, RdStyle* rs) {
    if (!c.frames.p) return fail(h, ARUCOHIP_E_INVALID, "render: frames is NULL");
    if (!c.mesh) return fail(h, ARUCOHIP_E_INVALID, "render: mesh is NULL");
    const arucohip_mesh_t& m = *c.mesh;
    if (!m.vertices || !m.triangles) return fail(h, ARUCOHIP_E_INVALID, "render: mesh->vertices / mesh->triangles is NULL");
    if (!c.K) return fail(h, ARUCOHIP_E_INVALID, "render: K is NULL (rendering needs the camera)");
    if (c.frames.n < 1) return fail(h, ARUCOHIP_E_INVALID, "render: nframes is below 1");
    if (c.w < 1 || c.frames.rows < 1) return fail(h, ARUCOHIP_E_INVALID, "render: width / height is below 1");
    if (c.ch != 1 && c.ch != 3) return fail(h, ARUCOHIP_E_INVALID, "render: channels must be 1 or 3");
    if (m.nverts < 1 || m.nverts > 65536) return fail(h, ARUCOHIP_E_INVALID, "render: mesh->nverts is outside 1..65536");
    if (m.ntris < 1 || m.ntris > 16384) return fail(h, ARUCOHIP_E_INVALID, "render: mesh->ntris is outside 1..16384");
    const arucohip_render_t& s = c.style;
    if (s.opacity < 0 || s.opacity > 255) return fail(h, ARUCOHIP_E_INVALID, "render: style->opacity is outside 0..255");
    if (s.ambient < 0 || s.ambient > 255) return fail(h, ARUCOHIP_E_INVALID, "render: style->ambient is outside 0..255");
    if (!(s.scale > 0) || !std::isfinite(s.scale)) return fail(h, ARUCOHIP_E_INVALID, "render: style->scale must be positive and finite");
    const double lx = s.light[0], ly = s.light[1], lz = s.light[2], len = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!(len > 0) || !std::isfinite(len)) return fail(h, ARUCOHIP_E_INVALID, "render: style->light is zero or not finite");
    if (!(c.ndist == 0 || c.ndist == 4 || c.ndist == 5 || c.ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "render: ndist must be 0, 4, 5 or 8");
    if (c.ndist > 0 && !c.dist) return fail(h, ARUCOHIP_E_INVALID, "render: dist is NULL with ndist > 0");
    if (const int rc = check_strides(h, "render", "", c.frames)) return rc;
    if (const int rc = check_disjoint(h, "render", "mesh->vertices", flat(m.vertices, (size_t)m.nverts * 12, m.on_device), "the frames", c.frames)) return rc;
    if (const int rc = check_disjoint(h, "render", "mesh->triangles", flat(m.triangles, (size_t)m.ntris * 12, m.on_device), "the frames", c.frames)) return rc;
    if (m.colors)
        if (const int rc = check_disjoint(h, "render", "mesh->colors", flat(m.colors, (size_t)m.ntris * 3, m.on_device), "the frames", c.frames)) return rc;
    if (c.masks.p)
        if (const int rc = check_disjoint(h, "render", "masks", c.masks, "the frames", c.frames)) return rc;
    if (!m.on_device)
        for (size_t i = 0; i < (size_t)m.ntris * 3; i++)
            if (m.triangles[i] < 0 || m.triangles[i] >= m.nverts) return fail(h, ARUCOHIP_E_INVALID, "render: mesh->triangles holds an index outside 0..nverts-1");
    if (c.w > h->lim.max_width || c.frames.rows > h->lim.max_height) return fail(h, ARUCOHIP_E_UNSUPPORTED, "render: width / height exceed the handle's limits");
    rs->flags = s.flags, rs->opacity = s.opacity, rs->ambient = s.ambient;
    rs->color = (uint32_t)s.color[0] | (uint32_t)s.color[1] << 8 | (uint32_t)s.color[2] << 16;
    rs->light[0] = lx / len, rs->light[1] = ly / len, rs->light[2] = lz / len;
    rs->scale = (double)s.scale;
    return ARUCOHIP_OK;
}

struct Scratch {
    uint8_t *insts, *verts, *tris, *src;
    int32_t* counts;
    float* vertices;
    int32_t* triangles;
    uint8_t* colors;
    size_t frames_at, masks_at;   // staged host frames and masks
};

// The common part: `slots` instance slots per frame (cap for markers, 1 for boards). src / counts: device pointers, or host arrays of
// `elem` bytes per slot that are staged behind the records in the handle's arena, with the host mesh, frames and masks. instances(stream, frames, src, counts, insts) enqueues the front kernel of
// one chunk.
template <typename Instances>
int render(arucohip_handle* h, const Call& c, const RdStyle& rs, const void* src, size_t elem, int slots, const int32_t* counts, int src_on_device,
           Instances instances) {
    const arucohip_mesh_t& m = *c.mesh;
    const int n = c.frames.n;
    // the scratch holds the records of a chunk of frames: at most 64 MiB (and 65535 frames, the grid's z limit), at least one frame
    const size_t per_frame = (size_t)slots * (RD_INST_BYTES + (size_t)m.nverts * RD_VERT_BYTES + (size_t)m.ntris * RD_TRI_BYTES);
    if (per_frame > ((size_t)1 << 30)) return fail(h, ARUCOHIP_E_UNSUPPORTED, "render: cap times the mesh needs more than 1 GiB of scratch for one frame");
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, 65535, ((size_t)64 << 20) / per_frame}));
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const bool stage_masks = c.masks.p && !c.masks.on_device;
    Scratch sc;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            sc.insts = cv.take<uint8_t>((size_t)chunk * slots * RD_INST_BYTES);
            sc.verts = cv.take<uint8_t>((size_t)chunk * slots * m.nverts * RD_VERT_BYTES);
            sc.tris = cv.take<uint8_t>((size_t)chunk * slots * m.ntris * RD_TRI_BYTES);
            sc.src = cv.take<uint8_t>(src_on_device ? 0 : (size_t)n * slots * elem);
            sc.counts = cv.take<int32_t>((src_on_device || !counts) ? 0 : (size_t)n);
            sc.vertices = cv.take<float>(m.on_device ? 0 : (size_t)m.nverts * 3);
            sc.triangles = cv.take<int32_t>(m.on_device ? 0 : (size_t)m.ntris * 3);
            sc.colors = cv.take<uint8_t>((m.on_device || !m.colors) ? 0 : (size_t)m.ntris * 3);
            sc.frames_at = cv.take_at(c.frames.on_device ? 0 : c.frames.packed_bytes());
            sc.masks_at = cv.take_at(stage_masks ? c.masks.packed_bytes() : 0);
        }))
        return rc;
    if (!src_on_device) {
        HIPCHK(h, hipMemcpyAsync(sc.src, src, (size_t)n * slots * elem, hipMemcpyHostToDevice, s));
        src = sc.src;
        if (counts) {
            HIPCHK(h, hipMemcpyAsync(sc.counts, counts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
            counts = sc.counts;
        }
    }
    RdMesh mesh = {m.vertices, m.triangles, m.colors, m.nverts, m.ntris};
    if (!m.on_device) {
        HIPCHK(h, hipMemcpyAsync(sc.vertices, m.vertices, (size_t)m.nverts * 12, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(sc.triangles, m.triangles, (size_t)m.ntris * 12, hipMemcpyHostToDevice, s));
        if (m.colors) HIPCHK(h, hipMemcpyAsync(sc.colors, m.colors, (size_t)m.ntris * 3, hipMemcpyHostToDevice, s));
        mesh.vertices = sc.vertices, mesh.triangles = sc.triangles, mesh.colors = m.colors ? sc.colors : nullptr;
    }
    DevImages dev, mk = {nullptr, 0, 0};
    if (const int rc = stage_input(h, s, c.frames, h->scratch, sc.frames_at, &dev)) return rc;
    if (c.masks.p)
        if (const int rc = stage_input(h, s, c.masks, h->scratch, sc.masks_at, &mk)) return rc;
    CamModel cam;
    fill_cam(&cam, c.K, c.dist, c.ndist, 0.f, 0);
    // with timing (arucohip_enable_timing) the build and the raster of every chunk are bracketed by events and waited for
    hipEvent_t ev[3] = {};
    if (h->timing)
        for (hipEvent_t& e : ev) HIPCHK(h, hipEventCreate(&e));
    int rc = ARUCOHIP_OK;
    for (int f0 = 0; f0 < n && !rc; f0 += chunk) {
        const int nf = std::min(chunk, n - f0);
        auto enqueue = [&]() -> int {
            if (h->timing) HIPCHK(h, hipEventRecord(ev[0], s));
            instances(s, nf, (const uint8_t*)src + (size_t)f0 * slots * elem, counts ? counts + f0 : nullptr, sc.insts);
            HIPCHK(h, hipGetLastError());
            launch_render_build(s, sc.insts, nf * slots, cam, mesh, rs, sc.verts, sc.tris);
            HIPCHK(h, hipGetLastError());
            if (h->timing) HIPCHK(h, hipEventRecord(ev[1], s));
            launch_render_raster(s, dev.p + (size_t)f0 * dev.frame, nf, c.w, c.frames.rows, c.ch, dev.row, dev.frame,
                                 mk.p ? mk.p + (size_t)f0 * mk.frame : nullptr, mk.row, mk.frame, sc.insts, sc.tris, slots, m.ntris, rs);
            HIPCHK(h, hipGetLastError());
            if (h->timing) {
                HIPCHK(h, hipEventRecord(ev[2], s));
                HIPCHK(h, hipEventSynchronize(ev[2]));
                float build = 0, raster = 0;
                HIPCHK(h, hipEventElapsedTime(&build, ev[0], ev[1]));
                HIPCHK(h, hipEventElapsedTime(&raster, ev[1], ev[2]));
                h->render_ms[0] += build, h->render_ms[1] += raster;
            }
            return ARUCOHIP_OK;
        };
        rc = enqueue();
    }
    if (h->timing) {
        h->render_calls++;
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    if (rc) return rc;
    if (const int r = unstage(h, s, c.frames, dev)) return r;
    if (!c.frames.on_device || !src_on_device || !m.on_device || stage_masks) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // namespace

extern "C" {

void arucohip_default_render(arucohip_render_t* r) {
    if (!r) return;
    std::memset(r, 0, sizeof(*r));
    r->flags = ARUCOHIP_RENDER_CULL_BACK, r->opacity = 255, r->ambient = 64, r->scale = 1.f;
    r->light[2] = -1.f;
    r->color[1] = 200;
}

int arucohip_render_markers_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                  size_t frame_stride, int frames_on_device, const arucohip_marker_t* markers, int cap, const int32_t* counts,
                                  int markers_on_device, const float* K, const float* dist, int ndist, const arucohip_mesh_t* mesh,
                                  const arucohip_render_t* style, const uint8_t* masks, int masks_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = make_call(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, K, dist, ndist, mesh, style, masks, masks_on_device);
    if (!markers || !counts) return fail(h, ARUCOHIP_E_INVALID, "render_markers: markers / counts is NULL");
    if (cap < 1) return fail(h, ARUCOHIP_E_INVALID, "render_markers: cap is below 1");
    RdStyle rs;
    if (const int rc = check_call(h, c, &rs)) return rc;
    if (cap > 65535) return fail(h, ARUCOHIP_E_UNSUPPORTED, "render_markers: cap exceeds 65535");
    return render(h, c, rs, markers, sizeof(arucohip_marker_t), cap, counts, markers_on_device,
                  [&](hipStream_t s, int nf, const void* src, const int32_t* cnt, void* insts) {
                      launch_render_instances_markers(s, (const arucohip_marker_t*)src, cnt, nf, cap, rs.scale, insts);
                  });
}

int arucohip_render_boards_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                 size_t frame_stride, int frames_on_device, const arucohip_board_t* boards, int boards_on_device, const float* K,
                                 const float* dist, int ndist, const arucohip_mesh_t* mesh, const arucohip_render_t* style, const uint8_t* masks,
                                 int masks_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const Call c = make_call(frames, nframes, width, height, channels, row_stride, frame_stride, frames_on_device, K, dist, ndist, mesh, style, masks, masks_on_device);
    if (!boards) return fail(h, ARUCOHIP_E_INVALID, "render_boards: boards is NULL");
    RdStyle rs;
    if (const int rc = check_call(h, c, &rs)) return rc;
    return render(h, c, rs, boards, sizeof(arucohip_board_t), 1, nullptr, boards_on_device,
                  [&](hipStream_t s, int nf, const void* src, const int32_t*, void* insts) {
                      launch_render_instances_boards(s, (const arucohip_board_t*)src, nf, rs.scale, insts);
                  });
}

int arucohip_render_times(arucohip_handle* h, float* build_ms, float* raster_ms) {
    if (!h) return 0;
    const int n = h->render_calls;
    if (build_ms) *build_ms = n ? (float)(h->render_ms[0] / n) : 0.f;
    if (raster_ms) *raster_ms = n ? (float)(h->render_ms[1] / n) : 0.f;
    return n;
}

}  // extern "C"
