// Host side of the two planar pose solutions per marker (k_planar.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "handle.h"

// the argument checks of arucohip_calculate_extrinsics and the camera record the kernels take
static int planar_cam(arucohip_handle* h, const float* K, const float* dist, int ndist, float marker_size, int y_perp, CamModel* cam) {
    if (!K) return fail(h, ARUCOHIP_E_INVALID, "planar_poses: K is required");
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0, 4, 5 or 8");
    if (ndist > 0 && !dist) return fail(h, ARUCOHIP_E_INVALID, "planar_poses: dist is NULL with ndist > 0");
    if (!(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "marker size must be positive");
    fill_cam(cam, K, dist, ndist, marker_size, y_perp);
    return ARUCOHIP_OK;
}

extern "C" {

int arucohip_planar_poses(arucohip_handle* h, const arucohip_marker_t* markers, int n, int on_device, const float* K, const float* dist, int ndist,
                          float marker_size, int refine, int y_perp, arucohip_planar_poses_t* out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (n < 0 || (n > 0 && (!markers || !out))) return fail(h, ARUCOHIP_E_INVALID, "planar_poses: NULL markers / out or a negative count");
    CamModel cam;
    int rc = planar_cam(h, K, dist, ndist, marker_size, y_perp, &cam);
    if (rc) return rc;
    if (n == 0) return ARUCOHIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (on_device) {
        launch_planar_poses(s, markers, n, cam, refine, out);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(s));
        return ARUCOHIP_OK;
    }
    // in the arena: the results, then the markers
    const size_t out_bytes = (size_t)n * sizeof(arucohip_planar_poses_t), in_bytes = (size_t)n * sizeof(arucohip_marker_t);
    arucohip_planar_poses_t* d_out;
    arucohip_marker_t* d_in;
    if ((rc = carve_scratch(h, h, [&](Carver& cv) {
             d_out = cv.take<arucohip_planar_poses_t>((size_t)n);
             d_in = cv.take<arucohip_marker_t>((size_t)n);
         })))
        return rc;
    HIPCHK(h, hipMemcpyAsync(d_in, markers, in_bytes, hipMemcpyHostToDevice, s));
    launch_planar_poses(s, d_in, n, cam, refine, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_planar_poses_batch(arucohip_handle* h, int nframes, const float* K, const float* dist, int ndist, float marker_size, int refine,
                                int y_perp, arucohip_planar_poses_t* out, int cap, int out_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!out || cap < 1) return fail(h, ARUCOHIP_E_INVALID, "planar_poses_batch: NULL out or no capacity");
    CamModel cam;
    int rc = planar_cam(h, K, dist, ndist, marker_size, y_perp, &cam);
    if (rc) return rc;
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    // the counts first: a frame that does not fit fails the call before anything is written
    std::vector<int32_t> cnt((size_t)nframes);
    for (const Span& s : b) HIPCHK(h, hipMemcpyAsync(cnt.data() + s.first, s.w->buf.nmarkers, (size_t)s.count * sizeof(int32_t), hipMemcpyDeviceToHost, s.w->stream));
    for (const Span& s : b) HIPCHK(h, hipStreamSynchronize(s.w->stream));
    for (const Span& s : b)
        for (int f = s.first; f < s.first + s.count; f++) {
            cnt[f] = std::max(std::min(cnt[f], s.w->buf.cap_markers), 0);   // what the batch returned: clamped, 0 for a frame it gave up
            if (cnt[f] > cap) return fail(h, ARUCOHIP_E_CAPACITY, "planar_poses_batch: a frame holds more than cap markers");
        }
    // every worker solves the markers of the frames it detected, on its own stream; host results go through the worker's arena
    std::vector<arucohip_planar_poses_t> stage;
    if (!out_on_device) stage.resize((size_t)nframes * cap);
    rc = on_workers(h, b, [&](const Span& s) -> int {
        arucohip_handle* w = s.w;
        const int list_frames = h->last.span[b.index(s)].count;   // the worker's list holds the markers of every frame it detected
        if (out_on_device) {
            launch_planar_poses_list(w->stream, list_frames, s.count, s.first, w->buf, cam, refine, out, cap);
        } else {
            const size_t bytes = (size_t)s.count * cap * sizeof(arucohip_planar_poses_t);
            arucohip_planar_poses_t* d_out;
            if (const int e = carve_scratch(w, h, [&](Carver& cv) {
                    d_out = cv.take<arucohip_planar_poses_t>((size_t)s.count * cap);
                }))
                return e;
            launch_planar_poses_list(w->stream, list_frames, s.count, 0, w->buf, cam, refine, d_out, cap);
            HIPCHK(h, hipMemcpyAsync(stage.data() + (size_t)s.first * cap, d_out, bytes, hipMemcpyDeviceToHost, w->stream));
        }
        return ARUCOHIP_OK;
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(b.span[0].w->stream));
    if (!out_on_device)
        for (int f = 0; f < nframes; f++)
            std::memcpy(out + (size_t)f * cap, stage.data() + (size_t)f * cap, (size_t)cnt[f] * sizeof(arucohip_planar_poses_t));
    return ARUCOHIP_OK;
}

}  // extern "C"
