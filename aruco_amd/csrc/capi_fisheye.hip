// Host side of the fisheye calls (k_fisheye.hip): points, frames and the resident markers of the last batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

// the model, Knew (NULL: K) and max_angle (<= 0: the default) as the kernels take them
static int make_fisheye_cam(arucohip_handle* h, const arucohip_fisheye_t* m, const float* Knew, float max_angle, FisheyeCam* c) {
    if (!m) return fail(h, ARUCOHIP_E_INVALID, "fisheye: no model");
    const double* K = m->K;
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(K[i])) return fail(h, ARUCOHIP_E_INVALID, "fisheye: K is not finite");
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(m->D[i])) return fail(h, ARUCOHIP_E_INVALID, "fisheye: D is not finite");
    if (K[0] == 0 || K[4] == 0) return fail(h, ARUCOHIP_E_INVALID, "fisheye: K holds no focal lengths");
    if (K[1] != 0) return fail(h, ARUCOHIP_E_INVALID, "fisheye: skew is not supported");
    c->fx = K[0], c->fy = K[4], c->cx = K[2], c->cy = K[5];
    for (int i = 0; i < 4; i++) c->k[i] = m->D[i];
    for (int i = 0; i < 9; i++) c->Knew[i] = Knew ? (double)Knew[i] : (i == 1 ? 0.0 : K[i]);
    const double* S = c->Knew;
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (!std::isfinite(d) || d == 0) return fail(h, ARUCOHIP_E_INVALID, "fisheye: Knew is singular");
    d = 1. / d;
    double* ir = c->iKnew;
    ir[0] = (S[4] * S[8] - S[5] * S[7]) * d, ir[1] = (S[2] * S[7] - S[1] * S[8]) * d, ir[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    ir[3] = (S[5] * S[6] - S[3] * S[8]) * d, ir[4] = (S[0] * S[8] - S[2] * S[6]) * d, ir[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    ir[6] = (S[3] * S[7] - S[4] * S[6]) * d, ir[7] = (S[1] * S[6] - S[0] * S[7]) * d, ir[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    c->max_angle = max_angle > 0 ? (double)max_angle : FISHEYE_DEFAULT_MAX_ANGLE;
    if (!(c->max_angle < 1.5707963267948966)) return fail(h, ARUCOHIP_E_INVALID, "fisheye: max_angle must be below pi / 2");
    return ARUCOHIP_OK;
}

static int fisheye_points(arucohip_handle* h, const arucohip_fisheye_t* model, const float* Knew, float max_angle, const float* src, int n, int on_device,
                          float* dst, uint8_t* valid, int undistort) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (n < 0 || (n > 0 && (!src || !dst || (undistort && !valid)))) return fail(h, ARUCOHIP_E_INVALID, "fisheye points: src, dst and valid are required");
    FisheyeCam cam;
    int rc = make_fisheye_cam(h, model, Knew, max_angle, &cam);
    if (rc || n == 0) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (on_device) {
        launch_fisheye_points(s, cam, src, n, undistort, dst, valid);
        HIPCHK(h, hipGetLastError());
        return ARUCOHIP_OK;
    }
    const size_t pts = (size_t)n * 2 * sizeof(float);
    float *d_src, *d_dst;
    uint8_t* d_valid;
    if ((rc = carve_scratch(h, h, [&](Carver& cv) {
             d_src = cv.take<float>((size_t)n * 2);
             d_dst = cv.take<float>((size_t)n * 2);
             d_valid = cv.take<uint8_t>((size_t)n);
         })))
        return rc;
    HIPCHK(h, hipMemcpyAsync(d_src, src, pts, hipMemcpyHostToDevice, s));
    launch_fisheye_points(s, cam, d_src, n, undistort, d_dst, d_valid);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(dst, d_dst, pts, hipMemcpyDeviceToHost, s));
    if (undistort) HIPCHK(h, hipMemcpyAsync(valid, d_valid, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

// the start state of a fisheye run from (model, flags)
int calib_fisheye_state(arucohip_handle* h, int W, int H, int flags, const arucohip_fisheye_t* model, CalibState* stp) {
    CalibState& st = *stp;
    std::memset(&st, 0, sizeof(st));
    st.model = CALIB_MODEL_FISHEYE;
    st.flags = (flags & ARUCOHIP_FISHEYE_FIX_ASPECT_RATIO) ? ARUCOHIP_CALIB_FIX_ASPECT_RATIO : 0;   // the one flag the kernels read
    const double* K = model->K;
    st.aspect = (K[0] > 0 && K[4] > 0) ? K[0] / K[4] : 1.0;
    if (flags & ARUCOHIP_FISHEYE_USE_INTRINSIC_GUESS) {
        if (!(K[0] > 0 && K[4] > 0)) return fail(h, ARUCOHIP_E_INVALID, "USE_INTRINSIC_GUESS needs positive focal lengths");
        if (K[1] != 0) return fail(h, ARUCOHIP_E_INVALID, "fisheye: skew is not supported");
        st.intr[0] = K[0], st.intr[1] = K[4], st.intr[2] = K[2], st.intr[3] = K[5];
        for (int i = 0; i < 4; i++) st.intr[4 + i] = model->D[i];
        for (int i = 0; i < 8; i++)
            if (!std::isfinite(st.intr[i])) return fail(h, ARUCOHIP_E_INVALID, "fisheye: the start model is not finite");
    } else {
        st.intr[0] = st.intr[1] = std::max(W, H) / 3.14159265358979323846;
        st.intr[2] = (W - 1) * 0.5, st.intr[3] = (H - 1) * 0.5;
    }
    if (flags & ARUCOHIP_FISHEYE_FIX_ASPECT_RATIO) st.intr[0] = st.aspect * st.intr[1];
    int mask = 0xFF;   // the ninth column is zero: never free
    if (flags & ARUCOHIP_FISHEYE_FIX_ASPECT_RATIO) mask &= ~1;
    if (flags & ARUCOHIP_FISHEYE_FIX_PRINCIPAL_POINT) mask &= ~(4 | 8);
    if (flags & ARUCOHIP_FISHEYE_FIX_K1) mask &= ~16;
    if (flags & ARUCOHIP_FISHEYE_FIX_K2) mask &= ~32;
    if (flags & ARUCOHIP_FISHEYE_FIX_K3) mask &= ~64;
    if (flags & ARUCOHIP_FISHEYE_FIX_K4) mask &= ~128;
    st.free_mask = mask;
    return ARUCOHIP_OK;
}

// the fisheye run of the calibration solver (k_calib.hip with CALIB_MODEL_FISHEYE): start state from (model, flags), results back
static int calib_fisheye(arucohip_handle* h, const CalibViews& v, int W, int H, int flags, arucohip_fisheye_t* model, double* rvecs, double* tvecs,
                         double* per_view_rms, double* rms) {
    CalibState st;
    int rc = calib_fisheye_state(h, W, H, flags, model, &st);
    if (rc) return rc;
    double in[9];
    rc = calib_solve(h, v, st, false, in, rvecs, tvecs, per_view_rms, rms);
    if (rc) return rc;
    const double Ko[9] = {in[0], 0, in[2], 0, in[1], in[3], 0, 0, 1};
    for (int i = 0; i < 9; i++) model->K[i] = Ko[i];
    for (int i = 0; i < 4; i++) model->D[i] = in[4 + i];
    return ARUCOHIP_OK;
}

extern "C" {

int arucohip_fisheye_calibrate(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, int W, int H,
                               int flags, arucohip_fisheye_t* model, double* rvecs, double* tvecs, double* per_view_rms, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!obj || !img || !npoints || !model || nviews < 1 || W <= 0 || H <= 0)
        return fail(h, ARUCOHIP_E_INVALID, "fisheye_calibrate: NULL argument, no views or an empty image size");
    CalibViews v;
    const int rc = calib_views_of_points(h, obj, img, npoints, nviews, on_device, &v);
    if (rc) return rc;
    return calib_fisheye(h, v, W, H, flags, model, rvecs, tvecs, per_view_rms, rms);
}

int arucohip_fisheye_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                           float marker_size, int min_markers, int W, int H, int flags, arucohip_fisheye_t* model, int32_t* used,
                                           double* rvecs, double* tvecs, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!model || W <= 0 || H <= 0) return fail(h, ARUCOHIP_E_INVALID, "fisheye_calibrate_board_batch: NULL model or an empty image size");
    if (h->last.ideal) return fail(h, ARUCOHIP_E_INVALID, "fisheye_calibrate_board_batch: the last batch holds ideal corners, not the lens's pixels");
    CalibViews v;
    arucohip_handle* o = nullptr;
    int rc = calib_views_of_batch(h, nframes, BoardDef{ids, obj, nboard, info_type, marker_size, -1.f}, min_markers, used, &o, &v);
    if (rc) return rc;
    rc = calib_fisheye(o, v, W, H, flags, model, rvecs, tvecs, nullptr, rms);
    if (rc && o != h) h->err = o->err;
    return rc;
}

int arucohip_fisheye_undistort_points(arucohip_handle* h, const arucohip_fisheye_t* model, const float* Knew, float max_angle, const float* src, int n,
                                      int on_device, float* dst, uint8_t* valid) {
    return fisheye_points(h, model, Knew, max_angle, src, n, on_device, dst, valid, 1);
}

int arucohip_fisheye_distort_points(arucohip_handle* h, const arucohip_fisheye_t* model, const float* Knew, const float* src, int n, int on_device,
                                    float* dst) {
    return fisheye_points(h, model, Knew, 0.f, src, n, on_device, dst, nullptr, 0);
}

int arucohip_fisheye_undistort(arucohip_handle* h, const uint8_t* src, int nframes, int W, int H, size_t row_stride, size_t frame_stride, int channels,
                               int src_on_device, const arucohip_fisheye_t* model, const float* Knew, float max_angle, uint8_t* dst, int dst_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!src || !dst || (channels != 1 && channels != 3)) return fail(h, ARUCOHIP_E_INVALID, "fisheye_undistort: src, dst and 1 or 3 channels are required");
    if (nframes < 1 || nframes > h->lim.max_batch) return fail(h, ARUCOHIP_E_INVALID, "nframes outside 1..max_batch");
    if (W < 1 || H < 1 || W > h->lim.max_width || H > h->lim.max_height) return fail(h, ARUCOHIP_E_INVALID, "frame wider or taller than the handle was created for");
    if (row_stride < (size_t)W * channels) return fail(h, ARUCOHIP_E_INVALID, "row_stride < width * channels");
    if (nframes > 1 && frame_stride < (size_t)H * row_stride) return fail(h, ARUCOHIP_E_INVALID, "frame_stride < height * row_stride");
    FisheyeCam cam;
    int rc = make_fisheye_cam(h, model, Knew, max_angle, &cam);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // the map of this camera, in the fisheye slot: recomputed only when the size, the model, Knew or max_angle change
    double key[18];
    key[0] = cam.fx, key[1] = cam.fy, key[2] = cam.cx, key[3] = cam.cy;
    for (int i = 0; i < 4; i++) key[4 + i] = cam.k[i];
    for (int i = 0; i < 9; i++) key[8 + i] = cam.Knew[i];
    key[17] = cam.max_angle;
    if (!(h->fmap_w == W && h->fmap_h == H && std::memcmp(h->fmap_key, key, sizeof(key)) == 0)) {
        const size_t px = (size_t)W * H;
        h->fmap_w = 0;   // no valid map until this one is written
        HIPCHK(h, h->d_fmap_xy.reserve(px * sizeof(short2)));
        HIPCHK(h, h->d_fmap_f.reserve(px * sizeof(uint16_t)));
        launch_fisheye_map(s, cam, W, H, h->d_fmap_xy, h->d_fmap_f);
        HIPCHK(h, hipGetLastError());
        h->fmap_w = W, h->fmap_h = H;
        std::memcpy(h->fmap_key, key, sizeof(key));
    }
    // staged in the arena: the host frames, then the packed result a host caller gets
    const size_t row = (size_t)W * channels;
    const Images in = images(src, nframes, H, row, row_stride, frame_stride, src_on_device), out = images(dst, nframes, H, row, row, row * H, dst_on_device);
    size_t src_at, dst_at;
    if ((rc = carve_scratch(h, h, [&](Carver& cv) {
             src_at = cv.take_at(src_on_device ? 0 : in.packed_bytes());
             dst_at = cv.take_at(dst_on_device ? 0 : out.packed_bytes());
         })))
        return rc;
    DevImages sdev, ddev;
    if ((rc = stage_input(h, s, in, h->scratch, src_at, &sdev))) return rc;
    if ((rc = stage_output(h, out, h->scratch, dst_at, &ddev))) return rc;
    launch_remap(s, sdev.p, sdev.row, sdev.frame, W, H, channels, nframes, h->d_fmap_xy, h->d_fmap_f, ddev.p);
    HIPCHK(h, hipGetLastError());
    if ((rc = unstage(h, s, out, ddev))) return rc;
    if (!dst_on_device) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_fisheye_undistort_markers_batch(arucohip_handle* h, int nframes, const arucohip_fisheye_t* models, int nmodels, const float* Knew,
                                             float max_angle, arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device, int32_t* dropped) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    if (h->last.ideal) return fail(h, ARUCOHIP_E_INVALID, "fisheye_undistort_markers_batch: the last batch already holds ideal corners");
    if (!models || nmodels < 1) return fail(h, ARUCOHIP_E_INVALID, "fisheye_undistort_markers_batch: at least one model is required");
    if ((out == nullptr) != (n_out == nullptr) || (out && cap < 1))
        return fail(h, ARUCOHIP_E_INVALID, "fisheye_undistort_markers_batch: out and n_out go together, with cap >= 1");
    std::vector<FisheyeCam> cams((size_t)nmodels);
    int rc;
    for (int i = 0; i < nmodels; i++)
        if ((rc = make_fisheye_cam(h, models + i, Knew ? Knew + 9 * i : nullptr, max_angle, &cams[i]))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    h->fisheye_cams.swap(cams);
    const size_t cam_bytes = (size_t)nmodels * sizeof(FisheyeCam);
    const bool wait = (out && !out_on_device) || dropped;

    const Batch b = h->last.cut(nframes);
    std::vector<std::vector<arucohip_marker_t>> stage((size_t)b.nspan);
    std::vector<int32_t> n_host((size_t)nframes);
    rc = on_workers(h, b, [&](const Span& s) -> int {
        h->last.ideal = true;       // from the first span on a worker's lists may have changed, whatever happens to the rest of the call
        h->last.board_frames = 0;   // board poses left on the device came from the distorted corners
        arucohip_handle* w = s.w;
        int32_t* d_dropped;
        FisheyeCam* d_cams;
        if (const int e = carve_scratch(w, h, [&](Carver& cv) {
                d_dropped = cv.take<int32_t>((size_t)w->cap_frames);
                d_cams = cv.take<FisheyeCam>((size_t)nmodels);
            }))
            return e;
        hipStream_t st = w->stream;
        HIPCHK(h, hipMemcpyAsync(d_cams, h->fisheye_cams.data(), cam_bytes, hipMemcpyHostToDevice, st));
        launch_fisheye_markers(st, d_cams, nmodels, s.first, s.count, w->buf, d_dropped);
        if (out)
            if (const int e = enqueue_markers(h, s, out, cap, n_out, out_on_device, &stage[b.index(s)], n_host.data() + s.first)) return e;
        if (dropped) HIPCHK(h, hipMemcpyAsync(dropped + s.first, d_dropped, (size_t)s.count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return ARUCOHIP_OK;
    });
    if (rc) return rc;
    if (!wait) return ARUCOHIP_OK;
    HIPCHK(h, hipStreamSynchronize(b.span[0].w->stream));
    int ret = ARUCOHIP_OK;
    if (out && !out_on_device)
        for (const Span& s : b) {
            const int r = collect_markers(h, s, cap, out, n_out, stage[b.index(s)].data(), n_host.data() + s.first);
            if (ret == ARUCOHIP_OK) ret = r;
        }
    return ret;
}

}  // extern "C"
