// Host side of camera calibration (k_calib.hip): the pinhole entry points, and the pieces the fisheye ones (capi_fisheye.hip) share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

CalibCarve calib_carve(int V, size_t npts, int nframes, int nboard) {
    CalibCarve c;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    c.st = take(sizeof(CalibState));
    c.off = take((size_t)V * sizeof(int32_t)), c.npt = take((size_t)std::max(V, nframes) * sizeof(int32_t));
    c.init = take((size_t)V * 6 * sizeof(double)), c.red = take((size_t)V * CALIB_RED * sizeof(double));
    c.bs = take((size_t)V * CALIB_BS * sizeof(double)), c.pose = take((size_t)V * 12 * sizeof(double));
    c.vcost = take((size_t)V * 2 * sizeof(double)), c.vchg = take((size_t)V * 2 * sizeof(double));
    c.obj = take(npts * 3 * sizeof(float)), c.img = take(npts * 2 * sizeof(float));
    c.nmark = take((size_t)nframes * sizeof(int32_t));
    c.bids = take((size_t)nboard * sizeof(int32_t)), c.bobj = take((size_t)nboard * 12 * sizeof(float));
    c.total = at;
    return c;
}

// Levenberg-Marquardt on views whose points are already on the device (v.d.obj / v.d.img, offsets off[], counts npt[]) from the state
// `st` (start intrinsics, free mask, flags, model): start values, then one host synchronisation per iteration for the stop flag.
// focal_start: the focal lengths come from the views' homographies (pinhole without a guess).
int calib_solve(arucohip_handle* h, const CalibViews& v, CalibState st, bool focal_start, double intr[9], double* rvecs, double* tvecs,
                double* per_view_rms, double* rms) {
    CalibDev d = v.d;
    const CalibCarve& c = v.c;
    const int V = d.nviews;
    uint8_t* base = h->d_calib;
    d.off = (const int32_t*)(base + c.off), d.npt = (const int32_t*)(base + c.npt);
    d.init = (double*)(base + c.init), d.red = (double*)(base + c.red), d.bs = (double*)(base + c.bs);
    d.pose = (double*)(base + c.pose), d.vcost = (double*)(base + c.vcost), d.vchg = (double*)(base + c.vchg);
    d.st = (CalibState*)(base + c.st);
    st.max_iter = 30, st.lg = -3;
    hipStream_t s = h->stream;
    HIPCHK(h, h->hc_calib.reserve(sizeof(CalibState)));
    CalibState* hs = h->hc_calib;
    *hs = st;
    HIPCHK(h, hipMemcpyAsync(d.st, hs, sizeof(st), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync((void*)d.off, v.off.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync((void*)d.npt, v.npt.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_calib_init(s, d, !focal_start);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hs, d.st, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (hs->err & CALIB_ERR_NONPLANAR) return fail(h, ARUCOHIP_E_UNSUPPORTED, "calibration views must be planar (constant z per view)");
    if (hs->err) return fail(h, ARUCOHIP_E_INVALID, "degenerate calibration views: no start values");
    // at most 30 accepted steps; every rejected step raises lambda tenfold, and lambda above 1e16 stops
    for (int it = 0; it < 256 && !hs->done; it++) {
        launch_calib_iteration(s, d);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(hs, d.st, sizeof(st), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    st = *hs;
    std::vector<double> pose((size_t)V * 6), vcost((size_t)V);
    HIPCHK(h, hipMemcpyAsync(pose.data(), d.pose + (size_t)st.cur * V * 6, pose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(vcost.data(), d.vcost + (size_t)st.cur * V, vcost.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < 9; i++) intr[i] = st.intr[i];
    double e2 = 0, np = 0;
    for (int i = 0; i < V; i++) {
        e2 += vcost[i], np += v.npt[i];
        if (per_view_rms) per_view_rms[i] = std::sqrt(vcost[i] / v.npt[i]);
        for (int k = 0; k < 3; k++) {
            if (rvecs) rvecs[3 * i + k] = pose[6 * i + k];
            if (tvecs) tvecs[3 * i + k] = pose[6 * i + 3 + k];
        }
    }
    if (rms) *rms = std::sqrt(e2 / np);
    return ARUCOHIP_OK;
}

// the caller's views (host or device arrays) as the solver takes them, in h->d_calib
int calib_views_of_points(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, CalibViews* v) {
    HIPCHK(h, hipSetDevice(h->device));
    v->npt.resize((size_t)nviews), v->off.resize((size_t)nviews);
    if (on_device)
        HIPCHK(h, hipMemcpy(v->npt.data(), npoints, (size_t)nviews * sizeof(int32_t), hipMemcpyDeviceToHost));
    else
        std::memcpy(v->npt.data(), npoints, (size_t)nviews * sizeof(int32_t));
    size_t total = 0;
    for (int i = 0; i < nviews; i++) {
        if (v->npt[i] < 4) return fail(h, ARUCOHIP_E_INVALID, "a calibration view has fewer than 4 points");
        if (v->npt[i] > CALIB_MAX_POINTS) return fail(h, ARUCOHIP_E_CAPACITY, "a calibration view has more than ARUCOHIP_CALIB_MAX_VIEW_POINTS points");
        v->off[i] = (int32_t)total, total += (size_t)v->npt[i];
    }
    if (total > (size_t)INT32_MAX) return fail(h, ARUCOHIP_E_CAPACITY, "too many calibration points");
    v->c = calib_carve(nviews, on_device ? 0 : total, 0, 0);
    HIPCHK(h, h->d_calib.reserve(v->c.total));
    v->d = CalibDev{};
    v->d.nviews = nviews;
    if (on_device) {
        v->d.obj = obj, v->d.img = img;
    } else {
        float* dobj = (float*)((uint8_t*)h->d_calib + v->c.obj);
        float* dimg = (float*)((uint8_t*)h->d_calib + v->c.img);
        HIPCHK(h, hipMemcpyAsync(dobj, obj, total * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dimg, img, total * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        v->d.obj = dobj, v->d.img = dimg;
    }
    return ARUCOHIP_OK;
}

// the board detections of the last batch's first nframes frames as views, where they are: *owner is the worker of the batch's first chunk,
// in whose scratch and on whose stream the calibration then runs
int calib_views_of_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type, float marker_size,
                         int min_markers, int32_t* used, arucohip_handle** owner, CalibViews* v) {
    if (nboard <= 0 || !ids || !obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    arucohip_handle* o = b.span[0].w;
    *owner = o;
    // the metres-per-unit factor of board_pose_kernel for PIX boards (marker side from the first edge of marker 0)
    const float dx = obj[0] - obj[3], dy = obj[1] - obj[4], dz = obj[2] - obj[5];
    const double side = std::sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    const double mpp = (info_type == ARUCOHIP_BOARD_PIX && marker_size > 0) ? (double)marker_size / side : 1.0;
    const CalibCarve c = calib_carve(nframes, (size_t)nframes * CALIB_MAX_POINTS, nframes, nboard);
    HIPCHK(h, o->d_calib.reserve(c.total));
    uint8_t* base = o->d_calib;
    float* dobj = (float*)(base + c.obj);
    float* dimg = (float*)(base + c.img);
    int32_t* dnpt = (int32_t*)(base + c.npt);
    int32_t* dnmark = (int32_t*)(base + c.nmark);
    int32_t* dids = (int32_t*)(base + c.bids);
    float* dbobj = (float*)(base + c.bobj);
    HIPCHK(h, hipMemcpyAsync(dids, ids, (size_t)nboard * sizeof(int32_t), hipMemcpyHostToDevice, o->stream));
    HIPCHK(h, hipMemcpyAsync(dbobj, obj, (size_t)nboard * 12 * sizeof(float), hipMemcpyHostToDevice, o->stream));
    // every worker lays out the correspondences of the frames it detected, on its own stream
    int rc;
    if ((rc = fork_workers(h, b))) return rc;
    for (const Span& s : b) {
        launch_calib_gather(s.w->stream, s.count, s.w->buf, dids, dbobj, nboard, mpp, s.first, dobj, dimg, dnpt, dnmark);
        HIPCHK(h, hipGetLastError());
    }
    if ((rc = join_workers(h, b))) return rc;
    std::vector<int32_t> fnpt((size_t)nframes), fnmark((size_t)nframes);
    HIPCHK(h, hipMemcpyAsync(fnpt.data(), dnpt, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(h, hipMemcpyAsync(fnmark.data(), dnmark, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(h, hipStreamSynchronize(o->stream));
    v->off.clear(), v->npt.clear();
    for (int f = 0; f < nframes; f++) {
        const bool take = fnmark[f] >= std::max(min_markers, 1) && fnpt[f] != 0;
        if (take && fnpt[f] < 0) return fail(h, ARUCOHIP_E_CAPACITY, "a frame has more board points than ARUCOHIP_CALIB_MAX_VIEW_POINTS");
        if (used) used[f] = take ? 1 : 0;
        if (take) v->off.push_back(f * CALIB_MAX_POINTS), v->npt.push_back(fnpt[f]);
    }
    if (v->off.empty()) return fail(h, ARUCOHIP_E_INVALID, "no frame holds min_markers board markers");
    // the per-view arrays are carved for nframes >= views; the off / npt arrays are rewritten with the views
    v->c = c, v->d = CalibDev{};
    v->d.nviews = (int)v->off.size(), v->d.obj = dobj, v->d.img = dimg;
    return ARUCOHIP_OK;
}

// the pinhole run: start state from (K, dist, flags), results back into K and dist
static int calib_pinhole(arucohip_handle* h, const CalibViews& v, int W, int H, int flags, double* K, double* dist, double* rvecs, double* tvecs,
                         double* per_view_rms, double* rms) {
    const bool guess = flags & ARUCOHIP_CALIB_USE_INTRINSIC_GUESS;
    CalibState st;
    std::memset(&st, 0, sizeof(st));
    st.flags = flags, st.model = CALIB_MODEL_PINHOLE;
    st.aspect = (K[0] > 0 && K[4] > 0) ? K[0] / K[4] : 1.0;
    if (guess) {
        const double g[9] = {K[0], K[4], K[2], K[5], dist[0], dist[1], dist[2], dist[3], dist[4]};
        for (int i = 0; i < 9; i++) st.intr[i] = g[i];
        if (!(g[0] > 0 && g[1] > 0)) return fail(h, ARUCOHIP_E_INVALID, "USE_INTRINSIC_GUESS needs positive focal lengths");
        if (flags & ARUCOHIP_CALIB_FIX_ASPECT_RATIO) st.intr[0] = st.aspect * st.intr[1];
    } else {
        st.intr[2] = (W - 1) * 0.5, st.intr[3] = (H - 1) * 0.5;
    }
    if (flags & ARUCOHIP_CALIB_ZERO_TANGENT_DIST) st.intr[6] = st.intr[7] = 0;
    int mask = 0x1FF;
    if (flags & ARUCOHIP_CALIB_FIX_ASPECT_RATIO) mask &= ~1;
    if (flags & ARUCOHIP_CALIB_FIX_FOCAL_LENGTH) mask &= ~3;
    if (flags & ARUCOHIP_CALIB_FIX_PRINCIPAL_POINT) mask &= ~(4 | 8);
    if (flags & ARUCOHIP_CALIB_ZERO_TANGENT_DIST) mask &= ~(64 | 128);
    if (flags & ARUCOHIP_CALIB_FIX_K1) mask &= ~16;
    if (flags & ARUCOHIP_CALIB_FIX_K2) mask &= ~32;
    if (flags & ARUCOHIP_CALIB_FIX_K3) mask &= ~256;
    st.free_mask = mask;
    double in[9];
    const int rc = calib_solve(h, v, st, !guess, in, rvecs, tvecs, per_view_rms, rms);
    if (rc) return rc;
    const double Ko[9] = {in[0], 0, in[2], 0, in[1], in[3], 0, 0, 1};
    for (int i = 0; i < 9; i++) K[i] = Ko[i];
    for (int i = 0; i < 5; i++) dist[i] = in[4 + i];
    return ARUCOHIP_OK;
}

extern "C" {

int arucohip_calibrate_camera(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, int W,
                              int H, int flags, double* K, double* dist, double* rvecs, double* tvecs, double* per_view_rms, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!obj || !img || !npoints || !K || !dist || nviews < 1 || W <= 0 || H <= 0)
        return fail(h, ARUCOHIP_E_INVALID, "calibrate_camera: NULL argument, no views or an empty image size");
    CalibViews v;
    const int rc = calib_views_of_points(h, obj, img, npoints, nviews, on_device, &v);
    if (rc) return rc;
    return calib_pinhole(h, v, W, H, flags, K, dist, rvecs, tvecs, per_view_rms, rms);
}

int arucohip_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                   float marker_size, int min_markers, int W, int H, int flags, double* K, double* dist, int32_t* used,
                                   double* rvecs, double* tvecs, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!K || !dist || W <= 0 || H <= 0) return fail(h, ARUCOHIP_E_INVALID, "calibrate_board_batch: NULL K / dist or an empty image size");
    CalibViews v;
    arucohip_handle* o = nullptr;
    int rc = calib_views_of_batch(h, nframes, ids, obj, nboard, info_type, marker_size, min_markers, used, &o, &v);
    if (rc) return rc;
    rc = calib_pinhole(o, v, W, H, flags, K, dist, rvecs, tvecs, nullptr, rms);
    if (rc && o != h) h->err = o->err;
    return rc;
}

}  // extern "C"
