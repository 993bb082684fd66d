// Host side of camera calibration (k_calib.hip): the pinhole entry points, and the pieces the fisheye ones (capi_fisheye.hip) share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

// v's arrays from `c` for V views, npts staged points, nframes gather slots and a board of nboard markers.
// One quirk: npt is laid out for max(V, nframes) counts. A batch's gather counts every frame into it; the solve then overwrites
// off / npt with the (fewer) views that are used, and the per-view arrays, laid out for nframes, hold them with room to spare.
static void calib_layout(CalibViews& v, Carver& c, int V, size_t npts, int nframes, int nboard) {
    CalibDev& d = v.d;
    d.st = c.take<CalibState>(1);
    d.off = v.off_dev = c.take<int32_t>((size_t)V), d.npt = v.npt_dev = c.take<int32_t>((size_t)std::max(V, nframes));
    d.init = c.take<double>((size_t)V * 6), d.red = c.take<double>((size_t)V * CALIB_RED);
    d.bs = c.take<double>((size_t)V * CALIB_BS), d.pose = c.take<double>((size_t)V * 12);
    d.vcost = c.take<double>((size_t)V * 2), d.vchg = c.take<double>((size_t)V * 2);
    d.obj = v.obj = c.take<float>(npts * 3), d.img = v.img = c.take<float>(npts * 2);
    v.nmark = c.take<int32_t>((size_t)nframes);
    v.bids = c.take<int32_t>((size_t)nboard), v.bobj = c.take<float>((size_t)nboard * 12);
}

// the used views' offsets and counts, on h's stream
static int calib_counts_up(arucohip_handle* h, const CalibViews& v) {
    const size_t bytes = (size_t)v.d.nviews * sizeof(int32_t);
    HIPCHK(h, hipMemcpyAsync(v.off_dev, v.off.data(), bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(v.npt_dev, v.npt.data(), bytes, hipMemcpyHostToDevice, h->stream));
    return ARUCOHIP_OK;
}

// Levenberg-Marquardt (lm_drive) on views whose points are already on the device (v.d.obj / v.d.img, offsets off[], counts npt[]),
// in h's arena where v is bound, from the state `st` (start intrinsics, free mask, flags, model).
// focal_start: the focal lengths come from the views' homographies (pinhole without a guess).
int calib_solve(arucohip_handle* h, const CalibViews& v, CalibState st, bool focal_start, double intr[9], double* rvecs, double* tvecs,
                double* per_view_rms, double* rms) {
    const CalibDev& d = v.d;
    const int V = d.nviews;
    hipStream_t s = h->stream;
    if (const int up = calib_counts_up(h, v)) return up;
    const int rc = lm_drive(
        h, d.st, &st, [&] { launch_calib_init(s, d, !focal_start); },
        [&](const CalibState& at) {
            if (at.lm.err & CALIB_ERR_NONPLANAR) return fail(h, ARUCOHIP_E_UNSUPPORTED, "calibration views must be planar (constant z per view)");
            return at.lm.err ? fail(h, ARUCOHIP_E_INVALID, "degenerate calibration views: no start values") : 0;
        },
        [&] { launch_calib_iteration(s, d); });
    if (rc) return rc;
    std::vector<double> pose((size_t)V * 6), vcost((size_t)V);
    HIPCHK(h, hipMemcpyAsync(pose.data(), d.pose + (size_t)st.lm.cur * V * 6, pose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(vcost.data(), d.vcost + (size_t)st.lm.cur * V, vcost.size() * sizeof(double), hipMemcpyDeviceToHost, s));
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

// the caller's views (host or device arrays) as the solver takes them, in h's arena
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
    const size_t staged = on_device ? 0 : total;
    if (const int rc = carve_scratch(h, h, [&](Carver& c) { calib_layout(*v, c, nviews, staged, 0, 0); })) return rc;
    v->d.nviews = nviews;
    if (on_device) {
        v->d.obj = obj, v->d.img = img;
    } else {
        HIPCHK(h, hipMemcpyAsync(v->obj, obj, total * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(v->img, img, total * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    return ARUCOHIP_OK;
}

// the board detections of the last batch's first nframes frames as views, where they are: *owner is the worker of the batch's first chunk,
// in whose scratch and on whose stream the calibration then runs
int calib_views_of_batch(arucohip_handle* h, int nframes, const BoardDef& board, int min_markers, int32_t* used, arucohip_handle** owner,
                         CalibViews* v) {
    const int nboard = board.nboard;
    if (nboard <= 0 || !board.ids || !board.obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    arucohip_handle* o = b.span[0].w;
    *owner = o;
    const double mpp = board_mpp(board);   // board_pose_kernel's scale
    const size_t npts = (size_t)nframes * CALIB_MAX_POINTS;
    if (const int rc = carve_scratch(o, h, [&](Carver& c) { calib_layout(*v, c, nframes, npts, nframes, nboard); })) return rc;
    BoardDef bd;
    if (const int e = upload_board(h, board, o->stream, v->bids, v->bobj, &bd)) return e;
    // every worker lays out the correspondences of the frames it detected, on its own stream
    const int rc = on_workers(h, b, [&](const Span& s) {
        launch_calib_gather(s.w->stream, s.count, s.w->buf, bd, mpp, s.first, v->obj, v->img, v->npt_dev, v->nmark);
        return 0;
    });
    if (rc) return rc;
    std::vector<int32_t> fnpt((size_t)nframes), fnmark((size_t)nframes);
    HIPCHK(h, hipMemcpyAsync(fnpt.data(), v->npt_dev, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(h, hipMemcpyAsync(fnmark.data(), v->nmark, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(h, hipStreamSynchronize(o->stream));
    v->off.clear(), v->npt.clear();
    for (int f = 0; f < nframes; f++) {
        const bool take = fnmark[f] >= std::max(min_markers, 1) && fnpt[f] != 0;
        if (take && fnpt[f] < 0) return fail(h, ARUCOHIP_E_CAPACITY, "a frame has more board points than ARUCOHIP_CALIB_MAX_VIEW_POINTS");
        if (used) used[f] = take ? 1 : 0;
        if (take) v->off.push_back(f * CALIB_MAX_POINTS), v->npt.push_back(fnpt[f]);
    }
    if (v->off.empty()) return fail(h, ARUCOHIP_E_INVALID, "no frame holds min_markers board markers");
    v->d.nviews = (int)v->off.size();   // <= nframes, for which the per-view arrays are laid out (calib_layout)
    return ARUCOHIP_OK;
}

// the start state of a pinhole run from (K, dist, flags)
static int calib_pinhole_state(arucohip_handle* h, int W, int H, int flags, const double* K, const double* dist, CalibState* stp) {
    const bool guess = flags & ARUCOHIP_CALIB_USE_INTRINSIC_GUESS;
    CalibState& st = *stp;
    std::memset(&st, 0, sizeof(st));
    st.flags = flags, st.model = CALIB_MODEL_PINHOLE;
    st.aspect = (K[0] > 0 && K[4] > 0) ? K[0] / K[4] : 1.0;
    if (guess) {
        intr9(K, dist, st.intr);
        if (!(st.intr[0] > 0 && st.intr[1] > 0)) return fail(h, ARUCOHIP_E_INVALID, "USE_INTRINSIC_GUESS needs positive focal lengths");
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
    return ARUCOHIP_OK;
}

// the pinhole run: start state from (K, dist, flags), results back into K and dist
static int calib_pinhole(arucohip_handle* h, const CalibViews& v, int W, int H, int flags, double* K, double* dist, double* rvecs, double* tvecs,
                         double* per_view_rms, double* rms) {
    CalibState st;
    int rc = calib_pinhole_state(h, W, H, flags, K, dist, &st);
    if (rc) return rc;
    double in[9];
    rc = calib_solve(h, v, st, !(flags & ARUCOHIP_CALIB_USE_INTRINSIC_GUESS), in, rvecs, tvecs, per_view_rms, rms);
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

int arucohip_debug_calib_start(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, int W,
                               int H, int flags, int model, const double* K, const double* dist, double* intr, double* poses, double* cost,
                               int32_t* err) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!obj || !img || !npoints || !K || !dist || !intr || !poses || !cost || !err || nviews < 1 || W <= 0 || H <= 0)
        return fail(h, ARUCOHIP_E_INVALID, "debug_calib_start: NULL argument, no views or an empty image size");
    if (model != CALIB_MODEL_PINHOLE && model != CALIB_MODEL_FISHEYE) return fail(h, ARUCOHIP_E_INVALID, "debug_calib_start: model is 0 (pinhole) or 1 (fisheye)");
    CalibViews v;
    int rc = calib_views_of_points(h, obj, img, npoints, nviews, on_device, &v);
    if (rc) return rc;
    CalibState st;
    bool focal_start = false;
    if (model == CALIB_MODEL_FISHEYE) {
        arucohip_fisheye_t m;
        for (int i = 0; i < 9; i++) m.K[i] = K[i];
        for (int i = 0; i < 4; i++) m.D[i] = dist[i];
        rc = calib_fisheye_state(h, W, H, flags, &m, &st);
    } else {
        rc = calib_pinhole_state(h, W, H, flags, K, dist, &st);
        focal_start = !(flags & ARUCOHIP_CALIB_USE_INTRINSIC_GUESS);
    }
    if (rc) return rc;
    if ((rc = calib_counts_up(h, v))) return rc;
    hipStream_t s = h->stream;
    CalibState* at = nullptr;
    if ((rc = lm_start(h, v.d.st, &st, [&] { launch_calib_init(s, v.d, !focal_start); }, &at))) return rc;
    HIPCHK(h, hipMemcpyAsync(poses, v.d.pose, (size_t)nviews * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < 9; i++) intr[i] = at->intr[i];
    *cost = at->lm.cost, *err = at->lm.err;
    return ARUCOHIP_OK;
}

int arucohip_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                   float marker_size, int min_markers, int W, int H, int flags, double* K, double* dist, int32_t* used,
                                   double* rvecs, double* tvecs, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!K || !dist || W <= 0 || H <= 0) return fail(h, ARUCOHIP_E_INVALID, "calibrate_board_batch: NULL K / dist or an empty image size");
    CalibViews v;
    arucohip_handle* o = nullptr;
    int rc = calib_views_of_batch(h, nframes, BoardDef{ids, obj, nboard, info_type, marker_size, -1.f}, min_markers, used, &o, &v);
    if (rc) return rc;
    rc = calib_pinhole(o, v, W, H, flags, K, dist, rvecs, tvecs, nullptr, rms);
    if (rc && o != h) h->err = o->err;
    return rc;
}

}  // extern "C"
