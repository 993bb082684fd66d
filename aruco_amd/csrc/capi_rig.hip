// Host side of the camera rig calls (k_rig.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

extern "C" {

// The writable ends of what a call uploads or gathers into the arena: the board, the cameras, and the observation arrays (staging of
// host arrays, or a batch's gather). d.obs_* are set by rig_begin from where the observations are (RigObs).
struct RigStage {
    int32_t* ids;
    float* bobj;
    RigCam* cams;
    int32_t *obs_view, *obs_id, *obs_cnt;
    float* obs_corners;
};
// d's arrays from `c` for T instants of C cameras, nboard markers and room for nobs staged observations.
static void rig_layout(RigDev& d, RigStage& w, Carver& c, int T, int C, int nboard, size_t nobs) {
    const size_t t = (size_t)T, nc = (size_t)C, V = t * nc, N = (size_t)6 * (C - 1), nb = (size_t)nboard;
    d.st = c.take<RigState>(1), w.ids = c.take<int32_t>(nb), w.bobj = c.take<float>(nb * 12);
    d.cams = w.cams = c.take<RigCam>(nc);
    d.vn = c.take<int32_t>(V), d.vok = c.take<int32_t>(V), d.vact = c.take<int32_t>(V), d.vT = c.take<double>(V * 12);
    d.pobj = c.take<float>(V * RIG_VIEW_POINTS * 3), d.pimg = c.take<float>(V * RIG_VIEW_POINTS * 2);
    d.edge_t = c.take<int32_t>((size_t)RIG_MAX_CAMERAS * RIG_MAX_CAMERAS), d.edge_q = c.take<int32_t>((size_t)RIG_MAX_CAMERAS * RIG_MAX_CAMERAS);
    d.calibrated = c.take<int32_t>(nc), d.cpose = c.take<double>(nc * 12);
    d.used = c.take<int32_t>(t), d.lead = c.take<int32_t>(t), d.ipose = c.take<double>(t * 12);
    d.gram = c.take<double>(V * RIG_G), d.rec = c.take<double>(V * RIG_REC), d.fu = c.take<double>(t * 6);
    d.S = c.take<double>(N * N), d.delta = c.take<double>(N);
    d.vcost = c.take<double>(V * 2), d.vchg = c.take<double>(t * 2);
    d.boards = c.take<arucohip_board_t>(t), d.views_used = c.take<int32_t>(t);
    w.obs_view = c.take<int32_t>(nobs), w.obs_id = c.take<int32_t>(nobs), w.obs_corners = c.take<float>(nobs * 8);
    w.obs_cnt = c.take<int32_t>(V);
}
// sized, reserved on o (the handle whose arena holds the run), then bound there
static int rig_reserve(arucohip_handle* h, arucohip_handle* o, RigDev& d, RigStage& w, int T, int C, int nboard, size_t nobs) {
    return carve_scratch(o, h, [&](Carver& c) { rig_layout(d, w, c, T, C, nboard, nobs); });
}

// the board and the cameras of a call, checked before anything runs
static int rig_args(arucohip_handle* h, const char* who, int ninstants, const arucohip_rig_camera_t* cams, int ncams, const BoardDef& b, int min_markers,
                    std::vector<RigCam>* rc) {
    char msg[160];
    auto bad = [&](int code, const char* what) {
        std::snprintf(msg, sizeof(msg), "%s: %s", who, what);
        return fail(h, code, msg);
    };
    if (!cams || ncams < 2) return bad(ARUCOHIP_E_INVALID, "at least two cameras are needed");
    if (ninstants < 1) return bad(ARUCOHIP_E_INVALID, "no instants");
    if (!b.ids || !b.obj || b.nboard < 1) return bad(ARUCOHIP_E_INVALID, "NULL or empty board");
    if (b.info_type != ARUCOHIP_BOARD_PIX && b.info_type != ARUCOHIP_BOARD_METERS) return bad(ARUCOHIP_E_INVALID, "the board is neither PIX nor METERS");
    if (b.info_type == ARUCOHIP_BOARD_PIX && !(b.marker_size > 0)) return bad(ARUCOHIP_E_INVALID, "a PIX board needs a marker size");
    if (min_markers < 1) return bad(ARUCOHIP_E_INVALID, "min_markers must be at least 1");
    if (ncams > RIG_MAX_CAMERAS) return bad(ARUCOHIP_E_CAPACITY, "more than ARUCOHIP_RIG_MAX_CAMERAS cameras");
    if (b.nboard > RIG_MAX_BOARD) return bad(ARUCOHIP_E_CAPACITY, "more than 128 board markers");
    for (int c = 0; c < ncams; c++)
        if (!(cams[c].ndist == 0 || cams[c].ndist == 4 || cams[c].ndist == 5)) return bad(ARUCOHIP_E_INVALID, "a camera's ndist must be 0, 4 or 5");
    rc->assign((size_t)ncams, RigCam{});
    for (int c = 0; c < ncams; c++) {
        RigCam& r = (*rc)[c];
        fill_cam(&r.cam, cams[c].K, cams[c].dist, cams[c].ndist, b.marker_size, 0);
        intr9(r.cam.K, r.cam.k, r.in);
    }
    return ARUCOHIP_OK;
}

// where the observations of a call lie on the device
struct RigObs {
    const int32_t* view;   // null: the strided layout of a batch
    const int32_t* id;
    const float* corners;
    const int32_t* cnt;
    int nobs, stride;
};

// d, bound in o's arena, gets the call's numbers and observations, and the board and the cameras go up on o's stream; the solve then
// starts with the view kernel. A rig pose passes the caller's camera transforms (pose_cams), which go up with the rest, so that nothing
// waits between the view kernel and the pose kernel; a calibration passes null and computes them.
static int rig_begin(arucohip_handle* o, RigDev& d, const RigStage& w, int ninstants, int ncams, const BoardDef& b, int min_markers,
                     const std::vector<RigCam>& rc, const RigObs& obs, const arucohip_rig_camera_t* pose_cams) {
    hipStream_t s = o->stream;
    d.ncams = ncams, d.ninstants = ninstants, d.min_markers = min_markers;
    d.obs_view = obs.view, d.obs_id = obs.id, d.obs_corners = obs.corners, d.obs_cnt = obs.cnt, d.nobs = obs.nobs, d.obs_stride = obs.stride;
    if (const int e = upload_board(o, b, s, w.ids, w.bobj, &d.bd)) return e;
    HIPCHK(o, hipMemcpyAsync(w.cams, rc.data(), rc.size() * sizeof(RigCam), hipMemcpyHostToDevice, s));
    std::vector<double> cpose;
    std::vector<int32_t> calibrated;
    if (pose_cams) {
        cpose.assign((size_t)ncams * 6, 0.), calibrated.resize((size_t)ncams);
        for (int k = 0; k < ncams; k++) {
            calibrated[k] = pose_cams[k].calibrated != 0;
            for (int i = 0; i < 3 && k > 0; i++) cpose[6 * k + i] = pose_cams[k].rvec[i], cpose[6 * k + 3 + i] = pose_cams[k].tvec[i];   // camera 0 is the rig frame
        }
        HIPCHK(o, hipMemcpyAsync(d.cpose, cpose.data(), cpose.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(o, hipMemcpyAsync(d.calibrated, calibrated.data(), calibrated.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    HIPCHK(o, hipStreamSynchronize(s));   // the vectors and the caller's arrays are pageable: the copies above have left them
    return ARUCOHIP_OK;
}

// observations given as arrays: staged in h's arena unless they are on the device already
static int rig_stage(arucohip_handle* h, const RigStage& w, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs,
                     int on_device, RigObs* obs) {
    ObsArrays at;
    const int rc = stage_obs(h, ObsArrays{obs_view, obs_id, obs_corners}, nobs, on_device, w.obs_view, w.obs_id, w.obs_corners, &at);
    *obs = RigObs{at.owner, at.id, at.corners, nullptr, nobs, 0};
    return rc;
}

// the markers of the first nframes frames of the last batch, laid out per view by the workers that hold them (in the owner's arena)
static int rig_gather(arucohip_handle* h, const Batch& b, const RigStage& w, int nframes, int stride, RigObs* obs) {
    *obs = RigObs{nullptr, w.obs_id, w.obs_corners, w.obs_cnt, nframes * stride, stride};
    return on_workers(h, b, [&](const Span& s) {
        launch_map_gather(s.w->stream, s.count, s.w->buf, s.first, stride, w.obs_id, w.obs_corners, w.obs_cnt);
        return 0;
    });
}

struct RigCalibOut {
    int32_t* used;
    double *board_rvec, *board_tvec, *camera_rms, *rms;
    int32_t* iterations;
};

// The view kernel, start values and Levenberg-Marquardt (lm_drive) on o's stream; the state goes up ahead of the view kernel, which
// does not read it, so that no copy stands between the kernels.
// Nothing of the caller's is written before the solve is over.
static int rig_calibrate_solve(arucohip_handle* o, const RigDev& d, arucohip_rig_camera_t* cams, const RigCalibOut& out) {
    const int T = d.ninstants, C = d.ncams, V = T * C;
    hipStream_t s = o->stream;
    RigState st;
    std::memset(&st, 0, sizeof(st));
    const int rc = lm_drive(
        o, d.st, &st, [&] { launch_rig_views(s, d), launch_rig_calib_init(s, d); },
        [&](const RigState& at) {
            if (at.lm.err & RIG_ERR_NO_REFERENCE) return fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: no eligible instant shows camera 0");
            if (at.lm.err & RIG_ERR_TOO_FEW) return fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: no camera shares an instant with camera 0");
            return at.lm.err ? fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: degenerate observations, no start values") : 0;
        },
        [&] { launch_rig_calib_iteration(s, d); });
    if (rc) return rc;
    launch_rig_calib_finish(s, d);
    HIPCHK(o, hipGetLastError());
    std::vector<double> cpose((size_t)C * 6), ipose((size_t)T * 6), vcost((size_t)V);
    std::vector<int32_t> calibrated((size_t)C), used((size_t)T), vact((size_t)V), vn((size_t)V);
    HIPCHK(o, hipMemcpyAsync(cpose.data(), d.cpose + (size_t)st.lm.cur * C * 6, cpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(ipose.data(), d.ipose + (size_t)st.lm.cur * T * 6, ipose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(vcost.data(), d.vcost + (size_t)st.lm.cur * V, vcost.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(calibrated.data(), d.calibrated, calibrated.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(used.data(), d.used, used.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(vact.data(), d.vact, vact.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(vn.data(), d.vn, vn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    std::vector<double> ce2((size_t)C, 0.), cnt((size_t)C, 0.);
    for (int t = 0; t < T; t++) {
        const bool u = used[t] != 0;
        if (out.used) out.used[t] = u ? 1 : 0;
        for (int k = 0; k < 3; k++) {
            if (out.board_rvec) out.board_rvec[3 * t + k] = u ? ipose[6 * t + k] : 0.;
            if (out.board_tvec) out.board_tvec[3 * t + k] = u ? ipose[6 * t + 3 + k] : 0.;
        }
        for (int c = 0; c < C; c++)
            if (vact[(size_t)t * C + c]) ce2[c] += vcost[(size_t)t * C + c], cnt[c] += 4. * vn[(size_t)t * C + c];
    }
    for (int c = 0; c < C; c++) {
        const bool cal = calibrated[c] != 0;
        cams[c].calibrated = cal ? 1 : 0;
        for (int k = 0; k < 3; k++) cams[c].rvec[k] = (cal && c) ? cpose[6 * c + k] : 0., cams[c].tvec[k] = (cal && c) ? cpose[6 * c + 3 + k] : 0.;
        if (out.camera_rms) out.camera_rms[c] = (cal && cnt[c] > 0) ? std::sqrt(ce2[c] / cnt[c]) : 0.;
    }
    if (out.rms) *out.rms = std::sqrt(st.lm.cost / st.npts);
    if (out.iterations) *out.iterations = st.lm.iters;
    return ARUCOHIP_OK;
}

// the view kernel and the pose kernel behind it (the caller's camera transforms went up in rig_begin), the results back
static int rig_pose_solve(arucohip_handle* o, const RigDev& d, arucohip_board_t* out, int32_t* views_used) {
    const int T = d.ninstants;
    hipStream_t s = o->stream;
    launch_rig_views(s, d);
    launch_rig_pose(s, d);
    HIPCHK(o, hipGetLastError());
    std::vector<int32_t> vu((size_t)T);
    HIPCHK(o, hipMemcpyAsync(out, d.boards, (size_t)T * sizeof(arucohip_board_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(vu.data(), d.views_used, vu.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    if (views_used) std::copy(vu.begin(), vu.end(), views_used);
    return ARUCOHIP_OK;
}

static int rig_pose_args(arucohip_handle* h, const char* who, const arucohip_rig_camera_t* cams, int ncams, const arucohip_board_t* out) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%s: ", who);
    if (!out) return fail(h, ARUCOHIP_E_INVALID, std::strcat(msg, "out is NULL"));
    for (int c = 0; c < ncams; c++)
        if (cams[c].calibrated) return ARUCOHIP_OK;
    return fail(h, ARUCOHIP_E_INVALID, std::strcat(msg, "no camera is calibrated"));
}

static bool rig_obs_ok(const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs) {
    return nobs >= 0 && (nobs == 0 || (obs_view && obs_id && obs_corners));
}

int arucohip_rig_calibrate(arucohip_handle* h, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs, int on_device,
                           int ninstants, arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard, int info_type,
                           float marker_size, int min_markers, int32_t* used, double* board_rvec, double* board_tvec, double* camera_rms, double* rms,
                           int32_t* iterations) {
    if (!h) return ARUCOHIP_E_INVALID;
    const BoardDef b{ids, obj, nboard, info_type, marker_size, -1.f};
    std::vector<RigCam> rc;
    int r = rig_args(h, "rig_calibrate", ninstants, cams, ncams, b, min_markers, &rc);
    if (r) return r;
    if (!rig_obs_ok(obs_view, obs_id, obs_corners, nobs)) return fail(h, ARUCOHIP_E_INVALID, "rig_calibrate: NULL observations or a negative count");
    HIPCHK(h, hipSetDevice(h->device));
    RigDev d{};
    RigStage w;
    if ((r = rig_reserve(h, h, d, w, ninstants, ncams, nboard, on_device ? 0 : (size_t)nobs))) return r;
    RigObs obs;
    if ((r = rig_stage(h, w, obs_view, obs_id, obs_corners, nobs, on_device, &obs))) return r;
    if ((r = rig_begin(h, d, w, ninstants, ncams, b, min_markers, rc, obs, nullptr))) return r;
    return rig_calibrate_solve(h, d, cams, RigCalibOut{used, board_rvec, board_tvec, camera_rms, rms, iterations});
}

int arucohip_rig_pose(arucohip_handle* h, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs, int on_device, int ninstants,
                      const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard, int info_type, float marker_size,
                      int min_markers, arucohip_board_t* out, int32_t* views_used) {
    if (!h) return ARUCOHIP_E_INVALID;
    const BoardDef b{ids, obj, nboard, info_type, marker_size, -1.f};
    std::vector<RigCam> rc;
    int r = rig_args(h, "rig_pose", ninstants, cams, ncams, b, min_markers, &rc);
    if (r) return r;
    if ((r = rig_pose_args(h, "rig_pose", cams, ncams, out))) return r;
    if (!rig_obs_ok(obs_view, obs_id, obs_corners, nobs)) return fail(h, ARUCOHIP_E_INVALID, "rig_pose: NULL observations or a negative count");
    HIPCHK(h, hipSetDevice(h->device));
    RigDev d{};
    RigStage w;
    if ((r = rig_reserve(h, h, d, w, ninstants, ncams, nboard, on_device ? 0 : (size_t)nobs))) return r;
    RigObs obs;
    if ((r = rig_stage(h, w, obs_view, obs_id, obs_corners, nobs, on_device, &obs))) return r;
    if ((r = rig_begin(h, d, w, ninstants, ncams, b, min_markers, rc, obs, cams))) return r;
    return rig_pose_solve(h, d, out, views_used);
}

// the batch forms: frame f of the last batch is view f
static int rig_batch(arucohip_handle* h, const char* who, int nframes, arucohip_rig_camera_t* cams, int ncams, const BoardDef& b, int min_markers,
                     const RigCalibOut* calib, arucohip_board_t* out, int32_t* views_used) {
    std::vector<RigCam> rc;
    int r = rig_args(h, who, nframes, cams, ncams, b, min_markers, &rc);
    if (r) return r;
    if (!calib && (r = rig_pose_args(h, who, cams, ncams, out))) return r;
    if (nframes % ncams != 0) return fail(h, ARUCOHIP_E_INVALID, "the frames are not whole instants: nframes is no multiple of ncams");
    if (nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch batch = h->last.cut(nframes);
    arucohip_handle* o = batch.span[0].w;   // the worker of the batch's first chunk: the solve runs on its stream, in its scratch
    int stride = 1;
    for (const Span& s : batch) stride = std::max(stride, s.w->buf.cap_markers);
    const int ninstants = nframes / ncams;
    RigDev d{};
    RigStage w;
    if ((r = rig_reserve(h, o, d, w, ninstants, ncams, b.nboard, (size_t)nframes * stride))) return r;
    RigObs obs;
    if ((r = rig_gather(h, batch, w, nframes, stride, &obs))) return r;
    r = rig_begin(o, d, w, ninstants, ncams, b, min_markers, rc, obs, calib ? nullptr : cams);
    if (!r) r = calib ? rig_calibrate_solve(o, d, cams, *calib) : rig_pose_solve(o, d, out, views_used);
    if (r && o != h) h->err = o->err;
    return r;
}

int arucohip_rig_calibrate_batch(arucohip_handle* h, int nframes, arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard,
                                 int info_type, float marker_size, int min_markers, int32_t* used, double* board_rvec, double* board_tvec,
                                 double* camera_rms, double* rms, int32_t* iterations) {
    if (!h) return ARUCOHIP_E_INVALID;
    const RigCalibOut out{used, board_rvec, board_tvec, camera_rms, rms, iterations};
    return rig_batch(h, "rig_calibrate_batch", nframes, cams, ncams, BoardDef{ids, obj, nboard, info_type, marker_size, -1.f}, min_markers, &out, nullptr, nullptr);
}

int arucohip_rig_pose_batch(arucohip_handle* h, int nframes, const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard,
                            int info_type, float marker_size, int min_markers, arucohip_board_t* out, int32_t* views_used) {
    if (!h) return ARUCOHIP_E_INVALID;
    return rig_batch(h, "rig_pose_batch", nframes, const_cast<arucohip_rig_camera_t*>(cams), ncams, BoardDef{ids, obj, nboard, info_type, marker_size, -1.f},
                     min_markers, nullptr, out, views_used);
}

}  // extern "C"
