// Host side of the camera rig calls (k_rig.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

extern "C" {

// Byte offsets into h->d_rig for T instants of C cameras, nboard markers and room for nobs staged observations.
struct RigCarve {
    size_t st, ids, bobj, cams, vn, vok, vact, vT, pobj, pimg, edge_t, edge_q, calibrated, cpose, used, lead, ipose, gram, rec, fu, S, delta, vcost, vchg,
        boards, views_used, obs_view, obs_id, obs_corners, obs_cnt, total;
};
static RigCarve rig_carve(int T, int C, int nboard, size_t nobs) {
    RigCarve c;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t t = (size_t)T, V = t * C, N = (size_t)6 * (C - 1);
    c.st = take(sizeof(RigState)), c.ids = take((size_t)nboard * sizeof(int32_t)), c.bobj = take((size_t)nboard * 12 * sizeof(float));
    c.cams = take((size_t)C * sizeof(RigCam));
    c.vn = take(V * sizeof(int32_t)), c.vok = take(V * sizeof(int32_t)), c.vact = take(V * sizeof(int32_t)), c.vT = take(V * 12 * sizeof(double));
    c.pobj = take(V * RIG_VIEW_POINTS * 3 * sizeof(float)), c.pimg = take(V * RIG_VIEW_POINTS * 2 * sizeof(float));
    c.edge_t = take((size_t)RIG_MAX_CAMERAS * RIG_MAX_CAMERAS * sizeof(int32_t)), c.edge_q = take((size_t)RIG_MAX_CAMERAS * RIG_MAX_CAMERAS * sizeof(int32_t));
    c.calibrated = take((size_t)C * sizeof(int32_t)), c.cpose = take((size_t)C * 12 * sizeof(double));
    c.used = take(t * sizeof(int32_t)), c.lead = take(t * sizeof(int32_t)), c.ipose = take(t * 12 * sizeof(double));
    c.gram = take(V * RIG_G * sizeof(double)), c.rec = take(V * RIG_REC * sizeof(double)), c.fu = take(t * 6 * sizeof(double));
    c.S = take(N * N * sizeof(double)), c.delta = take(N * sizeof(double));
    c.vcost = take(V * 2 * sizeof(double)), c.vchg = take(t * 2 * sizeof(double));
    c.boards = take(t * sizeof(arucohip_board_t)), c.views_used = take(t * sizeof(int32_t));
    c.obs_view = take(nobs * sizeof(int32_t)), c.obs_id = take(nobs * sizeof(int32_t)), c.obs_corners = take(nobs * 8 * sizeof(float));
    c.obs_cnt = take(V * sizeof(int32_t));
    c.total = at;
    return c;
}

// the board and the cameras of a call, checked before anything runs
struct RigBoard {
    const int32_t* ids;
    const float* obj;
    int nboard, info_type;
    float marker_size;
    int min_markers;
};

static int rig_args(arucohip_handle* h, const char* who, int ninstants, const arucohip_rig_camera_t* cams, int ncams, const RigBoard& b, std::vector<RigCam>* rc) {
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
    if (b.min_markers < 1) return bad(ARUCOHIP_E_INVALID, "min_markers must be at least 1");
    if (ncams > RIG_MAX_CAMERAS) return bad(ARUCOHIP_E_CAPACITY, "more than ARUCOHIP_RIG_MAX_CAMERAS cameras");
    if (b.nboard > RIG_MAX_BOARD) return bad(ARUCOHIP_E_CAPACITY, "more than 128 board markers");
    for (int c = 0; c < ncams; c++)
        if (!(cams[c].ndist == 0 || cams[c].ndist == 4 || cams[c].ndist == 5)) return bad(ARUCOHIP_E_INVALID, "a camera's ndist must be 0, 4 or 5");
    rc->assign((size_t)ncams, RigCam{});
    for (int c = 0; c < ncams; c++) {
        RigCam& r = (*rc)[c];
        r.cam.has_K = 1, r.cam.has_dist = cams[c].ndist > 0;
        for (int i = 0; i < 9; i++) r.cam.K[i] = cams[c].K[i];
        for (int i = 0; i < cams[c].ndist; i++) r.cam.k[i] = (double)cams[c].dist[i];
        r.cam.marker_size = b.marker_size;
        const double in[9] = {r.cam.K[0], r.cam.K[4], r.cam.K[2], r.cam.K[5], r.cam.k[0], r.cam.k[1], r.cam.k[2], r.cam.k[3], r.cam.k[4]};
        for (int i = 0; i < 9; i++) r.in[i] = in[i];
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

// d over o's d_rig, the board, the cameras and a cleared solver state uploaded, the view kernel launched on o's stream. A rig pose
// passes the caller's camera transforms (pose_cams), which go up with the rest, so that nothing waits between the view kernel and
// the pose kernel; a calibration passes null and computes them.
static int rig_begin(arucohip_handle* o, const RigCarve& c, int ninstants, int ncams, const RigBoard& b, const std::vector<RigCam>& rc, const RigObs& obs,
                     const arucohip_rig_camera_t* pose_cams, RigDev* out) {
    uint8_t* base = o->d_rig;
    hipStream_t s = o->stream;
    RigDev d{};
    d.ncams = ncams, d.ninstants = ninstants, d.nboard = b.nboard, d.min_markers = b.min_markers, d.info_type = b.info_type, d.marker_size = b.marker_size;
    d.obs_view = obs.view, d.obs_id = obs.id, d.obs_corners = obs.corners, d.obs_cnt = obs.cnt, d.nobs = obs.nobs, d.obs_stride = obs.stride;
    d.ids = (const int32_t*)(base + c.ids), d.bobj = (const float*)(base + c.bobj), d.cams = (const RigCam*)(base + c.cams);
    d.vn = (int32_t*)(base + c.vn), d.vok = (int32_t*)(base + c.vok), d.vact = (int32_t*)(base + c.vact), d.vT = (double*)(base + c.vT);
    d.pobj = (float*)(base + c.pobj), d.pimg = (float*)(base + c.pimg);
    d.edge_t = (int32_t*)(base + c.edge_t), d.edge_q = (int32_t*)(base + c.edge_q);
    d.calibrated = (int32_t*)(base + c.calibrated), d.cpose = (double*)(base + c.cpose);
    d.used = (int32_t*)(base + c.used), d.lead = (int32_t*)(base + c.lead), d.ipose = (double*)(base + c.ipose);
    d.gram = (double*)(base + c.gram), d.rec = (double*)(base + c.rec), d.fu = (double*)(base + c.fu);
    d.S = (double*)(base + c.S), d.delta = (double*)(base + c.delta), d.vcost = (double*)(base + c.vcost), d.vchg = (double*)(base + c.vchg);
    d.boards = (arucohip_board_t*)(base + c.boards), d.views_used = (int32_t*)(base + c.views_used);
    d.st = (RigState*)(base + c.st);
    HIPCHK(o, o->hc_rig.reserve(sizeof(RigState)));
    RigState* hs = o->hc_rig;
    std::memset(hs, 0, sizeof(*hs));
    hs->max_iter = 30, hs->lg = -3;
    HIPCHK(o, hipMemcpyAsync(d.st, hs, sizeof(*hs), hipMemcpyHostToDevice, s));
    HIPCHK(o, hipMemcpyAsync(base + c.ids, b.ids, (size_t)b.nboard * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(o, hipMemcpyAsync(base + c.bobj, b.obj, (size_t)b.nboard * 12 * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(o, hipMemcpyAsync(base + c.cams, rc.data(), rc.size() * sizeof(RigCam), hipMemcpyHostToDevice, s));
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
    launch_rig_views(s, d);
    HIPCHK(o, hipGetLastError());
    *out = d;
    return ARUCOHIP_OK;
}

// observations given as arrays: staged in h's d_rig unless they are on the device already
static int rig_stage(arucohip_handle* h, const RigCarve& c, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs,
                     int on_device, RigObs* obs) {
    uint8_t* base = h->d_rig;
    *obs = RigObs{obs_view, obs_id, obs_corners, nullptr, nobs, 0};
    if (!on_device) {
        if (nobs > 0) {
            HIPCHK(h, hipMemcpyAsync(base + c.obs_view, obs_view, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(base + c.obs_id, obs_id, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(base + c.obs_corners, obs_corners, (size_t)nobs * 8 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        obs->view = (const int32_t*)(base + c.obs_view), obs->id = (const int32_t*)(base + c.obs_id), obs->corners = (const float*)(base + c.obs_corners);
    }
    if (!obs->view) obs->view = (const int32_t*)(base + c.obs_view);   // nobs == 0: nothing is read
    return ARUCOHIP_OK;
}

// the markers of the first nframes frames of the last batch, laid out per view by the workers that hold them (in o's d_rig)
static int rig_gather(arucohip_handle* h, const Batch& b, arucohip_handle* o, const RigCarve& c, int nframes, int stride, RigObs* obs) {
    uint8_t* base = o->d_rig;
    int32_t* obs_id = (int32_t*)(base + c.obs_id);
    float* obs_corners = (float*)(base + c.obs_corners);
    int32_t* obs_cnt = (int32_t*)(base + c.obs_cnt);
    int rc;
    if ((rc = fork_workers(h, b))) return rc;
    hipError_t launched = hipSuccess;
    for (const Span& s : b) {
        launch_map_gather(s.w->stream, s.count, s.w->buf, s.first, stride, obs_id, obs_corners, obs_cnt);
        if (launched == hipSuccess) launched = hipGetLastError();
    }
    // the workers rejoin the first worker's stream whether or not every launch was taken
    if ((rc = join_workers(h, b))) return rc;
    HIPCHK(h, launched);
    *obs = RigObs{nullptr, obs_id, obs_corners, obs_cnt, nframes * stride, stride};
    return ARUCOHIP_OK;
}

struct RigCalibOut {
    int32_t* used;
    double *board_rvec, *board_tvec, *camera_rms, *rms;
    int32_t* iterations;
};

// Start values and Levenberg-Marquardt behind the view kernel, on o's stream; one host synchronisation per iteration for the stop flag.
// Nothing of the caller's is written before the solve is over.
static int rig_calibrate_solve(arucohip_handle* o, const RigDev& d, arucohip_rig_camera_t* cams, const RigCalibOut& out) {
    const int T = d.ninstants, C = d.ncams, V = T * C;
    hipStream_t s = o->stream;
    RigState* hs = o->hc_rig;
    launch_rig_calib_init(s, d);
    HIPCHK(o, hipGetLastError());
    HIPCHK(o, hipMemcpyAsync(hs, d.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    if (hs->err & RIG_ERR_NO_REFERENCE) return fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: no eligible instant shows camera 0");
    if (hs->err & RIG_ERR_TOO_FEW) return fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: no camera shares an instant with camera 0");
    if (hs->err) return fail(o, ARUCOHIP_E_INVALID, "rig_calibrate: degenerate observations, no start values");
    // at most 30 accepted steps; every rejected step raises lambda tenfold, and lambda above 1e16 stops
    for (int it = 0; it < 256 && !hs->done; it++) {
        launch_rig_calib_iteration(s, d);
        HIPCHK(o, hipGetLastError());
        HIPCHK(o, hipMemcpyAsync(hs, d.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
        HIPCHK(o, hipStreamSynchronize(s));
    }
    const RigState st = *hs;
    launch_rig_calib_finish(s, d);
    HIPCHK(o, hipGetLastError());
    std::vector<double> cpose((size_t)C * 6), ipose((size_t)T * 6), vcost((size_t)V);
    std::vector<int32_t> calibrated((size_t)C), used((size_t)T), vact((size_t)V), vn((size_t)V);
    HIPCHK(o, hipMemcpyAsync(cpose.data(), d.cpose + (size_t)st.cur * C * 6, cpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(ipose.data(), d.ipose + (size_t)st.cur * T * 6, ipose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(vcost.data(), d.vcost + (size_t)st.cur * V, vcost.size() * sizeof(double), hipMemcpyDeviceToHost, s));
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
    if (out.rms) *out.rms = std::sqrt(st.cost / st.npts);
    if (out.iterations) *out.iterations = st.iters;
    return ARUCOHIP_OK;
}

// the pose kernel behind the view kernel (the caller's camera transforms went up in rig_begin), the results back
static int rig_pose_solve(arucohip_handle* o, const RigDev& d, arucohip_board_t* out, int32_t* views_used) {
    const int T = d.ninstants;
    hipStream_t s = o->stream;
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
    const RigBoard b{ids, obj, nboard, info_type, marker_size, min_markers};
    std::vector<RigCam> rc;
    int r = rig_args(h, "rig_calibrate", ninstants, cams, ncams, b, &rc);
    if (r) return r;
    if (!rig_obs_ok(obs_view, obs_id, obs_corners, nobs)) return fail(h, ARUCOHIP_E_INVALID, "rig_calibrate: NULL observations or a negative count");
    HIPCHK(h, hipSetDevice(h->device));
    const RigCarve c = rig_carve(ninstants, ncams, nboard, on_device ? 0 : (size_t)nobs);
    HIPCHK(h, h->d_rig.reserve(c.total));
    RigObs obs;
    if ((r = rig_stage(h, c, obs_view, obs_id, obs_corners, nobs, on_device, &obs))) return r;
    RigDev d;
    if ((r = rig_begin(h, c, ninstants, ncams, b, rc, obs, nullptr, &d))) return r;
    return rig_calibrate_solve(h, d, cams, RigCalibOut{used, board_rvec, board_tvec, camera_rms, rms, iterations});
}

int arucohip_rig_pose(arucohip_handle* h, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs, int on_device, int ninstants,
                      const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard, int info_type, float marker_size,
                      int min_markers, arucohip_board_t* out, int32_t* views_used) {
    if (!h) return ARUCOHIP_E_INVALID;
    const RigBoard b{ids, obj, nboard, info_type, marker_size, min_markers};
    std::vector<RigCam> rc;
    int r = rig_args(h, "rig_pose", ninstants, cams, ncams, b, &rc);
    if (r) return r;
    if ((r = rig_pose_args(h, "rig_pose", cams, ncams, out))) return r;
    if (!rig_obs_ok(obs_view, obs_id, obs_corners, nobs)) return fail(h, ARUCOHIP_E_INVALID, "rig_pose: NULL observations or a negative count");
    HIPCHK(h, hipSetDevice(h->device));
    const RigCarve c = rig_carve(ninstants, ncams, nboard, on_device ? 0 : (size_t)nobs);
    HIPCHK(h, h->d_rig.reserve(c.total));
    RigObs obs;
    if ((r = rig_stage(h, c, obs_view, obs_id, obs_corners, nobs, on_device, &obs))) return r;
    RigDev d;
    if ((r = rig_begin(h, c, ninstants, ncams, b, rc, obs, cams, &d))) return r;
    return rig_pose_solve(h, d, out, views_used);
}

// the batch forms: frame f of the last batch is view f
static int rig_batch(arucohip_handle* h, const char* who, int nframes, arucohip_rig_camera_t* cams, int ncams, const RigBoard& b, const RigCalibOut* calib,
                     arucohip_board_t* out, int32_t* views_used) {
    std::vector<RigCam> rc;
    int r = rig_args(h, who, nframes, cams, ncams, b, &rc);
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
    const RigCarve c = rig_carve(ninstants, ncams, b.nboard, (size_t)nframes * stride);
    HIPCHK(h, o->d_rig.reserve(c.total));
    RigObs obs;
    if ((r = rig_gather(h, batch, o, c, nframes, stride, &obs))) return r;
    RigDev d;
    r = rig_begin(o, c, ninstants, ncams, b, rc, obs, calib ? nullptr : cams, &d);
    if (!r) r = calib ? rig_calibrate_solve(o, d, cams, *calib) : rig_pose_solve(o, d, out, views_used);
    if (r && o != h) h->err = o->err;
    return r;
}

int arucohip_rig_calibrate_batch(arucohip_handle* h, int nframes, arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard,
                                 int info_type, float marker_size, int min_markers, int32_t* used, double* board_rvec, double* board_tvec,
                                 double* camera_rms, double* rms, int32_t* iterations) {
    if (!h) return ARUCOHIP_E_INVALID;
    const RigCalibOut out{used, board_rvec, board_tvec, camera_rms, rms, iterations};
    return rig_batch(h, "rig_calibrate_batch", nframes, cams, ncams, RigBoard{ids, obj, nboard, info_type, marker_size, min_markers}, &out, nullptr, nullptr);
}

int arucohip_rig_pose_batch(arucohip_handle* h, int nframes, const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj, int nboard,
                            int info_type, float marker_size, int min_markers, arucohip_board_t* out, int32_t* views_used) {
    if (!h) return ARUCOHIP_E_INVALID;
    return rig_batch(h, "rig_pose_batch", nframes, const_cast<arucohip_rig_camera_t*>(cams), ncams, RigBoard{ids, obj, nboard, info_type, marker_size, min_markers},
                     nullptr, out, views_used);
}

}  // extern "C"
