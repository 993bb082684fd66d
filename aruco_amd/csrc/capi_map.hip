// Host side of marker mapping (k_map.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

extern "C" {

// The writable ends of what a call uploads or gathers into the arena: the listed ids, and the observation arrays (staging of host
// arrays, or a batch's gather). d.obs_* are set by the caller, who knows where the observations are.
struct MapStage {
    int32_t *ids, *obs_frame, *obs_id, *obs_cnt;
    float* obs_corners;
};
// d's arrays from `c` for F frames, nboard markers and room for nobs staged observations.
static void map_layout(MapDev& d, MapStage& w, Carver& c, int F, int nboard, size_t nobs) {
    const size_t N = (size_t)6 * (nboard - 1), f = (size_t)F, nb = (size_t)nboard;
    d.st = c.take<MapState>(1), d.ids = w.ids = c.take<int32_t>(nb);
    d.slot = c.take<int8_t>(f * MAP_MAX_MARKERS), d.fm = c.take<int8_t>(f * MAP_SLOTS), d.fn = c.take<int32_t>(f), d.used = c.take<int32_t>(f);
    d.fc = c.take<float>(f * MAP_SLOTS * 8), d.fT = c.take<double>(f * MAP_SLOTS * 12), d.fq = c.take<double>(f * MAP_SLOTS);
    d.edge_f = c.take<int32_t>((size_t)MAP_MAX_MARKERS * MAP_MAX_MARKERS), d.edge_q = c.take<double>((size_t)MAP_MAX_MARKERS * MAP_MAX_MARKERS);
    d.mapped = c.take<int32_t>(nb), d.mpose = c.take<double>(nb * 12), d.fpose = c.take<double>(f * 12);
    d.rec = c.take<double>(f * MAP_SLOTS * MAP_REC), d.fu = c.take<double>(f * 6);
    d.S = c.take<double>(N * N), d.delta = c.take<double>(N);
    d.vcost = c.take<double>(f * 2), d.vchg = c.take<double>(f * 2), d.scost = c.take<double>(f * MAP_SLOTS);
    d.obj = c.take<float>(nb * 12);
    w.obs_frame = c.take<int32_t>(nobs), w.obs_id = c.take<int32_t>(nobs), w.obs_corners = c.take<float>(nobs * 8);
    w.obs_cnt = c.take<int32_t>(f);
}

struct MapOut {
    float* obj;
    double *marker_rvec, *marker_tvec;
    int32_t* mapped;
    int32_t* used;
    double *frame_rvec, *frame_tvec, *marker_rms, *rms;
    int32_t* iterations;
};

static int map_args(arucohip_handle* h, int nframes, const int32_t* ids, int nboard, const float* K, const float* dist, int ndist, float marker_size,
                    const MapOut& o, CamModel* cam) {
    if (!K) return fail(h, ARUCOHIP_E_INVALID, "board_map: K is required");
    if (!(ndist == 0 || ndist == 4 || ndist == 5)) return fail(h, ARUCOHIP_E_INVALID, "board_map: ndist must be 0, 4 or 5");
    if (ndist > 0 && !dist) return fail(h, ARUCOHIP_E_INVALID, "board_map: dist is NULL with ndist > 0");
    if (!(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "board_map: marker size must be positive");
    if (!ids || nboard < 2) return fail(h, ARUCOHIP_E_INVALID, "board_map: at least two marker ids are needed");
    if (nframes < 1) return fail(h, ARUCOHIP_E_INVALID, "board_map: no frames");
    if (!o.obj || !o.marker_rvec || !o.marker_tvec || !o.mapped) return fail(h, ARUCOHIP_E_INVALID, "board_map: NULL obj / marker_rvec / marker_tvec / mapped");
    if (nboard > MAP_MAX_MARKERS) return fail(h, ARUCOHIP_E_CAPACITY, "board_map: more than ARUCOHIP_MAP_MAX_MARKERS markers");
    fill_cam(cam, K, dist, ndist, marker_size, 0);
    return ARUCOHIP_OK;
}

// Start values and Levenberg-Marquardt (lm_drive) on observations that are already on the device (d.obs_*), on o's stream and in
// o's arena, where d is bound.
static int map_solve(arucohip_handle* o, MapDev d, int32_t* dids, const int32_t* ids, const CamModel& cam, const MapOut& out) {
    const int F = d.nframes, nb = d.nboard;
    hipStream_t s = o->stream;
    d.half = (float)((double)cam.marker_size / 2.);
    MapState st;
    std::memset(&st, 0, sizeof(st));
    intr9(cam.K, cam.k, st.intr);
    HIPCHK(o, hipMemcpyAsync(dids, ids, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int rc = lm_drive(
        o, d.st, &st, [&] { launch_map_init(s, d, cam); },
        [&](const MapState& at) {
            if (at.lm.err & MAP_ERR_NO_REFERENCE) return fail(o, ARUCOHIP_E_INVALID, "board_map: the reference marker (the first id) is in no used frame");
            if (at.lm.err & MAP_ERR_TOO_FEW) return fail(o, ARUCOHIP_E_INVALID, "board_map: no marker is seen together with the reference marker");
            return at.lm.err ? fail(o, ARUCOHIP_E_INVALID, "board_map: degenerate observations, no start values") : 0;
        },
        [&] { launch_map_iteration(s, d); });
    if (rc) return rc;
    launch_map_finish(s, d);
    HIPCHK(o, hipGetLastError());
    std::vector<double> mpose((size_t)nb * 6), fpose((size_t)F * 6), scost((size_t)F * MAP_SLOTS);
    std::vector<int32_t> mapped((size_t)nb), used((size_t)F), fn((size_t)F);
    std::vector<int8_t> fm((size_t)F * MAP_SLOTS);
    HIPCHK(o, hipMemcpyAsync(mpose.data(), d.mpose + (size_t)st.lm.cur * nb * 6, mpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(fpose.data(), d.fpose + (size_t)st.lm.cur * F * 6, fpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(scost.data(), d.scost, scost.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(mapped.data(), d.mapped, mapped.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(used.data(), d.used, used.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(fn.data(), d.fn, fn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(fm.data(), d.fm, fm.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(out.obj, d.obj, (size_t)nb * 12 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    std::vector<double> me2((size_t)nb, 0.), mcnt((size_t)nb, 0.);
    for (int f = 0; f < F; f++) {
        const bool u = used[f] != 0;
        if (out.used) out.used[f] = u ? 1 : 0;
        for (int k = 0; k < 3; k++) {
            if (out.frame_rvec) out.frame_rvec[3 * f + k] = u ? fpose[6 * f + k] : 0.;
            if (out.frame_tvec) out.frame_tvec[3 * f + k] = u ? fpose[6 * f + 3 + k] : 0.;
        }
        if (!u) continue;
        for (int sl = 0; sl < fn[f]; sl++) {
            const int m = fm[(size_t)f * MAP_SLOTS + sl];
            me2[m] += scost[(size_t)f * MAP_SLOTS + sl], mcnt[m] += 4.;
        }
    }
    for (int m = 0; m < nb; m++) {
        out.mapped[m] = mapped[m];
        for (int k = 0; k < 3; k++) out.marker_rvec[3 * m + k] = mpose[6 * m + k], out.marker_tvec[3 * m + k] = mpose[6 * m + 3 + k];
        if (out.marker_rms) out.marker_rms[m] = (mapped[m] && mcnt[m] > 0) ? std::sqrt(me2[m] / mcnt[m]) : 0.;
    }
    if (out.rms) *out.rms = std::sqrt(st.lm.cost / (4. * st.nobs));
    if (out.iterations) *out.iterations = st.lm.iters;
    return ARUCOHIP_OK;
}

int arucohip_board_map(arucohip_handle* h, const int32_t* obs_frame, const int32_t* obs_id, const float* obs_corners, int nobs, int on_device,
                       int nframes, const int32_t* ids, int nboard, const float* K, const float* dist, int ndist, float marker_size, float* obj,
                       double* marker_rvec, double* marker_tvec, int32_t* mapped, int32_t* used, double* frame_rvec, double* frame_tvec,
                       double* marker_rms, double* rms, int32_t* iterations) {
    if (!h) return ARUCOHIP_E_INVALID;
    const MapOut out{obj, marker_rvec, marker_tvec, mapped, used, frame_rvec, frame_tvec, marker_rms, rms, iterations};
    CamModel cam;
    int rc = map_args(h, nframes, ids, nboard, K, dist, ndist, marker_size, out, &cam);
    if (rc) return rc;
    if (nobs < 0 || (nobs > 0 && (!obs_frame || !obs_id || !obs_corners))) return fail(h, ARUCOHIP_E_INVALID, "board_map: NULL observations or a negative count");
    HIPCHK(h, hipSetDevice(h->device));
    MapDev d{};
    MapStage w;
    const size_t staged = on_device ? 0 : (size_t)nobs;
    if ((rc = carve_scratch(h, h, [&](Carver& c) { map_layout(d, w, c, nframes, nboard, staged); }))) return rc;
    d.nframes = nframes, d.nboard = nboard, d.min_markers = 2, d.nobs = nobs;
    ObsArrays obs;
    if ((rc = stage_obs(h, ObsArrays{obs_frame, obs_id, obs_corners}, nobs, on_device, w.obs_frame, w.obs_id, w.obs_corners, &obs))) return rc;
    d.obs_frame = obs.owner, d.obs_id = obs.id, d.obs_corners = obs.corners;
    return map_solve(h, d, w.ids, ids, cam, out);
}

int arucohip_board_map_batch(arucohip_handle* h, int nframes, const int32_t* ids, int nboard, const float* K, const float* dist, int ndist,
                             float marker_size, int min_markers, float* obj, double* marker_rvec, double* marker_tvec, int32_t* mapped, int32_t* used,
                             double* frame_rvec, double* frame_tvec, double* marker_rms, double* rms, int32_t* iterations) {
    if (!h) return ARUCOHIP_E_INVALID;
    const MapOut out{obj, marker_rvec, marker_tvec, mapped, used, frame_rvec, frame_tvec, marker_rms, rms, iterations};
    CamModel cam;
    int rc = map_args(h, nframes, ids, nboard, K, dist, ndist, marker_size, out, &cam);
    if (rc) return rc;
    if (nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    arucohip_handle* o = b.span[0].w;   // the worker of the batch's first chunk: the solve runs on its stream, in its scratch
    int stride = 1;
    for (const Span& s : b) stride = std::max(stride, s.w->buf.cap_markers);
    MapDev d{};
    MapStage w;
    if ((rc = carve_scratch(o, h, [&](Carver& c) { map_layout(d, w, c, nframes, nboard, (size_t)nframes * stride); }))) return rc;
    // every worker lays out the markers of the frames it detected, on its own stream
    rc = on_workers(h, b, [&](const Span& s) {
        launch_map_gather(s.w->stream, s.count, s.w->buf, s.first, stride, w.obs_id, w.obs_corners, w.obs_cnt);
        return 0;
    });
    if (rc) return rc;
    d.nframes = nframes, d.nboard = nboard, d.min_markers = min_markers, d.nobs = nframes * stride;
    d.obs_id = w.obs_id, d.obs_corners = w.obs_corners, d.obs_cnt = w.obs_cnt, d.obs_stride = stride;
    rc = map_solve(o, d, w.ids, ids, cam, out);
    if (rc && o != h) h->err = o->err;
    return rc;
}

}  // extern "C"
