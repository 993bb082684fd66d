// Host side of marker mapping (k_map.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

extern "C" {

// Byte offsets into h->d_map for F frames, nboard markers and room for nobs staged observations.
struct MapCarve {
    size_t st, ids, slot, fm, fn, used, fc, fT, fq, edge_f, edge_q, mapped, mpose, fpose, rec, fu, S, delta, vcost, vchg, scost, obj, obs_frame, obs_id,
        obs_corners, obs_cnt, total;
};
static MapCarve map_carve(int F, int nboard, size_t nobs) {
    MapCarve c;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t N = (size_t)6 * (nboard - 1), f = (size_t)F;
    c.st = take(sizeof(MapState)), c.ids = take((size_t)nboard * sizeof(int32_t));
    c.slot = take(f * MAP_MAX_MARKERS), c.fm = take(f * MAP_SLOTS), c.fn = take(f * sizeof(int32_t)), c.used = take(f * sizeof(int32_t));
    c.fc = take(f * MAP_SLOTS * 8 * sizeof(float)), c.fT = take(f * MAP_SLOTS * 12 * sizeof(double)), c.fq = take(f * MAP_SLOTS * sizeof(double));
    c.edge_f = take((size_t)MAP_MAX_MARKERS * MAP_MAX_MARKERS * sizeof(int32_t)), c.edge_q = take((size_t)MAP_MAX_MARKERS * MAP_MAX_MARKERS * sizeof(double));
    c.mapped = take((size_t)nboard * sizeof(int32_t)), c.mpose = take((size_t)nboard * 12 * sizeof(double)), c.fpose = take(f * 12 * sizeof(double));
    c.rec = take(f * MAP_SLOTS * MAP_REC * sizeof(double)), c.fu = take(f * 6 * sizeof(double));
    c.S = take(N * N * sizeof(double)), c.delta = take(N * sizeof(double));
    c.vcost = take(f * 2 * sizeof(double)), c.vchg = take(f * 2 * sizeof(double)), c.scost = take(f * MAP_SLOTS * sizeof(double));
    c.obj = take((size_t)nboard * 12 * sizeof(float));
    c.obs_frame = take(nobs * sizeof(int32_t)), c.obs_id = take(nobs * sizeof(int32_t)), c.obs_corners = take(nobs * 8 * sizeof(float));
    c.obs_cnt = take(f * sizeof(int32_t));
    c.total = at;
    return c;
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
    std::memset(cam, 0, sizeof(*cam));
    cam->has_K = 1;
    for (int i = 0; i < 9; i++) cam->K[i] = K[i];
    cam->has_dist = ndist > 0;
    for (int i = 0; i < ndist; i++) cam->k[i] = (double)dist[i];
    cam->marker_size = marker_size;
    return ARUCOHIP_OK;
}

// Start values and Levenberg-Marquardt on observations that are already on the device (d.obs_*), on o's stream and in o's d_map; one
// host synchronisation per iteration for the stop flag.
static int map_solve(arucohip_handle* o, MapDev d, const MapCarve& c, const int32_t* ids, const CamModel& cam, const MapOut& out) {
    const int F = d.nframes, nb = d.nboard;
    uint8_t* base = o->d_map;
    hipStream_t s = o->stream;
    int32_t* dids = (int32_t*)(base + c.ids);
    d.ids = dids;
    d.half = (float)((double)cam.marker_size / 2.);
    d.slot = (int8_t*)(base + c.slot), d.fm = (int8_t*)(base + c.fm), d.fn = (int32_t*)(base + c.fn), d.used = (int32_t*)(base + c.used);
    d.fc = (float*)(base + c.fc), d.fT = (double*)(base + c.fT), d.fq = (double*)(base + c.fq);
    d.edge_f = (int32_t*)(base + c.edge_f), d.edge_q = (double*)(base + c.edge_q);
    d.mapped = (int32_t*)(base + c.mapped), d.mpose = (double*)(base + c.mpose), d.fpose = (double*)(base + c.fpose);
    d.rec = (double*)(base + c.rec), d.fu = (double*)(base + c.fu), d.S = (double*)(base + c.S), d.delta = (double*)(base + c.delta);
    d.vcost = (double*)(base + c.vcost), d.vchg = (double*)(base + c.vchg), d.scost = (double*)(base + c.scost);
    d.obj = (float*)(base + c.obj), d.st = (MapState*)(base + c.st);
    HIPCHK(o, o->hc_map.reserve(sizeof(MapState)));
    MapState* hs = o->hc_map;
    std::memset(hs, 0, sizeof(*hs));
    hs->max_iter = 30, hs->lg = -3;
    const double in[9] = {cam.K[0], cam.K[4], cam.K[2], cam.K[5], cam.k[0], cam.k[1], cam.k[2], cam.k[3], cam.k[4]};
    for (int i = 0; i < 9; i++) hs->intr[i] = in[i];
    HIPCHK(o, hipMemcpyAsync(d.st, hs, sizeof(*hs), hipMemcpyHostToDevice, s));
    HIPCHK(o, hipMemcpyAsync(dids, ids, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_map_init(s, d, cam);
    HIPCHK(o, hipGetLastError());
    HIPCHK(o, hipMemcpyAsync(hs, d.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    if (hs->err & MAP_ERR_NO_REFERENCE) return fail(o, ARUCOHIP_E_INVALID, "board_map: the reference marker (the first id) is in no used frame");
    if (hs->err & MAP_ERR_TOO_FEW) return fail(o, ARUCOHIP_E_INVALID, "board_map: no marker is seen together with the reference marker");
    if (hs->err) return fail(o, ARUCOHIP_E_INVALID, "board_map: degenerate observations, no start values");
    // at most 30 accepted steps; every rejected step raises lambda tenfold, and lambda above 1e16 stops
    for (int it = 0; it < 256 && !hs->done; it++) {
        launch_map_iteration(s, d);
        HIPCHK(o, hipGetLastError());
        HIPCHK(o, hipMemcpyAsync(hs, d.st, sizeof(*hs), hipMemcpyDeviceToHost, s));
        HIPCHK(o, hipStreamSynchronize(s));
    }
    const MapState st = *hs;
    launch_map_finish(s, d);
    HIPCHK(o, hipGetLastError());
    std::vector<double> mpose((size_t)nb * 6), fpose((size_t)F * 6), scost((size_t)F * MAP_SLOTS);
    std::vector<int32_t> mapped((size_t)nb), used((size_t)F), fn((size_t)F);
    std::vector<int8_t> fm((size_t)F * MAP_SLOTS);
    HIPCHK(o, hipMemcpyAsync(mpose.data(), d.mpose + (size_t)st.cur * nb * 6, mpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipMemcpyAsync(fpose.data(), d.fpose + (size_t)st.cur * F * 6, fpose.size() * sizeof(double), hipMemcpyDeviceToHost, s));
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
    if (out.rms) *out.rms = std::sqrt(st.cost / (4. * st.nobs));
    if (out.iterations) *out.iterations = st.iters;
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
    const MapCarve c = map_carve(nframes, nboard, on_device ? 0 : (size_t)nobs);
    HIPCHK(h, h->d_map.reserve(c.total));
    MapDev d{};
    d.nframes = nframes, d.nboard = nboard, d.min_markers = 2, d.nobs = nobs;
    if (on_device) {
        d.obs_frame = obs_frame, d.obs_id = obs_id, d.obs_corners = obs_corners;
    } else {
        uint8_t* base = h->d_map;
        if (nobs > 0) {
            HIPCHK(h, hipMemcpyAsync(base + c.obs_frame, obs_frame, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(base + c.obs_id, obs_id, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(base + c.obs_corners, obs_corners, (size_t)nobs * 8 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        d.obs_frame = (const int32_t*)(base + c.obs_frame), d.obs_id = (const int32_t*)(base + c.obs_id);
        d.obs_corners = (const float*)(base + c.obs_corners);
    }
    if (!d.obs_frame) d.obs_frame = (const int32_t*)((uint8_t*)h->d_map + c.obs_frame);   // nobs == 0: nothing is read
    return map_solve(h, d, c, ids, cam, out);
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
    const MapCarve c = map_carve(nframes, nboard, (size_t)nframes * stride);
    HIPCHK(h, o->d_map.reserve(c.total));
    uint8_t* base = o->d_map;
    int32_t* obs_id = (int32_t*)(base + c.obs_id);
    float* obs_corners = (float*)(base + c.obs_corners);
    int32_t* obs_cnt = (int32_t*)(base + c.obs_cnt);
    // every worker lays out the markers of the frames it detected, on its own stream
    if ((rc = fork_workers(h, b))) return rc;
    hipError_t launched = hipSuccess;
    for (const Span& s : b) {
        launch_map_gather(s.w->stream, s.count, s.w->buf, s.first, stride, obs_id, obs_corners, obs_cnt);
        if (launched == hipSuccess) launched = hipGetLastError();
    }
    // the workers rejoin the first worker's stream whether or not every launch was taken
    if ((rc = join_workers(h, b))) return rc;
    HIPCHK(h, launched);
    MapDev d{};
    d.nframes = nframes, d.nboard = nboard, d.min_markers = min_markers, d.nobs = nframes * stride;
    d.obs_id = obs_id, d.obs_corners = obs_corners, d.obs_cnt = obs_cnt, d.obs_stride = stride;
    rc = map_solve(o, d, c, ids, cam, out);
    if (rc && o != h) h->err = o->err;
    return rc;
}

}  // extern "C"
