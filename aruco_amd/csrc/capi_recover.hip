// Host side of the board marker recovery (k_recover.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"

extern "C" {

void arucohip_default_recover(arucohip_recover_t* o) {
    if (!o) return;
    o->max_corner_dist = 10.f, o->max_cell_errors = 3, o->min_markers = 2, o->pose_markers = 0;
}

// r's arrays and the board (ids, obj) in a worker's arena for F frames of cap_markers markers and a board of nboard markers
static void recover_layout(RecoverBufs& r, int32_t** ids, float** obj, Carver& c, int F, int cap_markers, int nboard) {
    const size_t slots = (size_t)F * cap_markers;
    r.base = c.take<int32_t>((size_t)F), r.nrec = c.take<int32_t>((size_t)F), r.recovered = c.take<int32_t>((size_t)F);
    r.status = c.take<uint32_t>(1);
    r.rec = c.take<RecoverRec>(slots), r.rlist = c.take<uint32_t>(slots), r.plist = c.take<uint32_t>(slots);
    *ids = c.take<int32_t>((size_t)nboard), *obj = c.take<float>((size_t)nboard * 12);
}

int arucohip_board_recover_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type, const float* K,
                                 const float* dist, int ndist, float marker_size, float repj_err_thres, int y_perp, const arucohip_recover_t* opt,
                                 arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device, int32_t* recovered, arucohip_board_t* boards,
                                 float* prob) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (nboard <= 0 || !ids || !obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    if (nboard * 12 > 8192) return fail(h, ARUCOHIP_E_CAPACITY, "board with too many markers");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    if (h->last.ideal)
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "board_recover_batch: the markers hold ideal corners (arucohip_fisheye_undistort_markers_batch); undistort the frames instead");
    if ((out == nullptr) != (n_out == nullptr) || (out && cap < 1)) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: out and n_out go together, with cap >= 1");
    if (!K) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: K is required");
    if (info_type != ARUCOHIP_BOARD_PIX && info_type != ARUCOHIP_BOARD_METERS) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: info_type is neither PIX nor METERS");
    if (info_type == ARUCOHIP_BOARD_PIX && !(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: a PIX board needs marker_size > 0");
    arucohip_recover_t o;
    arucohip_default_recover(&o);
    if (opt) o = *opt;
    if (!(o.max_corner_dist > 0)) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: max_corner_dist must be positive");
    if (o.max_cell_errors < 0 || o.max_cell_errors > 49) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: max_cell_errors outside 0..49");
    if (o.min_markers < 1) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: min_markers must be at least 1");
    if (o.pose_markers && !(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "board_recover_batch: pose_markers needs marker_size > 0");
    const arucohip_params_t& p = h->params;
    if (p.corner_method != ARUCOHIP_CORNER_LINES && p.corner_method != ARUCOHIP_CORNER_NONE)
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "board_recover_batch: HARRIS / SUBPIX corners need the frames, which the handle does not hold");
    if (p.use_locked_corners) return fail(h, ARUCOHIP_E_UNSUPPORTED, "board_recover_batch: locked corners are not supported");
    if (p.decoder_kind != ARUCOHIP_DECODER_FIDUCIAL_5X5) return fail(h, ARUCOHIP_E_UNSUPPORTED, "board_recover_batch: only the built-in 5x5 decoder is supported (not HRM / USER)");
    if (ndist < 0 || ndist > 8 || (ndist > 0 && !dist)) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0..8, with dist");
    HIPCHK(h, hipSetDevice(h->device));
    // cam: the refinement's and the markers' own poses; bcam: the board solves, which always carry a distortion vector (board_detect_batch)
    CamModel cam, bcam;
    fill_cam(&cam, K, dist, ndist, marker_size, y_perp);
    bcam = cam, bcam.has_dist = 1;
    const BoardDef board{ids, obj, nboard, info_type, marker_size, repj_err_thres};
    RecoverArgs a;
    a.max_corner_dist = o.max_corner_dist, a.max_cell_errors = o.max_cell_errors, a.min_markers = o.min_markers;
    a.ws = p.warp_size;
    int rect[4];
    border_rect(p.border_dist, h->last.frame_w, h->last.frame_h, rect);
    a.bx0 = rect[0], a.by0 = rect[1], a.bx1 = rect[2], a.by1 = rect[3];
    const bool wait = !out_on_device || recovered || boards || prob;

    const Batch b = h->last.cut(nframes);
    std::vector<std::vector<arucohip_marker_t>> stage((size_t)b.nspan);
    std::vector<uint32_t> status((size_t)b.nspan, 0u);
    std::vector<int32_t> n_host((size_t)nframes);
    const int rc = on_workers(h, b, [&](const Span& s) -> int {
        const int c = b.index(s);
        arucohip_handle* w = s.w;
        const Buffers& wb = w->buf;
        const int capM = wb.cap_markers;
        RecoverBufs r;
        int32_t* dids;
        float* dobj;
        if (const int e = carve_scratch(w, h, [&](Carver& cv) { recover_layout(r, &dids, &dobj, cv, w->cap_frames, capM, nboard); })) return e;
        a.cells_valid = w->cells_valid ? 1 : 0;
        HIPCHK(h, w->d_board.reserve((size_t)w->cap_frames * (sizeof(arucohip_board_t) + sizeof(float)) + 8192 * sizeof(int32_t)));
        arucohip_board_t* d_boards = w->d_board;
        float* d_prob = (float*)(d_boards + w->cap_frames);
        hipStream_t st = w->stream;
        HIPCHK(h, hipMemsetAsync(r.base, 0xFF, (size_t)w->cap_frames * sizeof(int32_t), st));
        HIPCHK(h, hipMemsetAsync(r.status, 0, sizeof(uint32_t), st));
        if (const int e = upload_board(h, board, st, dids, dobj, &a.bd)) return e;
        launch_recover_match(st, h->last.span[c].count, s.count, wb, a, bcam, r);
        launch_refine_recovered(st, s.count, p.corner_method, cam, wb, r.rlist, r.nrec, capM);
        launch_recover_insert(st, s.count, wb, a, bcam, r, d_boards, d_prob);
        if (o.pose_markers) launch_pose_sparse(st, wb, r.plist, (uint32_t)s.count * (uint32_t)capM, cam);
        if (out)
            if (const int e = enqueue_markers(h, s, out, cap, n_out, out_on_device, &stage[c], n_host.data() + s.first)) return e;
        if (recovered) HIPCHK(h, hipMemcpyAsync(recovered + s.first, r.recovered, (size_t)s.count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (boards) HIPCHK(h, hipMemcpyAsync(boards + s.first, d_boards, (size_t)s.count * sizeof(arucohip_board_t), hipMemcpyDeviceToHost, st));
        if (prob) HIPCHK(h, hipMemcpyAsync(prob + s.first, d_prob, (size_t)s.count * sizeof(float), hipMemcpyDeviceToHost, st));
        if (wait) HIPCHK(h, hipMemcpyAsync(&status[c], r.status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        return ARUCOHIP_OK;
    });
    if (rc) return rc;
    h->last.board_frames = nframes;
    if (!wait) return ARUCOHIP_OK;
    HIPCHK(h, hipStreamSynchronize(b.span[0].w->stream));
    // the lists first: a board or a marker list that overflowed is reported ahead of an output array that is too small
    int ret = ARUCOHIP_OK;
    if (out && !out_on_device)
        for (int c = 0; c < b.nspan; c++) {
            const int r = collect_markers(h, b.span[c], cap, out, n_out, stage[c].data(), n_host.data() + b.span[c].first);
            if (ret == ARUCOHIP_OK) ret = r;
        }
    for (int c = 0; c < b.nspan; c++) {
        arucohip_handle* w = b.span[c].w;
        HIPCHK(h, hipMemcpy(w->h_counters, w->buf.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (w->h_counters[CNT_STATUS] & ST_MARKER_OVERFLOW) ret = fail(h, ARUCOHIP_E_CAPACITY, "a frame has more than 128 board markers");
        if (status[c] & 1u) ret = fail(h, ARUCOHIP_E_CAPACITY, "board_recover_batch: a frame's marker list is full (markers_per_frame)");
    }
    return ret;
}

}  // extern "C"
