// Host side of libarucohip: handle, device buffers, launch order. Implements include/arucohip.h together with capi_calib.hip,
// capi_chromatic.hip and capi_hrm.hip (handle.h holds what they share).
//
// Launch order of one batch (all on the handle's stream, no host round trip until the final D2H of the markers):
//   memset counters -> threshold(+masks+start candidates) -> walkers -> contour/quad -> frame candidates ->
//   warp+decode -> corner refinement (+rotation) -> finalize -> pose
// which is the stage order of MarkerDetector::detect (/root/reference/src/markerdetector.cpp:302-478).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bits_tiles.h"
#include "handle.h"

namespace ah {
void launch_rotate_x(hipStream_t s, double* rt);
}

// the environment's switches, read when the caller creates a handle (every getenv of the handle is here)
static EnvSettings read_env() {
    EnvSettings v;
    auto geti = [](const char* name, int dflt) {
        const char* e = getenv(name);
        return (e && *e) ? atoi(e) : dflt;
    };
    if (const char* e = getenv("ARUCOHIP_STREAMS")) v.streams = std::min(MAX_WORKERS, std::max(1, atoi(e)));
    v.graph = geti("ARUCOHIP_GRAPH", 1) != 0;
    if (const char* e = getenv("ARUCOHIP_CONTOURS")) v.contours = std::string(e) == "segments";
    if (const char* e = getenv("ARUCOHIP_GRID")) v.grid = atoi(e);
    if (v.grid != 1 && v.grid != 2 && v.grid != 4 && v.grid != 8 && v.grid != 16 && v.grid != 32) v.grid = 8;
    v.thres_lazy = geti("ARUCOHIP_THRES_BYTES", 0) == 0;
    v.quad_dual = geti("ARUCOHIP_QUAD_DUAL", 1) != 0;
#ifdef ARUCOHIP_STAGE_EXPERIMENT
    v.stop_after = geti("ARUCOHIP_STOP_AFTER", 99);   // truncates the pipeline: results are meaningless, only the step time is
#endif
    return v;
}

enum { STAGE_THRESHOLD = 0, STAGE_RECTANGLES, STAGE_IDENTIFY, STAGE_SUBPIXEL, STAGE_FILTERING, STAGE_COUNT };
static const char* kStageNames[STAGE_COUNT] = {"Threshold", "Rectangles", "Identify", "Subpixel", "Filtering"};
static const char* kKernelNames[K_COUNT] = {"threshold_kernel", "candidates_kernel", "walker_kernel", "walker_long_kernel", "contour_quad_kernel",
                                            "frame_candidates_kernel", "decode_kernel", "refine_lines_kernel", "refine_pixels_kernel", "finalize_kernel",
                                            "pose_kernel"};
static const int kKernelStage[K_COUNT] = {STAGE_THRESHOLD, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES,
                                          STAGE_IDENTIFY, STAGE_IDENTIFY, STAGE_SUBPIXEL, STAGE_FILTERING, STAGE_FILTERING};

// chunk c of a batch runs on worker c: the handle itself, then its chunk workers
static arucohip_handle* chunk_worker(arucohip_handle* h, int c) { return c == 0 ? h : h->kids[c - 1]; }

// A batch of nframes frames on h's workers: chunks of equal size, as few as the workers' buffers allow but one per worker when the batch is
// large enough to share
static Batch plan_batch(arucohip_handle* h, int nframes, int W, int H, int nthr) {
    int chunks = (nframes + h->cap_frames - 1) / h->cap_frames;
    if (h->nsub > 1 && (size_t)nframes * W * H >= (size_t)h->nsub * 32 * 1024 * 1024) chunks = std::max(chunks, std::min(h->nsub, nframes));
    const int per = (nframes + chunks - 1) / chunks;
    chunks = (nframes + per - 1) / per;
    Batch b;
    b.nspan = chunks, b.frames = nframes, b.W = W, b.H = H, b.nthr = nthr, b.frame_w = W, b.frame_h = H;
    for (int c = 0; c < chunks; c++) b.span[c] = {chunk_worker(h, c), c * per, std::min(per, nframes - c * per)};
    return b;
}

// Visits every worker of h's tree: its chunk workers, each pipeline lane with the lane's chunk workers, then h itself (children first, so
// that f may delete what it visits), and stops at the first error f returns. The retry handle is not part of the tree (drop_retry).
template <class F>
static int for_each_worker(arucohip_handle* h, const F& f) {
    int rc = ARUCOHIP_OK;
    for (auto* k : h->kids)
        if (!rc) rc = f(k);
    for (auto* l : h->lanes)
        if (!rc) rc = for_each_worker(l, f);
    return rc ? rc : f(h);
}

// create-time memory: held by the handle for its whole life, `view` is the pointer the code uses
template <typename T>
static hipError_t hold(arucohip_handle* h, T*& view, size_t bytes, bool pinned = false) {
    Mem<void>& m = h->held.emplace_back(pinned);
    const hipError_t e = m.reserve(bytes);
    view = (T*)m.p;
    return e;
}

extern "C" {

int arucohip_version(void) { return ARUCOHIP_VERSION; }

#ifndef ARUCOHIP_SRC_HASH
#define ARUCOHIP_SRC_HASH "unknown"
#endif
#ifndef ARUCOHIP_EXTRA_FLAGS
#define ARUCOHIP_EXTRA_FLAGS ""
#endif
const char* arucohip_build_info(void) { return "src=" ARUCOHIP_SRC_HASH " flags=[" ARUCOHIP_EXTRA_FLAGS "]"; }

void arucohip_default_params(arucohip_params_t* p) {
    std::memset(p, 0, sizeof(*p));
    p->thres_method = ARUCOHIP_THRES_ADPT;
    p->thres_param1 = 7, p->thres_param2 = 7, p->thres_param1_range = 0;
    p->corner_method = ARUCOHIP_CORNER_LINES;
    p->warp_size = 56;
    p->min_size = 0.04f, p->max_size = 0.5f;
    p->border_dist = 0.025f;
    p->use_locked_corners = 0;
    p->decoder_kind = ARUCOHIP_DECODER_FIDUCIAL_5X5;
}

void arucohip_default_limits(arucohip_limits_t* l, int max_width, int max_height, int max_batch) {
    l->max_width = max_width, l->max_height = max_height, l->max_batch = std::max(max_batch, 1);
    l->max_thres_planes = 1;
    long px = (long)max_width * max_height;
    l->triggers_per_frame = (int)std::min<long>(std::max<long>(px / 16, 16384), 1 << 20);
    l->contours_per_frame = (int)std::min<long>(std::max<long>(px / 256, 1024), 16384);   // per threshold plane
    l->points_per_frame = (int)std::min<long>(std::max<long>(px / 8, 65536), 1 << 21);
    l->candidates_per_frame = 256;
    l->markers_per_frame = 128;
    // a synthetic 1080p frame has ~200 long walks per plane, a cluttered one several times that; small batches can afford
    // more rings (a ring is max contour length / 16 words)
    l->long_walks_per_plane = l->max_batch <= 16 ? 8192 : l->max_batch <= 128 ? 2048 : 1024;
}

static int validate_params(arucohip_handle* h, const arucohip_params_t* p) {
    // CV_Assert of setMinMaxSize (markerdetector.cpp:1032-1034) and setWarpSize (:1048)
    if (!(p->min_size > 0 && p->min_size <= 1) || !(p->max_size > 0 && p->max_size <= 1) || !(p->min_size < p->max_size))
        return fail(h, ARUCOHIP_E_INVALID, "setMinMaxSize: need 0 < min < max <= 1");
    if (p->warp_size < 10) return fail(h, ARUCOHIP_E_INVALID, "setWarpSize: need >= 10");
    if (p->warp_size > 128) return fail(h, ARUCOHIP_E_UNSUPPORTED, "warp size > 128 not supported");
    if (p->thres_method < ARUCOHIP_THRES_FIXED || p->thres_method > ARUCOHIP_THRES_CANNY) return fail(h, ARUCOHIP_E_INVALID, "bad threshold method");
    if (p->corner_method < ARUCOHIP_CORNER_NONE || p->corner_method > ARUCOHIP_CORNER_LINES) return fail(h, ARUCOHIP_E_INVALID, "bad corner method");
    if (p->use_locked_corners && (p->corner_method == ARUCOHIP_CORNER_HARRIS || p->corner_method == ARUCOHIP_CORNER_SUBPIX) &&
        ((int)p->thres_param1 < 1 || (int)p->thres_param1 > 31))
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "locked corners: window (thres_param1) outside 1..31");
    if (p->decoder_kind < ARUCOHIP_DECODER_FIDUCIAL_5X5 || p->decoder_kind > ARUCOHIP_DECODER_USER) return fail(h, ARUCOHIP_E_INVALID, "bad decoder kind");
    if (p->thres_param1_range < 0 || 2 * p->thres_param1_range + 1 > 16) return fail(h, ARUCOHIP_E_UNSUPPORTED, "threshold range too large");
    if (p->corner_method == ARUCOHIP_CORNER_SUBPIX && (int)p->thres_param1 > 15) return fail(h, ARUCOHIP_E_UNSUPPORTED, "SUBPIX window > 15");
    if (p->corner_method == ARUCOHIP_CORNER_SUBPIX && (int)p->thres_param1 < 1) return fail(h, ARUCOHIP_E_INVALID, "SUBPIX window < 1");
    return ARUCOHIP_OK;
}

// a worker's own graph, events and streams; its memory goes with its Mem members when it is deleted
static void release(arucohip_handle* h) {
    if (h->fgraph.exec) hipGraphExecDestroy(h->fgraph.exec);
    if (h->ev_submit) hipEventDestroy(h->ev_submit);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_wfork) hipEventDestroy(h->ev_wfork);
    if (h->ev_wjoin) hipEventDestroy(h->ev_wjoin);
    if (h->side_stream) hipStreamDestroy(h->side_stream);
    for (auto& e : h->ev_join)
        if (e) hipEventDestroy(e);
    for (auto& set : h->ev)
        for (auto& e : set)
            if (e) hipEventDestroy(e);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
}

// The one-frame handle of arucohip_detect_batch_retry_overflowed copies parameters, dictionary and decoder callback when it is made: whenever
// one of them changes it is dropped and the next retry builds a fresh one (a stale copy would decode retried frames with the old dictionary).
static void drop_retry(arucohip_handle* h) {
    if (h->retry) arucohip_destroy(h->retry);
    h->retry = nullptr, h->retry_mult = 0;
}

// device-clock stamps of the wide threshold kernel (k_threshold.hip): taken while `on`, the accumulators restart with them
static void arm_stamps(arucohip_handle* w, bool on) {
    w->buf.thr_stamp_on = on && w->buf.thr_stamps && w->buf.thr_acc;
    if (on && w->buf.thr_acc) {
        hipSetDevice(w->device);
        (void)hipStreamSynchronize(w->stream);
        (void)hipMemset(w->buf.thr_acc, 0, 2 * sizeof(uint64_t));
    }
}

// worker w takes dictionary d once its batches in flight, which may still read the old one, are done; errors are reported on h
static int load_dictionary(arucohip_handle* h, arucohip_handle* w, const Dictionary& d) {
    HIPCHK(h, hipStreamSynchronize(w->stream));
    w->hrm = Dictionary{};   // none until the device copy is complete
    if (d.count > 0) {
        HIPCHK(h, w->d_hrm.reserve((size_t)d.count * sizeof(uint64_t)));
        HIPCHK(h, hipMemcpy(w->d_hrm, d.codes.data(), (size_t)d.count * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    w->hrm = d;
    return ARUCOHIP_OK;
}

// a new child (chunk worker, pipeline lane, retry handle) and its own chunk workers take the parent's parameters, decoder callback,
// dictionary and timing
static int inherit(arucohip_handle* parent, arucohip_handle* child) {
    return for_each_worker(child, [&](arucohip_handle* w) {
        w->params = parent->params;
        w->pyr = parent->pyr;
        w->decoder_fn = parent->decoder_fn, w->decoder_user = parent->decoder_user;
        w->timing = parent->timing;
        arm_stamps(w, parent->buf.thr_stamp_on != 0);
        return load_dictionary(parent, w, parent->hrm);
    });
}

// is_kid: the handle is one of another's chunk workers and gets none of its own; in_lane: it is a pipeline lane or a lane's chunk worker, whose
// batches run with other batches in flight: no side stream (WalkFork); env: the switches of the handle the caller creates
static int create_handle(const arucohip_params_t* params, int device, const arucohip_limits_t* lim, bool is_kid, bool in_lane, const EnvSettings& env,
                         arucohip_handle** out);

// a new child of `parent` with limits `lim`, holding the parent's settings and environment switches (errors are reported on the parent)
static int create_child(arucohip_handle* parent, const arucohip_limits_t& lim, bool is_kid, bool in_lane, arucohip_handle** out) {
    int rc = create_handle(&parent->params, parent->device, &lim, is_kid, in_lane, parent->buf.env, out);
    if (rc == ARUCOHIP_OK && (rc = inherit(parent, *out)) != ARUCOHIP_OK) {
        arucohip_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

static int create_handle(const arucohip_params_t* params, int device, const arucohip_limits_t* lim, bool is_kid, bool in_lane, const EnvSettings& env,
                         arucohip_handle** out) {
    if (!out || !lim) return ARUCOHIP_E_INVALID;
    *out = nullptr;
    if (lim->max_width < 32 || lim->max_height < 32 || lim->max_width > 16383 || lim->max_height > 16383 || lim->max_batch < 1 ||
        lim->max_thres_planes < 1 || lim->max_thres_planes > 16 || lim->candidates_per_frame > MAX_CANDS_PER_FRAME || lim->markers_per_frame > 256 ||
        lim->triggers_per_frame < 1 || lim->contours_per_frame < 1 || lim->points_per_frame < 1 || lim->candidates_per_frame < 1 ||
        lim->markers_per_frame < 1 /* a zero is a list of no entries, a negative value a huge unsigned capacity */ ||
        (long)lim->max_width * lim->max_height > (1L << 26) /* Quad::key holds a 26-bit raster index */)
        return ARUCOHIP_E_INVALID;
    arucohip_handle* h = new arucohip_handle();
    h->device = device;
    h->in_lane = in_lane;
    h->lim = *lim;
    if (params)
        h->params = *params;
    else
        arucohip_default_params(&h->params);
    int rc = validate_params(h, &h->params);
    if (rc != ARUCOHIP_OK) {
        delete h;
        return rc;
    }
    auto bail = [&](hipError_t e) {
        fprintf(stderr, "arucohip_create: %s\n", hipGetErrorString(e));
        arucohip_destroy(h);
        return ARUCOHIP_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e);
    if ((e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
    h->stream = h->own_stream;
    Buffers& b = h->buf;
    b.env = env;
    h->fgraph.disabled = env.graph ? 0 : 1;
    // workers: one by default; ARUCOHIP_STREAMS = 2..8 cuts large batches into chunks on separate streams (copies of host frames then
    // overlap the kernels), chunk workers have none of their own. With the late walker generations on their own side stream a second
    // chunk stream no longer gains anything for device-resident frames (1 stream 208 k fps, 2 streams 208 k at 1024 1080p frames).
    h->nsub = std::min(is_kid ? 1 : env.streams, lim->max_batch);
    h->cap_frames = (lim->max_batch + h->nsub - 1) / h->nsub;
    const size_t F = h->cap_frames, P = F * lim->max_thres_planes, px = (size_t)lim->max_width * lim->max_height;
    b.cap_raw = (uint32_t)lim->triggers_per_frame;
    b.cap_trig = (uint32_t)std::max(lim->triggers_per_frame, 8192);   // two halves: outer starts, hole starts
    b.long_cap = (uint32_t)std::min(std::max(lim->long_walks_per_plane, 64), 1 << 16);
    h->lim.long_walks_per_plane = (int32_t)b.long_cap;
    b.cap_cdesc = (uint32_t)lim->contours_per_frame;   // per plane
    b.cap_pool = (uint32_t)lim->points_per_frame;       // per plane
    // pool offsets are 32-bit (ContourDesc::pool_off = plane * cap_pool + offset)
    if (P * (size_t)b.cap_pool > 0xFFFFFFF0ull) b.cap_pool = (uint32_t)(0xFFFFFFF0ull / P);
    b.cap_quads = std::min(lim->candidates_per_frame * 2, 512);
    b.cap_cands = lim->candidates_per_frame;
    b.cap_markers = lim->markers_per_frame;
#define ALLOC(ptr, bytes) if ((e = hold(h, ptr, (bytes))) != hipSuccess) return bail(e)
    ALLOC(b.thres, P * px);
    ALLOC(b.thres_edge, P * thres_edge_stride(lim->max_width, lim->max_height));
    {   // timing stamps of the wide threshold kernel: its finest grid is one wave per 1024-px strip and 16 rows
        const size_t waves = (size_t)tile_strips(lim->max_width) * ((lim->max_height + 15) / 16) * F;
        ALLOC(b.thr_stamps, 2 * waves * sizeof(uint64_t));
        ALLOC(b.thr_acc, 2 * sizeof(uint64_t));
        b.thr_stamp_on = 0;
    }
    const size_t bits_bytes = P * (size_t)tiles_x(lim->max_width) * tiles_y(lim->max_height) * sizeof(uint64_t) + 64;
    ALLOC(b.tiles, bits_bytes);
    if ((e = hipMemset(b.tiles, 0, bits_bytes)) != hipSuccess) return bail(e);   // pad tiles must read as zero
    h->tile_bits_bytes = P * (size_t)tiles_y(lim->max_height) * 2 * tile_strips(lim->max_width) * sizeof(uint64_t);
    ALLOC(b.tile_bits, h->tile_bits_bytes);
    // the 16-pixel-per-lane threshold kernels write the bitmap rows of real tile rows only; a frame lower than 17 pixels has a tile row
    // beyond them (tiles_y() is at least 4) whose words candidates_sparse_kernel reads: they must read as zero like the tiles there
    if ((e = hipMemset(b.tile_bits, 0, h->tile_bits_bytes)) != hipSuccess) return bail(e);
    h->bits_bytes = bits_bytes;
    ALLOC(b.trig, P * (size_t)b.cap_trig * sizeof(uint2));
    {
        // contour pipeline: ARUCOHIP_CONTOURS = walkers | segments; default by handle shape. The per-candidate walkers win on
        // batches; a single small frame is a chain of up to max-contour dependent border steps for them, which the waypoint
        // segments cut (bench.py latency leg, 1000 calls: 640x480 stills 0.67-0.72 ms vs 0.49-0.52 ms; one 1080p frame 0.80 vs 0.51 since round 4:
        // per-plane workgroup counts scaled for one frame, the run rule read from the lane's block)
        b.seg_mode = env.contours >= 0 ? env.contours : (lim->max_batch == 1 && (long)lim->max_width * lim->max_height <= 2048L * 1536L);
        b.grid_mask = env.grid - 1;
        uint32_t hs = 1;
        while (hs < 2u * b.cap_raw) hs <<= 1;
        b.hash_mask = hs - 1;
    }
    if (b.seg_mode) {   // waypoint-segment pipeline only: a walker handle of 1024 frames would carry 5 GB of these for nothing
        ALLOC(b.raw, P * (size_t)b.cap_raw * sizeof(uint2));
        ALLOC(b.node, P * (size_t)b.cap_raw * sizeof(uint4));
        if (lim->max_batch <= 2) ALLOC(b.skipn, P * (size_t)b.cap_raw * sizeof(uint4));
        ALLOC(b.stamp, P * (size_t)b.cap_raw * sizeof(unsigned long long));
        ALLOC(b.hash, P * (size_t)(b.hash_mask + 1) * sizeof(uint32_t));
    }
    ALLOC(b.gen_buf, ((P + 7) / 8 * 8) * (size_t)b.long_cap * 4 * 20);   // [2 kinds][2 parities][planes rounded up to 8 * long_cap] walk states (16 B) + ring ids (4 B)
    ALLOC(b.cdesc, P * (size_t)b.cap_cdesc * sizeof(ContourDesc));
    ALLOC(b.pool, P * (size_t)b.cap_pool * sizeof(short2));
    ALLOC(b.quads, F * b.cap_quads * sizeof(Quad));
    ALLOC(b.cands, F * b.cap_cands * sizeof(Cand));
    ALLOC(b.ncands, F * sizeof(int32_t));
    // 96 candidates per frame on the batch's average, and never less than one frame's own candidate list: a single frame may fill it
    b.cap_flat = (uint32_t)std::max<size_t>(std::min<size_t>(F * (size_t)std::min(b.cap_cands, 96), 65535u * 16u), (size_t)b.cap_cands);
    ALLOC(b.cand_list, (size_t)b.cap_flat * sizeof(uint32_t));
    ALLOC(b.iM, (size_t)b.cap_flat * 9 * sizeof(double));
    ALLOC(b.hist, (size_t)b.cap_flat * 256 * sizeof(uint16_t));
    ALLOC(b.othr, (size_t)b.cap_flat * sizeof(int32_t));
    ALLOC(b.cells, (size_t)b.cap_flat * 64);
    ALLOC(b.markers, (F * b.cap_markers + 1) * sizeof(arucohip_marker_t));   // + the header slot of a one-frame call (k_finalize.hip: write_hdr)
    ALLOC(b.nmarkers, F * sizeof(int32_t));
    ALLOC(b.marker_list, F * (size_t)b.cap_markers * sizeof(uint32_t));
    {
        // every counter a batch starts from zero with lives in one block: one memset per batch instead of five (a single frame's
        // call is a chain of ~25 short operations, each memset was 6 us of it)
        const size_t w_cnt = (CNT_FIXED + F + 31) & ~(size_t)31, w_plane = P * TRIG_CNT_STRIDE;
        h->zero_words = w_cnt + GEN_CNT_WORDS + 3 * w_plane;
        ALLOC(h->zero_block, h->zero_words * sizeof(uint32_t));
        b.counters = h->zero_block;
        b.gen_cnt = b.counters + w_cnt;
        b.trig_cnt = b.gen_cnt + GEN_CNT_WORDS;
        b.raw_cnt = b.trig_cnt + w_plane;
        b.ring_cnt = b.raw_cnt + w_plane;
    }
    ALLOC(h->d_small_f, 8192 * sizeof(float));
    ALLOC(h->d_small_d, 64 * sizeof(double));
    ALLOC(h->d_small_i, 64 * sizeof(int));
    ALLOC(h->d_patch, 128 * 128);
#undef ALLOC
    if ((e = hold(h, h->h_markers, (F * b.cap_markers + 1) * sizeof(arucohip_marker_t), true)) != hipSuccess) return bail(e);
    if ((e = hold(h, h->h_n, F * sizeof(int32_t), true)) != hipSuccess) return bail(e);
    if ((e = hold(h, h->h_counters, (CNT_FIXED + F) * sizeof(uint32_t), true)) != hipSuccess) return bail(e);
    for (auto& set : h->ev)
        for (auto& ev : set)
            if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e);
    if (!in_lane) {   // the one place that decides whether a handle's batches fork their late walker generations (run_rectangles, launch_walkers)
        if ((e = hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
        if ((e = hipEventCreateWithFlags(&h->ev_wfork, hipEventDisableTiming)) != hipSuccess) return bail(e);
        if ((e = hipEventCreateWithFlags(&h->ev_wjoin, hipEventDisableTiming)) != hipSuccess) return bail(e);
    }
    if (h->nsub > 1) {
        if ((e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)) != hipSuccess) return bail(e);
        for (int i = 0; i < h->nsub - 1; i++) {
            if ((e = hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming)) != hipSuccess) return bail(e);
            arucohip_limits_t kl = *lim;
            kl.max_batch = h->cap_frames;
            arucohip_handle* kid = nullptr;
            const int krc = create_child(h, kl, true, in_lane, &kid);
            if (krc != ARUCOHIP_OK) {
                arucohip_destroy(h);
                return krc;
            }
            h->kids.push_back(kid);
        }
    }
    *out = h;
    return ARUCOHIP_OK;
}

int arucohip_create_ex(const arucohip_params_t* params, int device, const arucohip_limits_t* lim, arucohip_handle** out) {
    return create_handle(params, device, lim, false, false, read_env(), out);
}

int arucohip_create(const arucohip_params_t* params, int device, int max_width, int max_height, int max_batch, arucohip_handle** out) {
    arucohip_limits_t l;
    arucohip_default_limits(&l, max_width, max_height, max_batch);
    if (params) l.max_thres_planes = std::max(1, 2 * params->thres_param1_range + 1);
    return arucohip_create_ex(params, device, &l, out);
}

void arucohip_destroy(arucohip_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    drop_retry(h);
    for_each_worker(h, [](arucohip_handle* w) { release(w); delete w; return ARUCOHIP_OK; });
}

int arucohip_set_params(arucohip_handle* h, const arucohip_params_t* p) {
    if (!h || !p) return ARUCOHIP_E_INVALID;
    int rc = validate_params(h, p);
    if (rc != ARUCOHIP_OK) return rc;
    if (2 * p->thres_param1_range + 1 > h->lim.max_thres_planes)
        return fail(h, ARUCOHIP_E_INVALID, "threshold range exceeds the planes this handle was created with");
    for_each_worker(h, [&](arucohip_handle* w) { w->params = *p; return ARUCOHIP_OK; });
    drop_retry(h);
    return ARUCOHIP_OK;
}

int arucohip_get_params(const arucohip_handle* h, arucohip_params_t* p) {
    if (!h || !p) return ARUCOHIP_E_INVALID;
    *p = h->params;
    return ARUCOHIP_OK;
}

const char* arucohip_last_error_string(const arucohip_handle* h) { return h ? h->err.c_str() : "null handle"; }

int arucohip_set_stream(arucohip_handle* h, void* s) {
    if (!h) return ARUCOHIP_E_INVALID;
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return ARUCOHIP_OK;
}
void* arucohip_get_stream(arucohip_handle* h) { return h ? (void*)h->stream : nullptr; }

int arucohip_synchronize(arucohip_handle* h) {
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_wait_event(arucohip_handle* h, void* ev) {
    if (!h || !ev) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    // a submit forks its lane from the handle's stream (ev_submit), so one wait here orders both forms behind the producer
    HIPCHK(h, hipStreamWaitEvent(h->stream, (hipEvent_t)ev, 0));
    return ARUCOHIP_OK;
}

int arucohip_enable_timing(arucohip_handle* h, int on) {
    if (!h) return ARUCOHIP_E_INVALID;
    // on == 2: only the threshold kernel's device-clock stamps, no hipEvents between the kernels (the launches then overlap with the other
    // batches exactly as in an uninstrumented run: bench.py's replica pass)
    for_each_worker(h, [&](arucohip_handle* w) {
        w->timing = on == 1, w->tsets = 0;
        w->render_ms[0] = w->render_ms[1] = 0, w->render_calls = 0;
        arm_stamps(w, on != 0);
        return ARUCOHIP_OK;
    });
    return ARUCOHIP_OK;
}
// synchronises the stream and averages the per-kernel event intervals of the batches since enable/reset
// (with sub-batch pipelining: the average over the launches of all workers, each launch covering one chunk)
static void collect_times(arucohip_handle* h) {
    for (int k = 0; k < K_COUNT; k++) h->kernel_ms[k] = 0;
    hipSetDevice(h->device);
    int total = 0;
    for_each_worker(h, [&](arucohip_handle* w) {
        const int n = std::min(w->tsets, TSETS);
        if (n <= 0 || hipStreamSynchronize(w->stream) != hipSuccess) return ARUCOHIP_OK;
        for (int s = 0; s < n; s++)
            for (int k = 0; k < K_COUNT; k++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, w->ev[s][k], w->ev[s][k + 1]) == hipSuccess) h->kernel_ms[k] += ms;
            }
        total += n;
        return ARUCOHIP_OK;
    });
    if (total > 0)
        for (int k = 0; k < K_COUNT; k++) h->kernel_ms[k] /= total;
}
const char* arucohip_stage_name(int i) { return (i >= 0 && i < STAGE_COUNT) ? kStageNames[i] : ""; }
int arucohip_stage_times(arucohip_handle* h, float* ms, int cap) {
    if (!h) return 0;
    collect_times(h);
    for (int i = 0; i < STAGE_COUNT && i < cap; i++) ms[i] = 0;
    for (int k = 0; k < K_COUNT; k++)
        if (kKernelStage[k] < cap) ms[kKernelStage[k]] += h->kernel_ms[k];
    return STAGE_COUNT;
}
const char* arucohip_kernel_name(int i) { return (i >= 0 && i < K_COUNT) ? kKernelNames[i] : ""; }
int arucohip_threshold_exec_ms(arucohip_handle* h, double* total_ms, int* launches) {
    if (!h || !total_ms || !launches) return ARUCOHIP_E_INVALID;
    hipSetDevice(h->device);
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) return fail(h, ARUCOHIP_E_HIP, "no wall clock rate");
    unsigned long long ticks = 0, n = 0;
    const int rc = for_each_worker(h, [&](arucohip_handle* w) {
        if (!w->buf.thr_acc) return ARUCOHIP_OK;
        unsigned long long v[2] = {0, 0};
        HIPCHK(h, hipStreamSynchronize(w->stream));
        HIPCHK(h, hipMemcpy(v, w->buf.thr_acc, sizeof(v), hipMemcpyDeviceToHost));
        ticks += v[0], n += v[1];
        return ARUCOHIP_OK;
    });
    if (rc != ARUCOHIP_OK) return rc;
    *total_ms = (double)ticks / (double)khz, *launches = (int)n;
    return ARUCOHIP_OK;
}

int arucohip_kernel_times(arucohip_handle* h, float* ms, int cap) {
    if (!h) return 0;
    collect_times(h);
    for (int i = 0; i < K_COUNT && i < cap; i++) ms[i] = h->kernel_ms[i];
    return K_COUNT;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// level: the pyramid level the rectangle stage runs at (detection: the handle's; the stage entry points work on the image they are given: 0)
static int make_detect_params(arucohip_handle* h, int W, int H, DetectParams* dp, int level = 0) {
    const arucohip_params_t& p = h->params;
    std::memset(dp, 0, sizeof(*dp));
    dp->pyr = level;
    dp->thres_method = p.thres_method;
    dp->nthr = 2 * p.thres_param1_range + 1;
    if (dp->nthr > h->lim.max_thres_planes) return fail(h, ARUCOHIP_E_INVALID, "threshold range exceeds handle planes");
    for (int i = 0; i < dp->nthr; i++) {
        // markerdetector.cpp:325-333 (step is the range itself) and the odd/>=3 fix-up of :657-660
        double p1 = dp->nthr == 1 ? p.thres_param1 : p.thres_param1 - p.thres_param1_range + (double)p.thres_param1_range * i;
        if (p.thres_method == ARUCOHIP_THRES_ADPT) {
            if (p1 < 3)
                p1 = 3;
            else if (((int)p1) % 2 != 1)
                p1 = (int)(p1 + 1);
            dp->block[i] = (int)p1;
            if (dp->block[i] > 31) return fail(h, ARUCOHIP_E_UNSUPPORTED, "adaptive threshold block size > 31");
        }
        dp->p1[i] = p1;
    }
    dp->idelta = (int)std::floor(p.thres_param2);
    dp->corner_method = p.corner_method;
    dp->warp_size = p.warp_size;
    // the contour bounds come from the image the contours are found on (the reference measured thres.cols / rows), the border filter
    // below from the frame
    int Wr = W, Hr = H;
    for (int l = 0; l < level; l++) Wr = (Wr + 1) / 2, Hr = (Hr + 1) / 2;
    dp->min_contour = (int)(p.min_size * std::max(Wr, Hr) * 4);   // :500-501, float arithmetic
    dp->max_contour = (int)(p.max_size * std::max(Wr, Hr) * 4);
    if (dp->max_contour > 16383) dp->max_contour = 16383;       // offsets inside a border are 14-bit fields
    int rect[4];
    border_rect(p.border_dist, W, H, rect);
    dp->bx0 = rect[0], dp->by0 = rect[1], dp->bx1 = rect[2], dp->by1 = rect[3];
    dp->subpix_win = (int)p.thres_param1;
    dp->locked = p.use_locked_corners != 0, dp->locked_wsize = (int)p.thres_param1;   // findCornerMaxima(Corners, grey, _thresParam1)
    dp->decoder = p.decoder_kind;
    if (p.decoder_kind == ARUCOHIP_DECODER_HRM) {
        const Dictionary& d = h->hrm;
        if (!h->d_hrm || d.count <= 0) return fail(h, ARUCOHIP_E_INVALID, "decoder HRM without a dictionary (arucohip_set_dictionary)");
        if (p.warp_size < 2 * (d.n + 2)) return fail(h, ARUCOHIP_E_INVALID, "warp size too small for the dictionary's markers");
        dp->hrm_n = d.n, dp->hrm_count = d.count, dp->hrm_codes = h->d_hrm;
        dp->hrm_correction = (uint32_t)(d.rate * (float)((d.tau0 - 1) / 2));   // highlyreliablemarkers.cpp:318
    }
    if (p.decoder_kind == ARUCOHIP_DECODER_USER && !h->decoder_fn)
        return fail(h, ARUCOHIP_E_INVALID, "decoder USER without a callback (arucohip_set_decoder_callback)");
    return ARUCOHIP_OK;
}

static int make_cam(arucohip_handle* h, const float* K, const float* dist, int ndist, float marker_size, int y_perp, CamModel* cam) {
    if (ndist < 0 || ndist > 8) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0..8");
    fill_cam(cam, K, dist, ndist, marker_size, y_perp);
    return ARUCOHIP_OK;
}

static int check_status(arucohip_handle* h, uint32_t st) {
    if (!st) return ARUCOHIP_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "device list overflow:%s%s%s%s%s%s", (st & ST_TRIG_OVERFLOW) ? " triggers" : "",
             (st & ST_CDESC_OVERFLOW) ? " contours" : "", (st & ST_POOL_OVERFLOW) ? " points" : "",
             (st & ST_QUAD_OVERFLOW) ? " quads" : "", (st & ST_CAND_OVERFLOW) ? " candidates" : "",
             (st & ST_MARKER_OVERFLOW) ? " markers" : "");
    if (st & ST_SEGMENT_ERROR) snprintf(msg + strlen(msg), sizeof(msg) - strlen(msg), " segment-link");
    h->err = msg;
    return ARUCOHIP_E_OVERFLOW;
}

// the pad word of every bit-image row must be zero; its position depends on the frame width. The same holds for the bitmap words of tile
// rows no threshold kernel writes (see create_handle)
static int ensure_bits_geometry(arucohip_handle* h, int W, int H) {
    if (h->bits_w == W && h->bits_h == H) return ARUCOHIP_OK;
    HIPCHK(h, hipMemsetAsync(h->buf.tiles, 0, h->bits_bytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->buf.tile_bits, 0, h->tile_bits_bytes, h->stream));
    h->bits_w = W, h->bits_h = H;
    return ARUCOHIP_OK;
}

// the long walks keep their checkpoint rings in HBM; (re)size the space for this batch
static int ensure_walk_scratch(arucohip_handle* h, int nplanes, const DetectParams& dp) {
    size_t need = walk_scratch_words(nplanes, dp, h->buf.long_cap);
    if (need > 0xFFFFFFF0ull) return fail(h, ARUCOHIP_E_CAPACITY, "batch too large for 32-bit checkpoint offsets: fewer frames per batch or a smaller max size");
    HIPCHK(h, h->walk_scratch.reserve(need * sizeof(uint32_t)));
    h->buf.walk_scratch = h->walk_scratch;
    return ARUCOHIP_OK;
}

// The pyramid of a batch: level l (1 .. levels) is w[l] x h[l]; the levels below the last one have rows padded to 8 bytes (pyr_down_kernel's
// 8-byte loads) and alternate between the two halves of d_pyr, the last one is tightly packed, in d_pyr or where the caller wants it.
struct PyrPlan {
    int levels = 0;
    int w[4] = {}, h[4] = {};
    size_t row[4] = {}, frame[4] = {}, off[4] = {};   // off: byte offset of level l in d_pyr
    size_t bytes = 0;
    FrameGeom reduced() const { return FrameGeom{w[levels], h[levels], row[levels], frame[levels]}; }
};
static PyrPlan plan_pyramid(const FrameGeom& g, int nframes, int levels) {
    PyrPlan p;
    p.levels = levels, p.w[0] = g.width, p.h[0] = g.height;
    size_t half[2] = {0, 0};
    for (int l = 1; l <= levels; l++) {
        p.w[l] = (p.w[l - 1] + 1) / 2, p.h[l] = (p.h[l - 1] + 1) / 2;
        p.row[l] = l == levels ? (size_t)p.w[l] : ((size_t)p.w[l] + 7) & ~(size_t)7;
        p.frame[l] = l == levels ? p.row[l] * p.h[l] : (p.row[l] * p.h[l] + 7) & ~(size_t)7;
        half[l & 1] = std::max(half[l & 1], ((size_t)nframes * p.frame[l] + 255) & ~(size_t)255);
    }
    for (int l = 1; l <= levels; l++) p.off[l] = (l & 1) ? 0 : half[1];
    p.bytes = half[0] + half[1];
    return p;
}
// level after level on stream s; the last one goes to `last` (the caller's device memory) or, when null, to its place in d_pyr (reserved by the caller)
static const uint8_t* run_pyramid(arucohip_handle* h, hipStream_t s, const uint8_t* src, const FrameGeom& g, int nframes, const PyrPlan& p, uint8_t* last) {
    const uint8_t* from = src;
    size_t row = g.row_stride, frame = g.frame_stride;
    for (int l = 1; l <= p.levels; l++) {
        uint8_t* to = (l == p.levels && last) ? last : h->d_pyr + p.off[l];
        launch_pyr_down(s, from, row, frame, p.w[l - 1], p.h[l - 1], nframes, to, p.row[l], p.frame[l]);
        from = to, row = p.row[l], frame = p.frame[l];
    }
    return from;
}

// Host-side work in front of a batch's enqueued work (detect_core), which a captured graph does not repeat: the eager path and every graph
// replay run it first. In steady state it only compares integers. g: the frames; with a pyramid level the walk scratch and the bit tiles are
// sized for the reduced image, which is also reserved here.
static int batch_prologue(arucohip_handle* h, const FrameGeom& g, int nframes, const DetectParams& dp) {
    int rc;
    if ((rc = ensure_walk_scratch(h, nframes * dp.nthr, dp))) return rc;
    FrameGeom gr = g;
    if (dp.pyr > 0) {
        const PyrPlan pp = plan_pyramid(g, nframes, dp.pyr);
        HIPCHK(h, h->d_pyr.reserve(pp.bytes));
        gr = pp.reduced();
    }
    if ((rc = ensure_bits_geometry(h, gr.width, gr.height))) return rc;
    // canonical patches of the decode stage: cap_flat * warp_size^2 bytes, for the configurations whose kernels store and read them
    if (!decode_from_cells(g, nframes, dp)) {
        HIPCHK(h, h->patches.reserve((size_t)h->buf.cap_flat * dp.warp_size * dp.warp_size));
        h->buf.patches = h->patches;
    }
    return ARUCOHIP_OK;
}

// Plugin boundary (markerdetector.h:65-78, :243-245): the caller's decoder runs on the host between the device's warp and
// the rest of the pipeline. Candidates are decoded frame by frame in detectRectangles order like the loop at
// markerdetector.cpp:350-368.
static int user_decode_stage(arucohip_handle* h, const DetectParams& dp) {
    hipStream_t s = h->stream;
    const Buffers& b = h->buf;
    // pinned staging owned by the handle, grown on demand: the steady state of a stream of calls allocates nothing
    const size_t npx = (size_t)dp.warp_size * dp.warp_size;
    HIPCHK(h, h->hu_list.reserve((size_t)b.cap_flat * (sizeof(uint32_t) + sizeof(int2) + sizeof(uint32_t)) + sizeof(uint32_t)));
    uint32_t* list = h->hu_list;                                   // [cap_flat] frame << 16 | index
    int2* dec = (int2*)(list + b.cap_flat);                        // [cap_flat] {id, nRotations}
    uint32_t* order = (uint32_t*)(dec + b.cap_flat);               // [cap_flat] + the candidate count behind it
    uint32_t* ncand_p = order + b.cap_flat;
    HIPCHK(h, hipMemcpyAsync(ncand_p, b.counters + CNT_NCAND, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const uint32_t n = std::min(*ncand_p, b.cap_flat);
    if (!n) return ARUCOHIP_OK;
    HIPCHK(h, h->hu_patches.reserve((size_t)n * npx + npx));
    uint8_t* patches = h->hu_patches;
    uint8_t* scratch = patches + (size_t)n * npx;
    HIPCHK(h, hipMemcpyAsync(list, b.cand_list, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(patches, b.patches, (size_t)n * npx, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order, order + n, [&](uint32_t x, uint32_t y) { return list[x] < list[y]; });   // frame << 16 | index
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = order[k];
        std::memcpy(scratch, patches + (size_t)i * npx, npx);
        int nrot = 0;   // the reference leaves it uninitialised (markerdetector.cpp:354); 0 is the intent
        const int id = h->decoder_fn(h->decoder_user, scratch, dp.warp_size, &nrot);
        dec[i] = make_int2(id < 0 ? -1 : id, nrot & 3);
    }
    HIPCHK(h, h->d_user_dec.reserve((size_t)b.cap_flat * sizeof(int2)));   // once per handle
    HIPCHK(h, hipMemcpyAsync(h->d_user_dec, dec, n * sizeof(int2), hipMemcpyHostToDevice, s));
    launch_set_decoded(s, b, n, h->d_user_dec);
    // no synchronise: the staging belongs to the handle, and the next call that touches it synchronises the stream first (the count above)
    return ARUCOHIP_OK;
}

// per-kernel timing on stream s: ev = the batch's events (h->ev), nullptr when timing is off
#define MARK(i) do { if (ev) (void)hipEventRecord(ev[i], s); } while (0)

// Rectangles stage on the planes' bit tiles: start candidates, border following, quads, frame candidates (detect_core, and without timing
// events arucohip_detect_rectangles)
static int run_rectangles(arucohip_handle* h, hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& dp, hipEvent_t* ev) {
    const Buffers& b = h->buf;
    if (b.seg_mode) {
        launch_start_candidates(s, g, nframes * dp.nthr, b);   // also clears the planes' key -> node tables
        MARK(K_WALKERS);
        launch_segments(s, g, nframes * dp.nthr, dp, b);
        MARK(K_WALKERS_LONG);
        MARK(K_CONTOUR_QUADS);
        launch_contour_quads(s, g, nframes, dp, b);
    } else {
        if (RUN_STAGE(b.env, 1)) launch_start_candidates(s, g, nframes * dp.nthr, b, dp.min_contour);
        MARK(K_WALKERS);
        // walkers; where the handle has a side stream their late generations run there under the first quad pass (the contour_quad mark sits at
        // the fork); a pipeline lane has none: its late walks run inside the launch of the first quad pass, on s, and a small pass takes their borders
        WalkFork fk{h->side_stream, h->ev_wfork, h->ev_wjoin, ev ? ev[K_WALKERS_LONG] : nullptr};
        const int tail = RUN_STAGE(b.env, 2) ? launch_walkers(s, fk, g, nframes * dp.nthr, dp, b) : WALKS_DONE;
        MARK(K_CONTOUR_QUADS);
        if (tail == WALKS_LATE) {
            launch_late_quads(s, g, nframes, dp, b);
        } else {
            if (RUN_STAGE(b.env, 4)) launch_contour_quads(s, g, nframes, dp, b, tail == WALKS_FORKED ? 1 : 0);
            if (tail == WALKS_FORKED) {
                HIPCHK(h, hipStreamWaitEvent(s, h->ev_wjoin, 0));
                if (RUN_STAGE(b.env, 4)) launch_contour_quads(s, g, nframes, dp, b, 2);
            }
        }
    }
    MARK(K_FRAME_CANDS);
    if (RUN_STAGE(b.env, 5)) launch_frame_candidates(s, g, nframes, dp, b);
    return ARUCOHIP_OK;
}

// threshold stage of any method into buf.thres / buf.tiles (+ bitmap). CANNY (markerdetector.cpp:667-676) blocks the host while its
// hysteresis converges.
// want_bytes: the caller reads buf.thres right away (stage entry point, erosion); otherwise the byte image may be left as tiles + border
// lines (h->thres_bytes says which) and arucohip_get_thresholded expands the plane it is asked for.
static int run_threshold(arucohip_handle* h, hipStream_t s, const uint8_t* gray_dev, const FrameGeom& g, int nframes, const DetectParams& dp, bool want_bytes) {
    const Buffers& b = h->buf;
    h->thres_bytes = true;
    h->thr_plan_planes = 0;
    if (dp.thres_method != ARUCOHIP_THRES_CANNY) {
        const bool lazy = launch_threshold(s, gray_dev, g, nframes, dp, b, b.env.thres_lazy && !want_bytes, &h->thr_plan_done);
        h->thres_bytes = !lazy, h->thr_plan_planes = dp.nthr;
        return ARUCOHIP_OK;
    }
    const size_t ntiles = (size_t)nframes * dp.nthr * ((g.width + 7) / 8) * ((g.height + 7) / 8);
    HIPCHK(h, h->d_canny.reserve(2 * ntiles * sizeof(uint64_t) + 64));
    uint64_t* surv = h->d_canny;
    uint64_t* edge = surv + ntiles;
    if (launch_canny(s, gray_dev, g, nframes, dp.nthr, b, surv, edge, (uint32_t*)(edge + ntiles))) return fail(h, ARUCOHIP_E_HIP, "CANNY kernels failed");
    FrameGeom tg = g;
    tg.row_stride = (size_t)g.width, tg.frame_stride = (size_t)g.width * g.height;
    launch_binary_planes(s, b.thres, tg, nframes * dp.nthr, b);   // contour tiles + bitmap from the edge image
    return ARUCOHIP_OK;
}

// gf: the frames at gray_dev. With a pyramid level (dp.pyr > 0) threshold, erosion and the rectangle stage work on the reduced frames (gr, in
// d_pyr, reserved by batch_prologue); what they found is lifted to full-frame coordinates, and decoding, corner refinement and the border filter
// work on the frames themselves.
static int detect_core(arucohip_handle* h, const uint8_t* gray_dev, const FrameGeom& gf, int nframes, const DetectParams& dp, const CamModel& cam) {
    hipStream_t s = h->stream;
    Buffers& b = h->buf;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    hipEvent_t* ev = h->timing ? h->ev[h->tsets % TSETS] : nullptr;
    MARK(K_THRESHOLD);
    FrameGeom g = gf;   // of the rectangle stage
    const uint8_t* small_dev = gray_dev;
    if (dp.pyr > 0) {
        const PyrPlan pp = plan_pyramid(gf, nframes, dp.pyr);
        small_dev = run_pyramid(h, s, gray_dev, gf, nframes, pp, nullptr);
        g = pp.reduced();
    }
    {
        const int rc_ = run_threshold(h, s, small_dev, g, nframes, dp, false);
        if (rc_) return rc_;
    }
    if (h->params.erode) {
        // on the bit tiles where the byte image was left out (the default path), on the bytes otherwise
        const bool on_tiles = !h->thres_bytes;
        HIPCHK(h, h->d_erode.reserve(on_tiles ? erode_tiles_tmp_bytes(g, nframes * dp.nthr) : (size_t)nframes * dp.nthr * g.width * g.height));
        if (on_tiles)
            launch_erode_tiles(s, g, nframes * dp.nthr, b, h->d_erode);
        else
            launch_erode(s, g, nframes * dp.nthr, b, h->d_erode);
    }
    MARK(K_FILTER);
    {
        const int rc_ = run_rectangles(h, s, g, nframes, dp, ev);
        if (rc_) return rc_;
    }
    if (dp.pyr > 0) launch_lift(s, nframes, dp, b);
    MARK(K_DECODE);
    // built-in 5x5 decoder: a batch decodes from cell medians inside launch_decode; on a stored patch (one frame per call, other warp sizes) the cell
    // votes and the Hamming decode of a candidate are the head of its refinement wave (one dispatch less)
    h->cells_valid = decode_from_cells(gf, nframes, dp);
    const bool fused_cells = dp.decoder == ARUCOHIP_DECODER_FIDUCIAL_5X5 && !h->cells_valid;
    if (RUN_STAGE(b.env, 6)) launch_decode(s, gray_dev, gf, nframes, dp, b, fused_cells);
    if (dp.decoder == ARUCOHIP_DECODER_USER) {
        const int rc_ = user_decode_stage(h, dp);
        if (rc_) return rc_;
    }
    MARK(K_REFINE_LINES);
    if (RUN_STAGE(b.env, 7)) launch_refine_lines(s, gf, nframes, dp, cam, b, fused_cells);
    MARK(K_REFINE_PIXELS);
    if (dp.corner_method == ARUCOHIP_CORNER_HARRIS || dp.corner_method == ARUCOHIP_CORNER_SUBPIX) {
        if (dp.locked) launch_locked_corners(s, gray_dev, gf, nframes, dp, b);   // markerdetector.cpp:398-399
        launch_refine_pixels(s, gray_dev, gf, nframes, dp, b);
    }
    MARK(K_FINALIZE);
    if (RUN_STAGE(b.env, 8)) launch_finalize(s, gf, nframes, dp, cam, b, h->wt_out, h->wt_cap, h->wt_n);
    MARK(K_POSE);
    if (RUN_STAGE(b.env, 8) && cam.has_K && cam.marker_size > 0) launch_pose(s, nframes, cam, b);
    MARK(K_COUNT);
#undef MARK
    if (ev) h->tsets++;
    HIPCHK(h, hipGetLastError());
    return ARUCOHIP_OK;
}

// channels = 1: gray frames (device frames are used in place); channels = 3: B,G,R interleaved, converted into d_gray
static int stage_frames(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                        int on_device, int channels, const uint8_t** gray_dev, FrameGeom* g) {
    g->width = W, g->height = H;
    if (channels == 3) {
        const uint8_t* bgr = frames;
        size_t rs = row_stride, fs = frame_stride;
        if (!on_device) {
            HIPCHK(h, h->d_bgr.reserve((size_t)nframes * W * H * 3));
            for (int f = 0; f < nframes; f++)
                HIPCHK(h, hipMemcpy2DAsync(h->d_bgr + (size_t)f * W * H * 3, (size_t)W * 3, frames + (size_t)f * frame_stride, row_stride, (size_t)W * 3, H,
                                           hipMemcpyHostToDevice, h->stream));
            bgr = h->d_bgr, rs = (size_t)W * 3, fs = (size_t)W * H * 3;
        }
        HIPCHK(h, h->d_gray.reserve((size_t)nframes * W * H));
        launch_bgr2gray(h->stream, bgr, rs, fs, W, H, nframes, h->d_gray);
        HIPCHK(h, hipGetLastError());
        *gray_dev = h->d_gray;
        g->row_stride = W, g->frame_stride = (size_t)W * H;
        return ARUCOHIP_OK;
    }
    if (on_device) {
        *gray_dev = frames;
        g->row_stride = row_stride, g->frame_stride = frame_stride;
        return ARUCOHIP_OK;
    }
    HIPCHK(h, h->d_gray.reserve((size_t)nframes * W * H));
    if (row_stride == (size_t)W && frame_stride == (size_t)W * H) {
        // tightly packed frames (a pinned ring of camera frames): ONE copy for the batch instead of one 2-D copy per frame
        HIPCHK(h, hipMemcpyAsync(h->d_gray, frames, (size_t)nframes * W * H, hipMemcpyHostToDevice, h->stream));
    } else {
        for (int f = 0; f < nframes; f++)
            HIPCHK(h, hipMemcpy2DAsync(h->d_gray + (size_t)f * W * H, W, frames + (size_t)f * frame_stride, row_stride, W, H,
                                       hipMemcpyHostToDevice, h->stream));
    }
    *gray_dev = h->d_gray;
    g->row_stride = W, g->frame_stride = (size_t)W * H;
    return ARUCOHIP_OK;
}

static int check_geometry(arucohip_handle* h, int nframes, int W, int H, size_t row_stride, int channels = 1) {
    if (nframes < 1 || nframes > h->lim.max_batch) return fail(h, ARUCOHIP_E_INVALID, "nframes outside 1..max_batch");
    // every device array and packed field is sized per dimension (tile rows, 14-bit checkpoint coordinates, raster keys)
    if (W < 1 || H < 1 || W > h->lim.max_width || H > h->lim.max_height) return fail(h, ARUCOHIP_E_INVALID, "frame wider or taller than the handle was created for");
    if (row_stride < (size_t)W * channels) return fail(h, ARUCOHIP_E_INVALID, "row_stride < width * channels");
    return ARUCOHIP_OK;
}

// enqueue one chunk on worker w (its buffers, its stream); results go to device memory or to w's pinned staging
static int chunk_enqueue(arucohip_handle* w, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                         int frames_on_device, int channels, const DetectParams& dp, const CamModel& cam, arucohip_marker_t* out, int cap, int32_t* n_out,
                         int out_on_device) {
    int rc;
    const uint8_t* gray_dev;
    FrameGeom g;
    if ((rc = stage_frames(w, frames, nframes, W, H, row_stride, frame_stride, frames_on_device, channels, &gray_dev, &g))) return rc;
    if ((rc = batch_prologue(w, g, nframes, dp))) return rc;
    // results for device memory without poses: finalize_kernel stores them there itself
    const bool write_through = out_on_device && !(cam.has_K && cam.marker_size > 0) && cap > 0;
    w->wt_out = write_through ? out : nullptr, w->wt_cap = write_through ? cap : 0, w->wt_n = write_through ? n_out : nullptr;
    rc = detect_core(w, gray_dev, g, nframes, dp, cam);
    w->wt_out = nullptr, w->wt_cap = 0, w->wt_n = nullptr;
    if (rc) return rc;
    if (write_through) return ARUCOHIP_OK;
    const Buffers& b = w->buf;
    const int ncopy = std::min(cap, b.cap_markers);
    if (out_on_device) {
        if (ncopy > 0)
            HIPCHK(w, hipMemcpy2DAsync(out, (size_t)cap * sizeof(arucohip_marker_t), b.markers, (size_t)b.cap_markers * sizeof(arucohip_marker_t),
                                       (size_t)ncopy * sizeof(arucohip_marker_t), nframes, hipMemcpyDeviceToDevice, w->stream));
        HIPCHK(w, hipMemcpyAsync(n_out, b.nmarkers, nframes * sizeof(int32_t), hipMemcpyDeviceToDevice, w->stream));
        return ARUCOHIP_OK;
    }
    HIPCHK(w, hipMemcpyAsync(w->h_markers, b.markers, (size_t)nframes * b.cap_markers * sizeof(arucohip_marker_t), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipMemcpyAsync(w->h_n, b.nmarkers, nframes * sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(w, hipMemcpyAsync(w->h_counters, b.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    return ARUCOHIP_OK;
}

// after the worker's stream has drained: copy the chunk's markers from the pinned staging to the caller's arrays; a device list that
// overflowed is reported ahead of an output array that is too small
static int chunk_collect_host(arucohip_handle* h, const Span& s, arucohip_marker_t* out, int cap, int32_t* n_out) {
    const int fits = collect_markers(h, s, cap, out, n_out, s.w->h_markers, s.w->h_n);
    const int st = check_status(h, s.w->h_counters[CNT_STATUS] & ~(uint32_t)ST_MARKER_OVERFLOW);
    return st ? st : fits;
}

int fork_workers(arucohip_handle* h, const Batch& b) {
    if (b.nspan <= 1) return ARUCOHIP_OK;
    arucohip_handle* o = b.span[0].w;
    HIPCHK(h, hipEventRecord(o->ev_fork, o->stream));
    for (int c = 1; c < b.nspan; c++) HIPCHK(h, hipStreamWaitEvent(b.span[c].w->stream, o->ev_fork, 0));
    return ARUCOHIP_OK;
}
int join_workers(arucohip_handle* h, const Batch& b) {
    arucohip_handle* o = b.span[0].w;
    for (int c = 1; c < b.nspan; c++) {
        HIPCHK(h, hipEventRecord(o->ev_join[c - 1], b.span[c].w->stream));
        HIPCHK(h, hipStreamWaitEvent(o->stream, o->ev_join[c - 1], 0));
    }
    return ARUCOHIP_OK;
}

// h's last batch has been enqueued on h's stream: wait for it and copy every chunk's markers from the pinned staging to the caller
static int collect_batch_host(arucohip_handle* h, arucohip_marker_t* out, int cap, int32_t* n_out) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int ret = ARUCOHIP_OK;
    for (const Span& s : h->last) {
        int r = chunk_collect_host(h, s, out, cap, n_out);
        if (ret == ARUCOHIP_OK) ret = r;
    }
    return ret;
}

// FNV-1a over the bytes of everything a captured launch carries by value
static uint64_t digest(uint64_t hsh, const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) hsh = (hsh ^ c[i]) * 1099511628211ull;
    return hsh;
}

// arucohip_detect on one host frame through a captured graph. *handled = false: the caller takes the eager path (first call of a
// configuration or after a buffer was replaced, timing on, a decoder or threshold method that blocks the host, a failed capture). The frame's
// copy to the device and batch_prologue are issued eagerly in front of the graph; inside it: the counters' memset, every kernel of detect_core
// (with the fork to the side stream of the late walker generations) and the copy of the results into the handle's pinned staging.
static int detect_one_graphed(arucohip_handle* h, const uint8_t* frame, int W, int H, size_t row_stride, int channels, const DetectParams& dp, const CamModel& cam,
                              arucohip_marker_t* out, int cap, int32_t* n_out, bool* handled) {
    *handled = false;
    if (h->fgraph.disabled || h->timing || dp.decoder == ARUCOHIP_DECODER_USER || dp.thres_method == ARUCOHIP_THRES_CANNY || h->params.erode || dp.pyr > 0) return ARUCOHIP_OK;
    uint64_t key = 1469598103934665603ull;
    const int geo[5] = {W, H, channels, (int)h->buf.seg_mode, h->buf.thr_stamp_on};
    key = digest(key, geo, sizeof(geo));
    key = digest(key, &dp, sizeof(dp));
    key = digest(key, &cam, sizeof(cam));
    key = digest(key, &h->stream, sizeof(h->stream));
    if (h->fgraph.exec && h->fgraph.key != key) {   // another configuration: start over
        (void)hipGraphExecDestroy(h->fgraph.exec);
        h->fgraph.exec = nullptr, h->fgraph.seen = 0;
    }
    if (!h->fgraph.exec && h->fgraph.seen != key) {   // first call with this configuration: eager (it sizes every buffer), remember it
        h->fgraph.seen = key;
        return ARUCOHIP_OK;
    }
    int rc;
    const uint8_t* gray_dev;
    FrameGeom g;
    if ((rc = stage_frames(h, frame, 1, W, H, row_stride, (size_t)H * row_stride, 0, channels, &gray_dev, &g))) return rc;   // H2D (+ BGR conversion), eager
    if ((rc = batch_prologue(h, g, 1, dp))) return rc;   // also restores the bit-image geometry on the stream, ahead of the launch
    const std::array<const void*, 3> addrs = {gray_dev, h->buf.walk_scratch, h->buf.patches};   // what may move between calls (FrameGraph)
    if (h->fgraph.exec && h->fgraph.addrs != addrs) {   // a buffer was replaced since the capture: start over, like a new configuration
        (void)hipGraphExecDestroy(h->fgraph.exec);
        h->fgraph.exec = nullptr, h->fgraph.seen = key;
        return ARUCOHIP_OK;   // the frame is staged; the eager path stages it again, which is harmless
    }
    if (!h->fgraph.exec) {
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            h->fgraph.disabled = 1;
            return ARUCOHIP_OK;   // the frame is staged; the eager path stages it again, which is harmless
        }
        rc = detect_core(h, gray_dev, g, 1, dp, cam);
        const Buffers& b = h->buf;
        hipError_t e = hipSuccess;
        if (rc == ARUCOHIP_OK) {
            // ONE copy: the markers and, in the slot behind them, the count and the status word finalize_kernel left there
            e = hipMemcpyAsync(h->h_markers, b.markers, ((size_t)b.cap_markers + 1) * sizeof(arucohip_marker_t), hipMemcpyDeviceToHost, h->stream);
        }
        const hipError_t e2 = hipStreamEndCapture(h->stream, &graph);
        const std::array<const void*, 3> captured = {gray_dev, h->buf.walk_scratch, h->buf.patches};
        if (rc != ARUCOHIP_OK || e != hipSuccess || e2 != hipSuccess || !graph || captured != addrs ||
            hipGraphInstantiate(&h->fgraph.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (graph) (void)hipGraphDestroy(graph);
            h->fgraph.exec = nullptr, h->fgraph.disabled = 1;   // this handle stays on the eager path
            return ARUCOHIP_OK;
        }
        (void)hipGraphDestroy(graph);
        h->fgraph.key = key, h->fgraph.addrs = addrs, h->fgraph.thres_bytes = h->thres_bytes;
        h->fgraph.thr_plan = h->thr_plan_done, h->fgraph.thr_plan_planes = h->thr_plan_planes;
    }
    *handled = true;
    HIPCHK(h, hipGraphLaunch(h->fgraph.exec, h->stream));
    h->thres_bytes = h->fgraph.thres_bytes;
    h->thr_plan_done = h->fgraph.thr_plan, h->thr_plan_planes = h->fgraph.thr_plan_planes;
    h->cells_valid = false;   // one frame per call stores the patch
    h->last = plan_batch(h, 1, W, H, dp.nthr);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int32_t* hdr = (const int32_t*)(h->h_markers + h->buf.cap_markers);
    h->h_n[0] = hdr[0], h->h_counters[CNT_STATUS] = (uint32_t)hdr[1];
    return collect_batch_host(h, out, cap, n_out);
}

static int detect_batch_impl(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                             int frames_on_device, int channels, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                             arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device, bool defer = false) {
    if (!h || !frames || !n_out || (cap > 0 && !out) || cap < 0) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, nframes, W, H, row_stride, channels);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DetectParams dp;
    CamModel cam;
    if ((rc = make_detect_params(h, W, H, &dp, h->pyr))) return rc;
    if ((rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam))) return rc;
    if (nframes == 1 && !frames_on_device && !out_on_device && !defer && h->nsub == 1) {
        bool handled = false;
        rc = detect_one_graphed(h, frames, W, H, row_stride, channels, dp, cam, out, cap, n_out, &handled);
        if (handled) return rc;
    }
    h->last = plan_batch(h, nframes, W, H, dp.nthr);
    for (int l = 0; l < dp.pyr; l++) h->last.W = (h->last.W + 1) / 2, h->last.H = (h->last.H + 1) / 2;   // of the thresholded image
    const Batch& plan = h->last;
    if ((rc = fork_workers(h, plan))) return rc;
    for (int c = 0; c < plan.nspan; c++) {
        const Span& s = plan.span[c];
        rc = chunk_enqueue(s.w, frames + (size_t)s.first * frame_stride, s.count, W, H, row_stride, frame_stride, frames_on_device, channels, dp, cam,
                           out ? out + (size_t)s.first * cap : nullptr, cap, n_out + s.first, out_on_device);
        if (rc) {
            if (s.w != h) h->err = s.w->err;
            // the workers that already have queued work still have to rejoin the caller's stream
            const std::string keep = h->err;
            (void)join_workers(h, plan);
            h->err = keep;
            h->last = Batch{};   // the lists hold part of a batch
            return rc;
        }
    }
    if ((rc = join_workers(h, plan))) return rc;
    if (out_on_device || defer) return ARUCOHIP_OK;
    return collect_batch_host(h, out, cap, n_out);
}

extern "C" {

int arucohip_detect_batch(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                          int frames_on_device, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                          arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device) {
    return detect_batch_impl(h, frames, nframes, W, H, row_stride, frame_stride, frames_on_device, 1, K, dist, ndist, marker_size, y_perp, out, cap,
                             n_out, out_on_device);
}

int arucohip_detect_batch_bgr(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                              int frames_on_device, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                              arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device) {
    return detect_batch_impl(h, frames, nframes, W, H, row_stride, frame_stride, frames_on_device, 3, K, dist, ndist, marker_size, y_perp, out, cap,
                             n_out, out_on_device);
}

int arucohip_detect_bgr(arucohip_handle* h, const uint8_t* bgr, int W, int H, size_t row_stride, const float* K, const float* dist, int ndist,
                        float marker_size, int y_perp, arucohip_marker_t* out, int cap, int* n_out) {
    int32_t n = 0;
    int rc = arucohip_detect_batch_bgr(h, bgr, 1, W, H, row_stride, (size_t)H * row_stride, 0, K, dist, ndist, marker_size, y_perp, out, cap, &n, 0);
    if (n_out) *n_out = n;
    return rc;
}

int arucohip_bgr_to_gray(arucohip_handle* h, const uint8_t* bgr, int W, int H, size_t row_stride, uint8_t* gray) {
    if (!h || !bgr || !gray) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, 1, W, H, row_stride, 3);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const uint8_t* dev;
    FrameGeom g;
    if ((rc = stage_frames(h, bgr, 1, W, H, row_stride, (size_t)H * row_stride, 0, 3, &dev, &g))) return rc;
    HIPCHK(h, hipMemcpyAsync(gray, dev, (size_t)W * H, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

// cv::undistort(src, dst, K, dist) as the reference's GL apps call it before detect()
// (utils/aruco_test_gl.cpp:237-240, utils/aruco_test_board_gl.cpp:265-268)
int arucohip_undistort(arucohip_handle* h, const uint8_t* src, int nframes, int W, int H, size_t row_stride, size_t frame_stride, int channels,
                       int src_on_device, const float* K, const float* dist, int ndist, uint8_t* dst, int dst_on_device) {
    if (!h || !src || !dst || !K || (channels != 1 && channels != 3) || ndist < 0 || ndist > 8 || (ndist > 0 && !dist)) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, nframes, W, H, row_stride, channels);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // map of this camera: recomputed only when size, K or dist change
    bool same = h->umap_w == W && h->umap_h == H && h->umap_nd == ndist && std::memcmp(h->umap_K, K, sizeof(h->umap_K)) == 0 &&
                (ndist == 0 || std::memcmp(h->umap_d, dist, ndist * sizeof(float)) == 0);
    if (!same) {
        const size_t px = (size_t)W * H;
        h->umap_nd = -1;   // no valid map until this one is written
        HIPCHK(h, h->d_umap_xy.reserve(px * sizeof(short2)));
        HIPCHK(h, h->d_umap_f.reserve(px * sizeof(uint16_t)));
        launch_undist_map(s, W, H, K, dist, ndist, h->d_umap_xy, h->d_umap_f);
        HIPCHK(h, hipGetLastError());
        h->umap_w = W, h->umap_h = H, h->umap_nd = ndist;
        std::memcpy(h->umap_K, K, sizeof(h->umap_K));
        if (ndist) std::memcpy(h->umap_d, dist, ndist * sizeof(float));
    }
    // host frames and the packed result a host caller gets are staged in the arena
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
    launch_remap(s, sdev.p, sdev.row, sdev.frame, W, H, channels, nframes, h->d_umap_xy, h->d_umap_f, ddev.p);
    HIPCHK(h, hipGetLastError());
    if ((rc = unstage(h, s, out, ddev))) return rc;
    if (!dst_on_device) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

// MarkerDetector::pyrDown(level): the level is a property of the whole tree of workers, like the parameters
int arucohip_set_pyr_down(arucohip_handle* h, int level) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (level < 0 || level > 3) return fail(h, ARUCOHIP_E_INVALID, "pyrDown: level outside 0..3");
    for (auto* l : h->lanes)
        if (l->pend.active) return fail(h, ARUCOHIP_E_INVALID, "a submitted batch has not been waited for");
    for_each_worker(h, [&](arucohip_handle* w) { w->pyr = level; return ARUCOHIP_OK; });
    drop_retry(h);
    return ARUCOHIP_OK;
}

int arucohip_get_pyr_down(const arucohip_handle* h) { return h ? h->pyr : 0; }

int arucohip_pyr_down(arucohip_handle* h, const uint8_t* src, int nframes, int W, int H, size_t row_stride, size_t frame_stride, int src_on_device,
                      int levels, uint8_t* dst, int dst_on_device) {
    if (!h || !src || !dst) return ARUCOHIP_E_INVALID;
    if (levels < 1 || levels > 3) return fail(h, ARUCOHIP_E_INVALID, "pyr_down: levels outside 1..3");
    int rc = check_geometry(h, nframes, W, H, row_stride);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const uint8_t* sdev;
    FrameGeom g;
    if ((rc = stage_frames(h, src, nframes, W, H, row_stride, frame_stride, src_on_device, 1, &sdev, &g))) return rc;
    const PyrPlan pp = plan_pyramid(g, nframes, levels);
    HIPCHK(h, h->d_pyr.reserve(pp.bytes));
    const uint8_t* out = run_pyramid(h, s, sdev, g, nframes, pp, dst_on_device ? dst : nullptr);
    HIPCHK(h, hipGetLastError());
    if (!dst_on_device) {
        HIPCHK(h, hipMemcpyAsync(dst, out, (size_t)nframes * pp.frame[levels], hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    return ARUCOHIP_OK;
}

int arucohip_set_dictionary(arucohip_handle* h, int n, int count, const uint64_t* codes, int tau0, float correction_rate) {
    if (!h) return ARUCOHIP_E_INVALID;
    Dictionary d;
    if (count > 0) {
        if (!codes || n < 2 || n > 8 || count > 4096) return fail(h, ARUCOHIP_E_UNSUPPORTED, "dictionary: 2 <= n <= 8, count <= 4096");
        d.n = n, d.count = count, d.tau0 = tau0, d.rate = correction_rate, d.codes.assign(codes, codes + count);
    }
    drop_retry(h);
    HIPCHK(h, hipSetDevice(h->device));
    return for_each_worker(h, [&](arucohip_handle* w) { return load_dictionary(h, w, d); });
}

int arucohip_set_decoder_callback(arucohip_handle* h, arucohip_decoder_fn fn, void* user) {
    if (!h) return ARUCOHIP_E_INVALID;
    drop_retry(h);
    for_each_worker(h, [&](arucohip_handle* w) {
        w->decoder_fn = fn, w->decoder_user = user;
        if (!fn && w->params.decoder_kind == ARUCOHIP_DECODER_USER) w->params.decoder_kind = ARUCOHIP_DECODER_FIDUCIAL_5X5;
        return ARUCOHIP_OK;
    });
    return ARUCOHIP_OK;
}

int arucohip_batch_status(arucohip_handle* h) {
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t st = 0;
    for (const Span& s : h->last) {
        arucohip_handle* w = s.w;
        HIPCHK(h, hipMemcpyAsync(w->h_counters, w->buf.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipStreamSynchronize(w->stream));
        st |= w->h_counters[CNT_STATUS];
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_status(h, st);
}

int arucohip_batch_chunks(arucohip_handle* h, int* frames_per_chunk) {
    if (!h) return 0;
    if (frames_per_chunk) *frames_per_chunk = h->last.nspan ? h->last.span[0].count : 0;
    return std::max(h->last.nspan, 1);
}

int arucohip_detect(arucohip_handle* h, const uint8_t* gray, int W, int H, size_t row_stride, const float* K, const float* dist, int ndist,
                    float marker_size, int y_perp, arucohip_marker_t* out, int cap, int* n_out) {
    int32_t n = 0;
    int rc = arucohip_detect_batch(h, gray, 1, W, H, row_stride, (size_t)H * row_stride, 0, K, dist, ndist, marker_size, y_perp, out, cap, &n, 0);
    if (n_out) *n_out = n;
    return rc;
}

int arucohip_debug_threshold_plane(arucohip_handle* h0, int frame, int t, uint8_t* bytes, uint64_t* tiles, uint64_t* tile_bits) {
    if (!h0) return ARUCOHIP_E_INVALID;
    const Batch& r = h0->last;
    arucohip_handle* h = r.holder(frame, &frame);
    if (!h || t < 0 || t >= r.nthr) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t px = (size_t)r.W * r.H;
    const size_t plane = (size_t)frame * r.nthr + t;
    if (bytes) {
        if (!h->thres_bytes) {   // the batch kept the image as tiles + border lines: rebuild this plane's bytes
            FrameGeom g;
            g.width = r.W, g.height = r.H, g.row_stride = (size_t)r.W, g.frame_stride = px;
            launch_expand_thres(h->stream, g, (int)plane, h->buf);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, hipMemcpyAsync(bytes, h->buf.thres + plane * px, px, hipMemcpyDeviceToHost, h->stream));
    }
    const size_t ntiles = (size_t)tiles_x(r.W) * tiles_y(r.H), nwords = (size_t)tiles_y(r.H) * 2 * tile_strips(r.W);
    if (tiles) HIPCHK(h, hipMemcpyAsync(tiles, h->buf.tiles + plane * ntiles, ntiles * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (tile_bits) HIPCHK(h, hipMemcpyAsync(tile_bits, h->buf.tile_bits + plane * nwords, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_get_thresholded(arucohip_handle* h, int frame, uint8_t* dst) {
    if (!h || !dst) return ARUCOHIP_E_INVALID;
    return arucohip_debug_threshold_plane(h, frame, h->last.nthr / 2, dst, nullptr, nullptr);   // thres = thres_images[n_param1 / 2]
}

int arucohip_debug_threshold_plan(arucohip_handle* h, int32_t* out, int cap, int* nplanes) {
    if (!h || !nplanes || (cap > 0 && !out) || cap < 0) return ARUCOHIP_E_INVALID;
    const arucohip_handle* w = h->last.nspan > 0 ? h->last.span[0].w : h;
    const int n = w->thr_plan_planes;
    *nplanes = n;
    if (n <= 0) return fail(h, ARUCOHIP_E_INVALID, "no threshold launch to report");
    if (cap < 5 * n + 3) return fail(h, ARUCOHIP_E_CAPACITY, "threshold plan: 5 words per plane and 3 behind them");
    const ThrPlan& pl = w->thr_plan_done;
    for (int t = 0; t < n; t++) {
        const ThrPlanePlan& q = pl.plane[t];
        int32_t* o = out + 5 * t;
        o[0] = (int32_t)q.family, o[1] = q.R, o[2] = q.p16, o[3] = q.fast, o[4] = q.seg;
    }
    out[5 * n] = pl.strips, out[5 * n + 1] = pl.no_bytes, out[5 * n + 2] = pl.bitmap_pass;
    return ARUCOHIP_OK;
}

int arucohip_debug_threshold_batch(arucohip_handle* h, const uint8_t* gray, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                                   int frames_on_device, int want_bytes) {
    if (!h || !gray) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, nframes, W, H, row_stride);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DetectParams dp;
    if ((rc = make_detect_params(h, W, H, &dp))) return rc;
    h->last = plan_batch(h, nframes, W, H, dp.nthr);
    const Batch& plan = h->last;
    if ((rc = fork_workers(h, plan))) return rc;
    for (const Span& s : plan) {
        const uint8_t* gray_dev;
        FrameGeom g;
        rc = stage_frames(s.w, gray + (size_t)s.first * frame_stride, s.count, W, H, row_stride, frame_stride, frames_on_device, 1, &gray_dev, &g);
        s.w->cells_valid = false;   // the cell medians belong to the batch this one replaces
        if (!rc) rc = ensure_bits_geometry(s.w, W, H);
        if (!rc) rc = run_threshold(s.w, s.w->stream, gray_dev, g, s.count, dp, want_bytes != 0);
        if (!rc && hipGetLastError() != hipSuccess) rc = fail(s.w, ARUCOHIP_E_HIP, "threshold launch failed");
        if (rc) {
            const std::string keep = s.w->err;
            (void)join_workers(h, plan);
            h->err = keep;
            h->last = Batch{};   // the planes hold part of a batch
            return rc;
        }
    }
    if ((rc = join_workers(h, plan))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

static int fetch_cands(arucohip_handle* h0, int frame, std::vector<Cand>* v) {
    if (!h0) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = h0->last.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    int32_t n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, h->buf.ncands + frame, sizeof(n), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    v->resize(std::max(n, 0));
    if (n > 0) {
        HIPCHK(h, hipMemcpyAsync(v->data(), h->buf.cands + (size_t)frame * h->buf.cap_cands, n * sizeof(Cand), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return ARUCOHIP_OK;
}

int arucohip_get_candidates(arucohip_handle* h, int frame, float* quads, int cap, int* n) {
    std::vector<Cand> v;
    int rc = fetch_cands(h, frame, &v);
    if (rc) return rc;
    int k = 0;
    for (auto& c : v) {
        if (c.id != -1) continue;
        if (k < cap)
            for (int i = 0; i < 8; i++) quads[k * 8 + i] = c.c[i];
        k++;
    }
    if (n) *n = k;
    return k > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

// Otsu threshold of every candidate of a frame (candidate order of arucohip_debug_candidates): what otsu_kernel left in the flat list's threshold slots
int arucohip_debug_otsu(arucohip_handle* h0, int frame, int32_t* thr, int cap, int* n) {
    if (!h0 || !thr || !n) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = h0->last.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t cnt[CNT_FIXED];
    int32_t nc = 0;
    HIPCHK(h, hipMemcpyAsync(cnt, h->buf.counters, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&nc, h->buf.ncands + frame, sizeof(nc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t nflat = std::min(cnt[CNT_NCAND], h->buf.cap_flat);
    std::vector<uint32_t> list(nflat);
    std::vector<int32_t> othr(nflat);
    if (nflat) {
        HIPCHK(h, hipMemcpyAsync(list.data(), h->buf.cand_list, nflat * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(othr.data(), h->buf.othr, nflat * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *n = std::max(nc, 0);
    for (int i = 0; i < std::min(*n, cap); i++) thr[i] = -1;
    for (uint32_t i = 0; i < nflat; i++)
        if ((int)(list[i] >> 16) == frame && (int)(list[i] & 0xFFFFu) < cap) thr[list[i] & 0xFFFFu] = othr[i];
    return *n > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

// Cell medians of every candidate of a frame (same order): what warp_hist_kernel<ROWS, true> left for otsu_kernel<true> in the last batch
int arucohip_debug_cells(arucohip_handle* h0, int frame, uint8_t* cells49, int cap, int* n) {
    if (!h0 || !cells49 || !n) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = h0->last.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    if (!h->cells_valid) return fail(h, ARUCOHIP_E_INVALID, "the last batch did not decode from cell medians");
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t cnt[CNT_FIXED];
    int32_t nc = 0;
    HIPCHK(h, hipMemcpyAsync(cnt, h->buf.counters, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&nc, h->buf.ncands + frame, sizeof(nc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint32_t nflat = std::min(cnt[CNT_NCAND], h->buf.cap_flat);
    std::vector<uint32_t> list(nflat);
    std::vector<uint8_t> cells((size_t)nflat * 64);
    if (nflat) {
        HIPCHK(h, hipMemcpyAsync(list.data(), h->buf.cand_list, nflat * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(cells.data(), h->buf.cells, cells.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *n = std::max(nc, 0);
    for (uint32_t i = 0; i < nflat; i++) {
        const int ci = (int)(list[i] & 0xFFFFu);
        if ((int)(list[i] >> 16) != frame || ci >= cap) continue;
        for (int cy = 0; cy < 7; cy++)
            for (int cx = 0; cx < 7; cx++) cells49[(size_t)ci * 49 + cy * 7 + cx] = cells[(size_t)i * 64 + cy * 8 + cx];
    }
    return *n > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

int arucohip_debug_candidates(arucohip_handle* h, int frame, float* quads0, int32_t* ids, int32_t* nrot, int cap, int* n) {
    std::vector<Cand> v;
    int rc = fetch_cands(h, frame, &v);
    if (rc) return rc;
    int k = 0;
    for (auto& c : v) {
        if (k < cap) {
            for (int i = 0; i < 4; i++) quads0[k * 8 + 2 * i] = c.qx[i], quads0[k * 8 + 2 * i + 1] = c.qy[i];
            if (ids) ids[k] = c.id;
            if (nrot) nrot[k] = c.nrot;
        }
        k++;
    }
    if (n) *n = k;
    return k > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

// contours of one frame in reference (RETR_LIST) order: planes ascending, raster key descending
static int fetch_contours(arucohip_handle* h0, int frame, std::vector<ContourDesc>* out, arucohip_handle** owner = nullptr) {
    if (!h0) return ARUCOHIP_E_INVALID;
    const int nthr = h0->last.nthr;
    arucohip_handle* h = h0->last.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    if (owner) *owner = h;
    HIPCHK(h, hipSetDevice(h->device));
    // the frame's planes are consecutive; every plane owns cap_cdesc descriptor slots
    std::vector<ContourDesc> all;
    for (int t = 0; t < nthr; t++) {
        const int plane = frame * nthr + t;
        uint32_t line[TC_LATE + 1] = {};
        HIPCHK(h, hipMemcpyAsync(line, h->buf.trig_cnt + (size_t)plane * TRIG_CNT_STRIDE, sizeof(line), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const uint32_t n = std::min(line[TC_CDESC], h->buf.cap_cdesc);
        const uint32_t nlate = std::min(line[TC_LATE], h->buf.cap_cdesc - n);   // a lane's late list: the last nlate slots of the plane's array
        if (!n && !nlate) continue;
        const size_t at = all.size();
        all.resize(at + n + nlate);
        const ContourDesc* base = h->buf.cdesc + (size_t)plane * h->buf.cap_cdesc;
        if (n) HIPCHK(h, hipMemcpyAsync(all.data() + at, base, n * sizeof(ContourDesc), hipMemcpyDeviceToHost, h->stream));
        if (nlate) HIPCHK(h, hipMemcpyAsync(all.data() + at + n, base + (h->buf.cap_cdesc - nlate), nlate * sizeof(ContourDesc), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    out->clear();
    for (auto& c : all)
        if (c.n > 0) out->push_back(c);
    std::sort(out->begin(), out->end(), [](const ContourDesc& a, const ContourDesc& b) {
        if (a.plane != b.plane) return a.plane < b.plane;
        return a.key > b.key;
    });
    return ARUCOHIP_OK;
}

int arucohip_debug_num_contours(arucohip_handle* h, int frame, int* n) {
    std::vector<ContourDesc> v;
    int rc = fetch_contours(h, frame, &v);
    if (rc) return rc;
    *n = (int)v.size();
    return ARUCOHIP_OK;
}

int arucohip_debug_contour(arucohip_handle* h0, int frame, int index, int* is_hole, int* sx, int* sy, int16_t* xy, int cap_points, int* n_points) {
    std::vector<ContourDesc> v;
    arucohip_handle* h = h0;
    int rc = fetch_contours(h0, frame, &v, &h);
    if (rc) return rc;
    if (index < 0 || index >= (int)v.size()) return ARUCOHIP_E_INVALID;
    const ContourDesc& c = v[index];
    if (is_hole) *is_hole = c.hole;
    if (sx) *sx = c.x0;
    if (sy) *sy = c.y0;
    if (n_points) *n_points = c.n;
    if (xy && cap_points >= c.n) {
        HIPCHK(h, hipMemcpyAsync(xy, h->buf.pool + c.pool_off, (size_t)c.n * sizeof(short2), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else if (xy) {
        return ARUCOHIP_E_CAPACITY;
    }
    return ARUCOHIP_OK;
}

// start candidates of one frame and kind as candidates_sparse_kernel left them: the filled part of each plane's half of buf.trig
int arucohip_debug_start_candidates(arucohip_handle* h0, int frame, int kind, uint32_t* yx, int cap, int* n) {
    if (!h0 || !n || (!yx && cap > 0) || cap < 0 || kind < 0 || kind > 1) return ARUCOHIP_E_INVALID;
    const int nthr = h0->last.nthr;
    arucohip_handle* h = h0->last.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    if (h->buf.seg_mode) return fail(h0, ARUCOHIP_E_INVALID, "debug_start_candidates: this handle follows borders by waypoint segments and keeps no start-candidate lists");
    HIPCHK(h, hipSetDevice(h->device));
    const uint32_t half = h->buf.cap_trig / 2;
    std::vector<uint2> recs;
    int k = 0;
    for (int t = 0; t < nthr; t++) {
        const size_t plane = (size_t)frame * nthr + t;
        uint32_t cnt = 0;
        HIPCHK(h, hipMemcpyAsync(&cnt, h->buf.trig_cnt + plane * TRIG_CNT_STRIDE + kind, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        cnt = std::min(cnt, half);   // a list that overflowed holds its first half-capacity records (ST_TRIG_OVERFLOW is set)
        if (!cnt) continue;
        recs.resize(cnt);
        HIPCHK(h, hipMemcpyAsync(recs.data(), h->buf.trig + plane * h->buf.cap_trig + (size_t)kind * half, cnt * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (uint32_t i = 0; i < cnt; i++, k++)
            if (k < cap) yx[k] = recs[i].y;
    }
    *n = k;
    return k > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

int arucohip_debug_counters(arucohip_handle* h, uint32_t* out8) {
    if (!h || !out8) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    const Batch& r = h->last;
    uint64_t acc[CNT_FIXED] = {};
    uint64_t ntrig = 0, nraw = 0, nlong = 0, nlate = 0, nside = 0;
    for (const Span& s : r) {
        arucohip_handle* w = s.w;
        uint32_t cnt[CNT_FIXED];
        HIPCHK(h, hipMemcpyAsync(cnt, w->buf.counters, sizeof(cnt), hipMemcpyDeviceToHost, w->stream));
        const int planes = s.count * r.nthr;
        std::vector<uint32_t> tc((size_t)planes * TRIG_CNT_STRIDE), rc_((size_t)planes * TRIG_CNT_STRIDE), rg((size_t)planes * TRIG_CNT_STRIDE);
        HIPCHK(h, hipMemcpyAsync(tc.data(), w->buf.trig_cnt, tc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(rc_.data(), w->buf.raw_cnt, rc_.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(rg.data(), w->buf.ring_cnt, rg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        // walks that entered the first generation behind the fork point (both kinds, every sublist), forked or not
        uint32_t late[2][8] = {};
        if (!w->buf.seg_mode)
            for (int kind = 0; kind < 2; kind++)
                HIPCHK(h, hipMemcpy2DAsync(late[kind], sizeof(uint32_t), w->buf.gen_cnt + gen_cnt_word(kind, GEN_FORK_AFTER + 1, 0),
                                           (gen_cnt_word(kind, GEN_FORK_AFTER + 1, 1) - gen_cnt_word(kind, GEN_FORK_AFTER + 1, 0)) * sizeof(uint32_t),
                                           sizeof(uint32_t), 8, hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipStreamSynchronize(w->stream));
        for (int i = 0; i < 16; i++) nlate += late[i / 8][i % 8];
        nside += w->side_stream ? 1 : 0;
        for (int i = 0; i < CNT_FIXED; i++)
            if (i != 1 && i != 2) acc[i] = (i == CNT_STATUS) ? (acc[i] | cnt[i]) : acc[i] + cnt[i];   // [1], [2] come from the planes' own counters below
        for (int p = 0; p < planes; p++) {
            ntrig += tc[(size_t)p * TRIG_CNT_STRIDE] + tc[(size_t)p * TRIG_CNT_STRIDE + 1];
            acc[1] += tc[(size_t)p * TRIG_CNT_STRIDE + TC_CDESC] + tc[(size_t)p * TRIG_CNT_STRIDE + TC_LATE], acc[2] += tc[(size_t)p * TRIG_CNT_STRIDE + TC_POOL];
            nraw += rc_[(size_t)p * TRIG_CNT_STRIDE];
            nlong += rg[(size_t)p * TRIG_CNT_STRIDE] + rg[(size_t)p * TRIG_CNT_STRIDE + 1];
        }
    }
    for (int i = 0; i < CNT_FIXED; i++) out8[i] = (uint32_t)std::min<uint64_t>(acc[i], 0xFFFFFFFFu);
    out8[0] = (uint32_t)std::min<uint64_t>(ntrig, 0xFFFFFFFFu);   // start candidates after the run rule (all planes)
    const bool seg = r.nspan > 0 && r.span[0].w->buf.seg_mode;
    out8[4] = (uint32_t)std::min<uint64_t>(seg ? nraw : nlong, 0xFFFFFFFFu);   // waypoint records (segment mode) / long walks = checkpoint rings handed out
    out8[5] = seg ? 1u : 0u;                                      // which of the two [4] counts
    out8[6] = (uint32_t)std::min<uint64_t>(nlate, 0xFFFFFFFFu);   // long walks that reached the late generations (the ones a side stream carries)
    out8[7] = (uint32_t)nside;                                    // side streams among the workers that hold the batch (a pipeline lane: 0)
    return ARUCOHIP_OK;
}

// One threshold plane's counters of the last batch as the kernels left them: reads, launches nothing. plane = frame * planes per frame + t.
int arucohip_debug_plane_counters(arucohip_handle* h0, int plane, uint32_t* out, int cap) {
    constexpr int WORDS = TRIG_CNT_STRIDE + 4;
    if (!h0 || !out || plane < 0) return ARUCOHIP_E_INVALID;
    if (cap < WORDS) return ARUCOHIP_E_CAPACITY;
    const int nthr = h0->last.nthr;
    int frame = 0;
    arucohip_handle* h = h0->last.holder(plane / nthr, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t at = ((size_t)frame * nthr + plane % nthr) * TRIG_CNT_STRIDE;
    uint32_t rings[2] = {}, raw = 0;
    HIPCHK(h, hipMemcpyAsync(out, h->buf.trig_cnt + at, TRIG_CNT_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(rings, h->buf.ring_cnt + at, sizeof(rings), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&raw, h->buf.raw_cnt + at, sizeof(raw), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[TRIG_CNT_STRIDE] = rings[0], out[TRIG_CNT_STRIDE + 1] = rings[1], out[TRIG_CNT_STRIDE + 2] = raw;
    out[TRIG_CNT_STRIDE + 3] = h->buf.seg_mode ? 1u : 0u;
    return ARUCOHIP_OK;
}

// ---- stage entry points (markerdetector.h:255-280)
int arucohip_threshold(arucohip_handle* h, int method, const uint8_t* gray, int W, int H, size_t row_stride, double param1, double param2, uint8_t* dst) {
    if (!h || !gray || !dst) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, 1, W, H, row_stride);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    arucohip_params_t saved = h->params;
    arucohip_params_t p = saved;
    p.thres_method = method;
    if (param1 != -1) p.thres_param1 = param1;   // thresHold(): -1 selects the configured value (:646-649)
    if (param2 != -1) p.thres_param2 = param2;
    p.thres_param1_range = 0;
    if ((rc = validate_params(h, &p))) return rc;
    h->params = p;
    DetectParams dp;
    rc = make_detect_params(h, W, H, &dp);
    h->params = saved;
    if (rc) return rc;
    const uint8_t* gray_dev;
    FrameGeom g;
    if ((rc = stage_frames(h, gray, 1, W, H, row_stride, (size_t)H * row_stride, 0, 1, &gray_dev, &g))) return rc;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), h->stream));
    if ((rc = ensure_bits_geometry(h, W, H))) return rc;
    if ((rc = run_threshold(h, h->stream, gray_dev, g, 1, dp, true))) return rc;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(dst, h->buf.thres, (size_t)W * H, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->last = plan_batch(h, 1, W, H, 1);
    return ARUCOHIP_OK;
}

int arucohip_detect_rectangles(arucohip_handle* h, const uint8_t* thres, int W, int H, size_t row_stride, float* quads, int cap, int* n) {
    if (!h || !thres || !n) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, 1, W, H, row_stride);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DetectParams dp;
    arucohip_params_t saved = h->params;
    h->params.thres_param1_range = 0;
    rc = make_detect_params(h, W, H, &dp);
    h->params = saved;
    if (rc) return rc;
    const uint8_t* dev;
    FrameGeom g;
    if ((rc = stage_frames(h, thres, 1, W, H, row_stride, (size_t)H * row_stride, 0, 1, &dev, &g))) return rc;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), h->stream));
    if ((rc = ensure_walk_scratch(h, 1, dp))) return rc;
    if ((rc = ensure_bits_geometry(h, W, H))) return rc;
    launch_binary_planes(h->stream, dev, g, 1, h->buf);
    if ((rc = run_rectangles(h, h->stream, g, 1, dp, nullptr))) return rc;
    HIPCHK(h, hipGetLastError());
    h->last = plan_batch(h, 1, W, H, 1);
    std::vector<Cand> v;
    if ((rc = fetch_cands(h, 0, &v))) return rc;
    HIPCHK(h, hipMemcpy(h->h_counters, h->buf.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if ((rc = check_status(h, h->h_counters[CNT_STATUS]))) return rc;
    *n = (int)v.size();
    for (int k = 0; k < (int)v.size() && k < cap; k++)
        for (int i = 0; i < 8; i++) quads[k * 8 + i] = v[k].c[i];
    return (int)v.size() > cap ? ARUCOHIP_E_CAPACITY : ARUCOHIP_OK;
}

int arucohip_warp(arucohip_handle* h, const uint8_t* gray, int W, int H, size_t row_stride, const float quad[8], int size, uint8_t* dst) {
    if (!h || !gray || !quad || !dst) return ARUCOHIP_E_INVALID;
    if (size < 1 || size > 128) return fail(h, ARUCOHIP_E_INVALID, "warp size outside 1..128");
    int rc = check_geometry(h, 1, W, H, row_stride);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const uint8_t* dev;
    FrameGeom g;
    if ((rc = stage_frames(h, gray, 1, W, H, row_stride, (size_t)H * row_stride, 0, 1, &dev, &g))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_small_f, quad, 8 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    launch_warp_only(h->stream, dev, g, h->d_small_f, size, h->d_patch);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(dst, h->d_patch, (size_t)size * size, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

// MarkerDetector::refineCandidateLines (markerdetector.cpp:931-997) on a caller-supplied contour: the contour becomes border 0 of plane 0, the
// corners candidate 0 of frame 0, and one wave of refine_lines_kernel does what it does for a decoded candidate of a batch.
int arucohip_refine_candidate_lines(arucohip_handle* h, const int32_t* contour_xy, int npoints, float corners[8], const float* K, const float* dist, int ndist) {
    if (!h || !contour_xy || !corners || npoints < 1) return ARUCOHIP_E_INVALID;
    if ((uint32_t)npoints > h->buf.cap_pool) return fail(h, ARUCOHIP_E_CAPACITY, "contour longer than the handle's point list (points_per_frame)");
    HIPCHK(h, hipSetDevice(h->device));
    CamModel cam;
    int rc = make_cam(h, K, dist, ndist, -1.f, 0, &cam);
    if (rc) return rc;
    std::vector<short2> pts((size_t)npoints);
    for (int i = 0; i < npoints; i++) {
        const int32_t x = contour_xy[2 * i], y = contour_xy[2 * i + 1];
        if (x < 0 || y < 0 || x > 32767 || y > 32767) return fail(h, ARUCOHIP_E_INVALID, "contour point outside 0..32767");
        pts[i] = make_short2((short)x, (short)y);
    }
    ContourDesc cd{};
    cd.plane = 0, cd.x0 = pts[0].x, cd.y0 = pts[0].y, cd.hole = 0, cd.n = npoints, cd.key = 0, cd.pool_off = 0, cd.ck_off = 0xFFFFFFFFu;
    Cand c{};
    for (int k = 0; k < 4; k++) {
        c.c[2 * k] = corners[2 * k], c.c[2 * k + 1] = corners[2 * k + 1];
        // Point(candidate[k]): cv::Point2f -> cv::Point rounds to nearest, ties to even (saturate_cast<int>(float) = cvRound)
        const long qx = lrintf(corners[2 * k]), qy = lrintf(corners[2 * k + 1]);
        c.qx[k] = (int16_t)std::min<long>(std::max<long>(qx, -32768), 32767), c.qy[k] = (int16_t)std::min<long>(std::max<long>(qy, -32768), 32767);
    }
    c.cdesc = 0, c.swapped = 0, c.id = 0, c.nrot = 0;
    DetectParams dp;
    std::memset(&dp, 0, sizeof(dp));
    dp.nthr = 1, dp.corner_method = ARUCOHIP_CORNER_LINES, dp.warp_size = h->params.warp_size, dp.decoder = ARUCOHIP_DECODER_USER;   // ids are given: no cell decode
    hipStream_t s = h->stream;
    const Buffers& b = h->buf;
    const uint32_t one = 1, entry = 0;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    HIPCHK(h, hipMemcpyAsync(b.pool, pts.data(), pts.size() * sizeof(short2), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.cdesc, &cd, sizeof(cd), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.cands, &c, sizeof(c), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.cand_list, &entry, sizeof(entry), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.counters + CNT_NCAND, &one, sizeof(one), hipMemcpyHostToDevice, s));
    FrameGeom g{};
    g.width = h->lim.max_width, g.height = h->lim.max_height;
    launch_refine_lines(s, g, 1, dp, cam, b, false);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&c, b.cands, sizeof(c), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int k = 0; k < 8; k++) corners[k] = c.c[k];
    h->last = Batch{};   // the lists no longer hold a batch
    return ARUCOHIP_OK;
}

// Test hook: the locked-corner pre-pass (findCornerMaxima) and the SUBPIX / HARRIS refinement on caller-supplied corners. The corners become
// candidates of frame 0 (four a candidate, id 0; a partly filled last one repeats its last corner) and the two launches of detect_core do
// what they do for a batch's decoded candidates. Unlike stage_frames the frame keeps its row stride on the device, so that the kernels'
// row indexing is part of what runs.
int arucohip_debug_refine_pixels(arucohip_handle* h, const uint8_t* gray, int W, int H, size_t row_stride, float* corners_xy, int ncorners, int method,
                                 int win, int locked_wsize) {
    if (!h || !gray || !corners_xy) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, 1, W, H, row_stride);
    if (rc) return rc;
    if (row_stride > 4 * (size_t)h->lim.max_width) return fail(h, ARUCOHIP_E_INVALID, "row_stride beyond four times the handle's width");
    if (method != ARUCOHIP_CORNER_NONE && method != ARUCOHIP_CORNER_HARRIS && method != ARUCOHIP_CORNER_SUBPIX)
        return fail(h, ARUCOHIP_E_INVALID, "refine_pixels: method is not NONE, HARRIS or SUBPIX");
    if (locked_wsize < 0) return fail(h, ARUCOHIP_E_INVALID, "locked-corner window < 0");
    if (locked_wsize > 31) return fail(h, ARUCOHIP_E_UNSUPPORTED, "locked corners: window outside 1..31");
    if (method == ARUCOHIP_CORNER_NONE && locked_wsize == 0) return fail(h, ARUCOHIP_E_INVALID, "refine_pixels: nothing to run");
    if (method == ARUCOHIP_CORNER_SUBPIX && win > 15) return fail(h, ARUCOHIP_E_UNSUPPORTED, "SUBPIX window > 15");
    if (method == ARUCOHIP_CORNER_SUBPIX && win < 1) return fail(h, ARUCOHIP_E_INVALID, "SUBPIX window < 1");
    const Buffers& b = h->buf;
    if (ncorners < 1) return fail(h, ARUCOHIP_E_INVALID, "ncorners < 1");
    if (ncorners > 4 * b.cap_cands) return fail(h, ARUCOHIP_E_CAPACITY, "more corners than four times the handle's candidates per frame");
    for (int i = 0; i < 2 * ncorners; i++)
        if (!(std::fabs(corners_xy[i]) <= 65534.f)) return fail(h, ARUCOHIP_E_INVALID, "corner not finite or outside +-65534");   // NaN fails the comparison
    HIPCHK(h, hipSetDevice(h->device));
    const int nc = (ncorners + 3) / 4;
    std::vector<Cand> v((size_t)nc);
    for (int k = 0; k < nc; k++) {
        Cand c{};
        for (int j = 0; j < 4; j++) {
            const int i = std::min(4 * k + j, ncorners - 1);
            c.c[2 * j] = corners_xy[2 * i], c.c[2 * j + 1] = corners_xy[2 * i + 1];
        }
        c.cdesc = 0, c.swapped = 0, c.id = 0, c.nrot = 0;
        v[k] = c;
    }
    DetectParams dp;
    std::memset(&dp, 0, sizeof(dp));
    dp.nthr = 1, dp.corner_method = method, dp.subpix_win = win, dp.locked = locked_wsize > 0, dp.locked_wsize = locked_wsize;
    hipStream_t s = h->stream;
    const size_t bytes = (size_t)(H - 1) * row_stride + (size_t)W;   // the last row need not be padded
    HIPCHK(h, h->d_gray.reserve(bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_gray, gray, bytes, hipMemcpyHostToDevice, s));
    FrameGeom g{};
    g.width = W, g.height = H, g.row_stride = row_stride, g.frame_stride = (size_t)H * row_stride;
    const int32_t n32 = nc;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    HIPCHK(h, hipMemcpyAsync(b.cands, v.data(), v.size() * sizeof(Cand), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.ncands, &n32, sizeof(n32), hipMemcpyHostToDevice, s));
    if (dp.locked) launch_locked_corners(s, h->d_gray, g, 1, dp, b);
    if (method != ARUCOHIP_CORNER_NONE) launch_refine_pixels(s, h->d_gray, g, 1, dp, b);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(v.data(), b.cands, v.size() * sizeof(Cand), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < ncorners; i++) corners_xy[2 * i] = v[i / 4].c[2 * (i % 4)], corners_xy[2 * i + 1] = v[i / 4].c[2 * (i % 4) + 1];
    h->last = Batch{};   // the lists no longer hold a batch
    return ARUCOHIP_OK;
}

// Test hook: the decode stage on caller-supplied integer quads. The quads become candidates of the frames they name (in the order given, which is
// also their order in the flat list), stage_quads_kernel solves their inverse homographies with the pipeline's homography_lane, and launch_decode
// runs with the handle's current parameters and the frame count of the call, so the kernels a batch of that shape would take are the ones that
// run (fused_cells = false: cells_decode_kernel stands in for the head of refine_lines_kernel, the same cells_decode_wave). Like
// arucohip_debug_refine_pixels the frames keep their row stride on the device.
int arucohip_debug_decode_quads(arucohip_handle* h, const uint8_t* gray, int nframes, int W, int H, size_t row_stride, const int16_t* quads_xy,
                                const int32_t* frame_of, int n, double* iM, uint16_t* hist, int32_t* thr, uint8_t* cells49, uint8_t* patches, int32_t* ids,
                                int32_t* nrot, int32_t* paths) {
    if (!h || !gray || !quads_xy || !frame_of) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, nframes, W, H, row_stride);
    if (rc) return rc;
    if (nframes > h->cap_frames) return fail(h, ARUCOHIP_E_INVALID, "decode_quads: more frames than one worker of the handle holds");
    if (row_stride > 4 * (size_t)h->lim.max_width) return fail(h, ARUCOHIP_E_INVALID, "row_stride beyond four times the handle's width");
    if (h->params.decoder_kind == ARUCOHIP_DECODER_USER) return fail(h, ARUCOHIP_E_UNSUPPORTED, "decode_quads: the caller's decoder runs on the host");
    const Buffers& b = h->buf;
    if (n < 1) return fail(h, ARUCOHIP_E_INVALID, "decode_quads: n < 1");
    if ((uint32_t)n > b.cap_flat) return fail(h, ARUCOHIP_E_CAPACITY, "decode_quads: more quads than the handle's flat candidate list holds");
    std::vector<int32_t> per_frame((size_t)nframes, 0);
    std::vector<uint32_t> list((size_t)n);
    for (int i = 0; i < n; i++) {
        const int32_t f = frame_of[i];
        if (f < 0 || f >= nframes) return fail(h, ARUCOHIP_E_INVALID, "decode_quads: frame index outside the call's frames");
        if (per_frame[f] >= b.cap_cands) return fail(h, ARUCOHIP_E_CAPACITY, "decode_quads: more quads in a frame than candidates_per_frame");
        list[i] = ((uint32_t)f << 16) | (uint32_t)per_frame[f]++;
    }
    DetectParams dp;
    if ((rc = make_detect_params(h, W, H, &dp))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<Cand> v((size_t)nframes * b.cap_cands);
    for (int i = 0; i < n; i++) {
        Cand c{};
        for (int k = 0; k < 4; k++) {
            c.qx[k] = quads_xy[8 * i + 2 * k], c.qy[k] = quads_xy[8 * i + 2 * k + 1];
            c.c[2 * k] = (float)c.qx[k], c.c[2 * k + 1] = (float)c.qy[k];
        }
        c.cdesc = 0, c.swapped = 0, c.id = -1, c.nrot = 0;
        v[(size_t)(list[i] >> 16) * b.cap_cands + (list[i] & 0xFFFFu)] = c;
    }
    FrameGeom g{};
    g.width = W, g.height = H, g.row_stride = row_stride, g.frame_stride = (size_t)H * row_stride;
    const bool cells = decode_from_cells(g, nframes, dp);
    const size_t npx = (size_t)dp.warp_size * dp.warp_size;
    if (!cells) {
        HIPCHK(h, h->patches.reserve((size_t)b.cap_flat * npx));
        h->buf.patches = h->patches;
    }
    hipStream_t s = h->stream;
    const size_t bytes = ((size_t)nframes * H - 1) * row_stride + (size_t)W;   // the last row need not be padded
    HIPCHK(h, h->d_gray.reserve(bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_gray, gray, bytes, hipMemcpyHostToDevice, s));
    const uint32_t n32 = (uint32_t)n;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    HIPCHK(h, hipMemcpyAsync(b.cands, v.data(), v.size() * sizeof(Cand), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.ncands, per_frame.data(), per_frame.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.cand_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.counters + CNT_NCAND, &n32, sizeof(n32), hipMemcpyHostToDevice, s));
    launch_stage_quads(s, b, n32, dp.warp_size);
    launch_decode(s, h->d_gray, g, nframes, dp, b, false);
    HIPCHK(h, hipGetLastError());
    std::vector<uint8_t> cells64;
    if (iM) HIPCHK(h, hipMemcpyAsync(iM, b.iM, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (hist) HIPCHK(h, hipMemcpyAsync(hist, b.hist, (size_t)n * 256 * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
    if (thr) HIPCHK(h, hipMemcpyAsync(thr, b.othr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (cells49 && cells) {
        cells64.resize((size_t)n * 64);
        HIPCHK(h, hipMemcpyAsync(cells64.data(), b.cells, cells64.size(), hipMemcpyDeviceToHost, s));
    }
    if (patches && !cells) HIPCHK(h, hipMemcpyAsync(patches, b.patches, (size_t)n * npx, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(v.data(), b.cands, v.size() * sizeof(Cand), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    h->last = Batch{};   // the lists no longer hold a batch
    h->cells_valid = false;
    for (size_t i = 0; i < cells64.size() / 64; i++)
        for (int cy = 0; cy < 7; cy++)
            for (int cx = 0; cx < 7; cx++) cells49[i * 49 + cy * 7 + cx] = cells64[i * 64 + cy * 8 + cx];
    for (int i = 0; i < n; i++) {
        const Cand& c = v[(size_t)(list[i] >> 16) * b.cap_cands + (list[i] & 0xFFFFu)];
        if (ids) ids[i] = c.id;
        if (nrot) nrot[i] = c.nrot;
    }
    if (paths) *paths = cells ? 1 : 2;
    return ARUCOHIP_OK;
}

// Test hook: the marker-list tail of a batch (finalize_kernel, then the list-driven pose_kernel under detect_core's condition) on caller-made decoded
// candidates. They become the candidates of the frames they name, in the order given; make_detect_params builds the parameters, so the border
// rectangle is the pipeline's; the counters are cleared as a batch clears them, plane_status goes into the planes' TC_STATUS words, and the marker
// rows with the header slot are filled with 0xA5 first, so that what the kernels leave alone can be told. Unlike the other hooks it leaves h->last
// describing these frames (one span on this handle): the batch consumers then run on the crafted lists.
int arucohip_debug_marker_tail(arucohip_handle* h, int nframes, int W, int H, const int32_t* ids, const float* corners, const int32_t* frame_of, int n,
                               const uint32_t* plane_status, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                               arucohip_marker_t* out_dev, int out_cap, int32_t* n_out_dev, arucohip_marker_t* rows, int32_t* nmarkers, uint32_t* status,
                               uint32_t* nmark, uint32_t* marker_list, int32_t* hdr) {
    if (!h || n < 0 || (n > 0 && (!ids || !corners || !frame_of))) return ARUCOHIP_E_INVALID;
    int rc = check_geometry(h, nframes, W, H, (size_t)W);
    if (rc) return rc;
    if (nframes > h->cap_frames) return fail(h, ARUCOHIP_E_INVALID, "marker_tail: more frames than one worker of the handle holds");
    if ((out_dev || n_out_dev) && (!out_dev || !n_out_dev || out_cap < 1))
        return fail(h, ARUCOHIP_E_INVALID, "marker_tail: the write-through arrays come together, with out_cap >= 1");
    const Buffers& b = h->buf;
    std::vector<int32_t> per_frame((size_t)nframes, 0);
    std::vector<Cand> v((size_t)nframes * b.cap_cands);
    for (int i = 0; i < n; i++) {
        const int32_t f = frame_of[i];
        if (f < 0 || f >= nframes) return fail(h, ARUCOHIP_E_INVALID, "marker_tail: frame index outside the call's frames");
        if (per_frame[f] >= b.cap_cands) return fail(h, ARUCOHIP_E_CAPACITY, "marker_tail: more candidates in a frame than candidates_per_frame");
        Cand c{};
        for (int k = 0; k < 8; k++) {
            const float x = corners[8 * (size_t)i + k];
            if (!(std::fabs(x) <= 65534.f)) return fail(h, ARUCOHIP_E_INVALID, "corner not finite or outside +-65534");   // NaN fails the comparison
            c.c[k] = x;
        }
        for (int k = 0; k < 4; k++) c.qx[k] = (int16_t)std::min<long>(std::max<long>(lrintf(c.c[2 * k]), -32768), 32767),
                                    c.qy[k] = (int16_t)std::min<long>(std::max<long>(lrintf(c.c[2 * k + 1]), -32768), 32767);
        c.cdesc = 0, c.swapped = 0, c.id = ids[i], c.nrot = 0;
        v[(size_t)f * b.cap_cands + per_frame[f]++] = c;
    }
    DetectParams dp;
    if ((rc = make_detect_params(h, W, H, &dp))) return rc;
    CamModel cam;
    if ((rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nrows = (size_t)nframes * b.cap_markers;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    uint32_t st_all = 0;
    if (plane_status) {   // one word per plane, each in the plane's own counter line; the batch's status word carries every bit as well (flag_overflow)
        HIPCHK(h, hipMemcpy2DAsync(b.trig_cnt + TC_STATUS, TRIG_CNT_STRIDE * sizeof(uint32_t), plane_status, sizeof(uint32_t), sizeof(uint32_t),
                                   (size_t)nframes * dp.nthr, hipMemcpyHostToDevice, s));
        for (int i = 0; i < nframes * dp.nthr; i++) st_all |= plane_status[i];
        HIPCHK(h, hipMemcpyAsync(b.counters + CNT_STATUS, &st_all, sizeof(st_all), hipMemcpyHostToDevice, s));
    }
    HIPCHK(h, hipMemsetAsync(b.markers, 0xA5, (nrows + 1) * sizeof(arucohip_marker_t), s));
    HIPCHK(h, hipMemsetAsync(b.marker_list, 0xA5, nrows * sizeof(uint32_t), s));
    HIPCHK(h, hipMemcpyAsync(b.cands, v.data(), v.size() * sizeof(Cand), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b.ncands, per_frame.data(), per_frame.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    FrameGeom g{};
    g.width = W, g.height = H, g.row_stride = (size_t)W, g.frame_stride = (size_t)W * H;
    launch_finalize(s, g, nframes, dp, cam, b, out_dev, out_cap, n_out_dev);
    if (cam.has_K && cam.marker_size > 0) launch_pose(s, nframes, cam, b);
    HIPCHK(h, hipGetLastError());
    std::vector<uint32_t> cnt(CNT_FIXED);
    if (rows) HIPCHK(h, hipMemcpyAsync(rows, b.markers, nrows * sizeof(arucohip_marker_t), hipMemcpyDeviceToHost, s));
    if (nmarkers) HIPCHK(h, hipMemcpyAsync(nmarkers, b.nmarkers, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (marker_list) HIPCHK(h, hipMemcpyAsync(marker_list, b.marker_list, nrows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (hdr) HIPCHK(h, hipMemcpyAsync(hdr, b.markers + nrows, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cnt.data(), b.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (status) *status = cnt[CNT_STATUS];
    if (nmark) *nmark = cnt[CNT_NMARK];
    Batch last;
    last.nspan = 1, last.frames = nframes, last.W = W, last.H = H, last.nthr = dp.nthr, last.frame_w = W, last.frame_h = H;
    last.span[0] = {h, 0, nframes};
    h->last = last;
    h->cells_valid = false;
    return ARUCOHIP_OK;
}

int arucohip_board_detect_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type, const float* K,
                                const float* dist, int ndist, float marker_size, float repj_err_thres, int y_perp, arucohip_board_t* out, float* prob) {
    if (!h || !out || !prob) return ARUCOHIP_E_INVALID;
    if (nboard <= 0 || !ids || !obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    if (nboard * 12 > 8192) return fail(h, ARUCOHIP_E_CAPACITY, "board with too many markers");
    HIPCHK(h, hipSetDevice(h->device));
    float zeros[4] = {0, 0, 0, 0};
    if (!dist || ndist == 0) dist = zeros, ndist = 4;
    CamModel cam;
    int rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam);
    if (rc) return rc;
    const BoardDef board{ids, obj, nboard, info_type, marker_size, repj_err_thres};
    // every worker solves the boards of the frames it detected, on its own stream
    const Batch b = h->last.cut(nframes);
    rc = on_workers(h, b, [&](const Span& s) -> int {
        arucohip_handle* w = s.w;
        HIPCHK(h, w->d_board.reserve((size_t)w->cap_frames * (sizeof(arucohip_board_t) + sizeof(float)) + 8192 * sizeof(int32_t)));
        arucohip_board_t* d_out = w->d_board;
        float* d_prob = (float*)(d_out + w->cap_frames);
        BoardDef bd;
        if (const int r = upload_board(h, board, w->stream, (int32_t*)(d_prob + w->cap_frames), w->d_small_f, &bd)) return r;
        launch_board_pose(w->stream, s.count, w->buf, bd, cam, d_out, d_prob);
        HIPCHK(h, hipMemcpyAsync(out + s.first, d_out, (size_t)s.count * sizeof(arucohip_board_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(prob + s.first, d_prob, (size_t)s.count * sizeof(float), hipMemcpyDeviceToHost, w->stream));
        return ARUCOHIP_OK;
    });
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(b.span[0].w->stream));
    // a frame with more member markers than the kernel's correspondence array holds is reported, not truncated silently
    for (const Span& s : h->last) {
        arucohip_handle* w = s.w;
        HIPCHK(h, hipMemcpy(w->h_counters, w->buf.counters, CNT_FIXED * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (w->h_counters[CNT_STATUS] & ST_MARKER_OVERFLOW) return fail(h, ARUCOHIP_E_CAPACITY, "a frame has more than 128 board markers");
    }
    h->last.board_frames = nframes;
    return ARUCOHIP_OK;
}

// SURVEY §8 row f4, batched: Marker::glGetModelViewMatrix (src/marker.h:90) for every marker of the last batch in one launch
int arucohip_gl_modelview_batch(arucohip_handle* h, int nframes, int cap, double* modelview, int32_t* n_out) {
    if (!h || !modelview || !n_out || cap < 1) return ARUCOHIP_E_INVALID;
    const Batch& r = h->last;
    if (r.nspan > 1) return fail(h, ARUCOHIP_E_UNSUPPORTED, "not available for batches split over chunk streams");
    if (nframes < 1 || nframes > r.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    arucohip_handle* w = r.span[0].w;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t need = (size_t)nframes * cap * 16 * sizeof(double);
    double* d_mv;
    if (const int rc = carve_scratch(w, h, [&](Carver& cv) {
            d_mv = cv.take<double>((size_t)nframes * cap * 16);
        }))
        return rc;
    launch_gl_modelview(w->stream, nframes, cap, w->buf, d_mv);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(modelview, d_mv, need, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(h, hipMemcpyAsync(n_out, w->buf.nmarkers, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(h, hipStreamSynchronize(w->stream));
    for (int f = 0; f < nframes; f++) n_out[f] = std::min(std::min(n_out[f], cap), w->buf.cap_markers);
    return ARUCOHIP_OK;
}

int arucohip_calculate_extrinsics(arucohip_handle* h, arucohip_marker_t* markers, int n, const float* K, const float* dist, int ndist,
                                  float marker_size, int y_perp) {
    if (!h || !markers || n < 0 || !K) return ARUCOHIP_E_INVALID;
    if (!(marker_size > 0)) return fail(h, ARUCOHIP_E_INVALID, "marker size must be positive");   // marker.cpp:114
    if (n == 0) return ARUCOHIP_OK;
    if ((size_t)n > (size_t)h->cap_frames * h->buf.cap_markers) return fail(h, ARUCOHIP_E_CAPACITY, "too many markers for this handle");
    HIPCHK(h, hipSetDevice(h->device));
    CamModel cam;
    int rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->buf.markers, markers, (size_t)n * sizeof(arucohip_marker_t), hipMemcpyHostToDevice, h->stream));
    launch_marker_pose(h->stream, h->buf.markers, n, cam);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(markers, h->buf.markers, (size_t)n * sizeof(arucohip_marker_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

// BoardDetector::detect (boarddetector.cpp:90-205). The id filter and point gathering are a few hundred bytes of host
// glue; both solvePnP calls and the reprojection run on the device.
int arucohip_board_detect(arucohip_handle* h, const arucohip_marker_t* markers, int n, const int32_t* ids, const float* obj, int nboard,
                          int info_type, const float* K, const float* dist, int ndist, float marker_size, float repj_err_thres, int y_perp,
                          arucohip_marker_t* out_markers, arucohip_board_t* out, float* prob) {
    if (!h || !out || !prob || n < 0 || (n > 0 && (!markers || !out_markers))) return ARUCOHIP_E_INVALID;
    if (nboard <= 0 || !ids || !obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    std::memset(out, 0, sizeof(*out));
    *prob = 0;
    float ssize = -1;
    if (info_type == ARUCOHIP_BOARD_PIX && marker_size > 0)
        ssize = marker_size;
    else if (info_type == ARUCOHIP_BOARD_METERS)
        ssize = (float)board_side(obj);
    std::vector<int> slot;
    int nb = 0;
    for (int i = 0; i < n; i++) {
        const int32_t* f = std::find(ids, ids + nboard, markers[i].id);
        if (f == ids + nboard) continue;
        out_markers[nb] = markers[i];
        out_markers[nb].ssize = ssize;
        slot.push_back((int)(f - ids));
        nb++;
    }
    out->n_markers = nb;
    if (nb == 0 || !K) return ARUCOHIP_OK;
    bool enough = (marker_size > 0 && info_type == ARUCOHIP_BOARD_PIX) || info_type == ARUCOHIP_BOARD_METERS;
    if (!enough) return ARUCOHIP_OK;
    const double mpp = board_mpp(BoardDef{ids, obj, nboard, info_type, marker_size, repj_err_thres});
    std::vector<float> o3, i2;
    for (int i = 0; i < nb; i++)
        for (int p = 0; p < 4; p++) {
            i2.push_back(out_markers[i].corners[2 * p]), i2.push_back(out_markers[i].corners[2 * p + 1]);
            const float* q = obj + ((size_t)slot[i] * 4 + p) * 3;
            for (int c = 0; c < 3; c++) o3.push_back((float)(q[c] * mpp));
        }
    int npts = nb * 4;
    // d_small_f holds obj[3 npts] + img[2 npts] + the reprojected points [2 npts]
    if (npts * 7 > 8192) return fail(h, ARUCOHIP_E_CAPACITY, "board with too many points");
    HIPCHK(h, hipSetDevice(h->device));
    float zeros[4] = {0, 0, 0, 0};
    if (!dist || ndist == 0) dist = zeros, ndist = 4;
    CamModel cam;
    int rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam);
    if (rc) return rc;
    float* d_obj = h->d_small_f;
    float* d_img = h->d_small_f + 3 * npts;
    double rt[6];
    int ok = 0;
    auto solve = [&](int m) -> int {
        HIPCHK(h, hipMemcpyAsync(d_obj, o3.data(), 3 * m * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_img, i2.data(), 2 * m * sizeof(float), hipMemcpyHostToDevice, h->stream));
        launch_pnp_points(h->stream, d_obj, d_img, m, cam, h->d_small_d, h->d_small_i);
        HIPCHK(h, hipGetLastError());
        return ARUCOHIP_OK;
    };
    if ((rc = solve(npts))) return rc;
    if (repj_err_thres > 0) {
        std::vector<float> rp(2 * npts);
        launch_project_points(h->stream, d_obj, npts, h->d_small_d, cam, d_img + 2 * npts);
        HIPCHK(h, hipMemcpyAsync(rp.data(), d_img + 2 * npts, 2 * npts * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<float> o3f, i2f;
        for (int i = 0; i < npts; i++) {
            float dx = rp[2 * i] - i2[2 * i], dy = rp[2 * i + 1] - i2[2 * i + 1];
            float err = (float)std::sqrt((double)dx * dx + (double)dy * dy);
            if (err < repj_err_thres) {
                for (int c = 0; c < 3; c++) o3f.push_back(o3[3 * i + c]);
                i2f.push_back(i2[2 * i]), i2f.push_back(i2[2 * i + 1]);
            }
        }
        o3.swap(o3f), i2.swap(i2f);
        // fewer than 4 surviving points: the reference's second cv::solvePnP would throw; like the batched kernel the
        // board then has no pose
        if (i2.size() / 2 < 4) {
            *prob = float(nb) / float(nboard);
            return ARUCOHIP_OK;
        }
        if ((rc = solve((int)(i2.size() / 2)))) return rc;
    }
    if (y_perp) launch_rotate_x(h->stream, h->d_small_d);
    HIPCHK(h, hipMemcpyAsync(rt, h->d_small_d, sizeof(rt), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&ok, h->d_small_i, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out->has_pose = ok;
    for (int k = 0; k < 3; k++) out->rvec[k] = rt[k], out->tvec[k] = rt[3 + k];
    *prob = float(nb) / float(nboard);
    return ARUCOHIP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Batches in flight. No reference counterpart (MarkerDetector::detect is synchronous); this is how a stream of batches
// keeps the GPU busy: the tail of a batch is a chain of dependent border steps that a handful of wavefronts work on, the
// head of the next batch is a streaming kernel that wants the whole chip.
// ---------------------------------------------------------------------------------------------
extern "C" {

int arucohip_set_pipeline_depth(arucohip_handle* h, int depth) {
    if (!h || depth < 0 || depth > 8) return ARUCOHIP_E_INVALID;
    for (auto* l : h->lanes)
        if (l->pend.active) return fail(h, ARUCOHIP_E_INVALID, "a submitted batch has not been waited for");
    HIPCHK(h, hipSetDevice(h->device));
    for (auto* l : h->lanes) arucohip_destroy(l);
    h->lanes.clear();
    if (h->last.nspan && h->last.span[0].w != h) h->last = Batch{};   // it was a lane's
    h->next_ticket = 0;
    if (depth == 0) return ARUCOHIP_OK;
    if (!h->ev_submit) HIPCHK(h, hipEventCreateWithFlags(&h->ev_submit, hipEventDisableTiming));
    for (int i = 0; i < depth; i++) {
        arucohip_handle* l = nullptr;
        const int rc = create_child(h, h->lim, false, true, &l);
        if (rc != ARUCOHIP_OK) {   // all or nothing: a later submit must not run at a smaller depth than the caller asked for
            for (auto* made : h->lanes) arucohip_destroy(made);
            h->lanes.clear();
            return fail(h, rc, "creating a pipeline lane failed (no lanes kept)");
        }
        h->lanes.push_back(l);
    }
    return ARUCOHIP_OK;
}

int arucohip_detect_batch_submit(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                                 int frames_on_device, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                                 arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device, int* ticket) {
    if (!h || !ticket) return ARUCOHIP_E_INVALID;
    if (h->lanes.empty()) return fail(h, ARUCOHIP_E_INVALID, "arucohip_set_pipeline_depth first");
    arucohip_handle* l = h->lanes[h->next_ticket % (int)h->lanes.size()];
    if (l->pend.active) return fail(h, ARUCOHIP_E_CAPACITY, "pipeline full: wait for the oldest ticket first");
    HIPCHK(h, hipSetDevice(h->device));
    // what the caller's stream has queued so far (the frames) is visible to the lane
    HIPCHK(h, hipEventRecord(h->ev_submit, h->stream));
    HIPCHK(h, hipStreamWaitEvent(l->stream, h->ev_submit, 0));
    int rc = detect_batch_impl(l, frames, nframes, W, H, row_stride, frame_stride, frames_on_device, 1, K, dist, ndist, marker_size, y_perp, out, cap, n_out,
                               out_on_device, true);
    if (rc) {
        h->err = l->err;
        return rc;
    }
    l->pend.active = true, l->pend.ticket = h->next_ticket, l->pend.cap = cap, l->pend.out_on_device = out_on_device;
    l->pend.out = out, l->pend.n_out = n_out;
    *ticket = h->next_ticket++;
    return ARUCOHIP_OK;
}

// One bad frame must not void a batch (the reference has no limits at all, src/markerdetector.cpp:496-635): a frame whose lists overflowed
// comes back with n = -1 and everything else is valid. This call runs exactly those frames again, one at a time, on a one-frame handle
// whose per-frame lists are 4x (then 16x, 64x) the batch handle's, and patches their results into the caller's arrays.
int arucohip_detect_batch_retry_overflowed(arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride, size_t frame_stride,
                                           int frames_on_device, const float* K, const float* dist, int ndist, float marker_size, int y_perp,
                                           arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device, int* n_retried) {
    if (!h || !frames || !n_out || (cap > 0 && !out) || cap < 0 || nframes < 1) return ARUCOHIP_E_INVALID;
    if (n_retried) *n_retried = 0;
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int32_t> n(nframes);
    if (out_on_device)
        HIPCHK(h, hipMemcpy(n.data(), n_out, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost));
    else
        std::memcpy(n.data(), n_out, (size_t)nframes * sizeof(int32_t));
    std::vector<arucohip_marker_t> tmp((size_t)std::max(cap, 1));
    int ret = ARUCOHIP_OK;
    for (int f = 0; f < nframes; f++) {
        if (n[f] >= 0) continue;
        int32_t got = 0;
        int rc = ARUCOHIP_E_OVERFLOW;
        for (int attempt = 0; attempt < 3 && rc == ARUCOHIP_E_OVERFLOW; attempt++) {
            // 4x, 16x, 64x the batch handle's lists and never more: a cached handle is reused at its size, a frame that overflows 64x is reported
            const int want = h->retry ? std::min(64, attempt == 0 ? h->retry_mult : h->retry_mult * 4) : 4;
            if (attempt > 0 && h->retry && want == h->retry_mult) break;   // already at the cap
            if (!h->retry || want != h->retry_mult) {
                drop_retry(h);
                arucohip_limits_t l = h->lim;
                l.max_batch = 1;
                auto grow = [&](int32_t v, long top) { return (int32_t)std::min<long>((long)v * want, top); };
                l.triggers_per_frame = grow(l.triggers_per_frame, 1L << 22), l.contours_per_frame = grow(l.contours_per_frame, 1L << 18);
                l.points_per_frame = grow(l.points_per_frame, 1L << 24), l.long_walks_per_plane = grow(l.long_walks_per_plane, 1L << 16);
                l.candidates_per_frame = std::min(512, l.candidates_per_frame * 2);
                const int crc = create_child(h, l, false, false, &h->retry);
                if (crc != ARUCOHIP_OK) return fail(h, crc, "creating the retry handle failed");
                h->retry_mult = want;
            }
            rc = arucohip_detect_batch(h->retry, frames + (size_t)f * frame_stride, 1, W, H, row_stride, frame_stride, frames_on_device, K, dist, ndist, marker_size,
                                       y_perp, tmp.data(), cap, &got, 0);
        }
        if (rc != ARUCOHIP_OK && rc != ARUCOHIP_E_CAPACITY) {
            if (ret == ARUCOHIP_OK) ret = fail(h, rc, h->retry ? h->retry->err.c_str() : "retry failed");
            continue;
        }
        if (rc == ARUCOHIP_E_CAPACITY && ret == ARUCOHIP_OK) ret = fail(h, rc, "marker output array too small");
        const int ncopy = std::min<int>(std::max<int>(got, 0), cap);
        if (out_on_device) {
            if (ncopy > 0) HIPCHK(h, hipMemcpy(out + (size_t)f * cap, tmp.data(), (size_t)ncopy * sizeof(arucohip_marker_t), hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(n_out + f, &got, sizeof(int32_t), hipMemcpyHostToDevice));
        } else {
            if (ncopy > 0) std::memcpy(out + (size_t)f * cap, tmp.data(), (size_t)ncopy * sizeof(arucohip_marker_t));
            n_out[f] = got;
        }
        if (n_retried) (*n_retried)++;
    }
    return ret;
}

int arucohip_detect_batch_wait(arucohip_handle* h, int ticket) {
    if (!h || h->lanes.empty() || ticket < 0) return ARUCOHIP_E_INVALID;
    arucohip_handle* l = h->lanes[ticket % (int)h->lanes.size()];
    if (!l->pend.active || l->pend.ticket != ticket) return fail(h, ARUCOHIP_E_INVALID, "no such batch in flight");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = l->pend.out_on_device ? arucohip_batch_status(l) : collect_batch_host(l, l->pend.out, l->pend.cap, l->pend.n_out);
    l->pend.active = false;
    h->last = l->last;
    if (rc) h->err = l->err;
    return rc;
}

}  // extern "C"
