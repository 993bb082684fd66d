// Host side of libarucohip: handle, device buffers, launch order. Implements include/arucohip.h.
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
#include <memory>
#include <string>
#include <vector>

#include "bits_tiles.h"
#include "internal.h"

namespace ah {
void launch_rotate_x(hipStream_t s, double* rt);
}

namespace ah {
Tuning read_tuning() {
    Tuning t;
    auto geti = [](const char* name, int dflt) {
        const char* e = getenv(name);
        return (e && *e) ? atoi(e) : dflt;
    };
    t.walk_fork = geti("ARUCOHIP_WALK_FORK", 1) != 0;
    t.chain = geti("ARUCOHIP_CHAIN", 0) != 0;
    t.cand_sparse = geti("ARUCOHIP_CAND_SPARSE", 1) != 0;
    t.cand_waves = std::max(1, geti("ARUCOHIP_CAND_WAVES", 32));
    t.cand_chunks = std::max(1, geti("ARUCOHIP_CAND_CHUNKS", 16));
    t.leash = geti("ARUCOHIP_LEASH", 0);
    t.fork_after = geti("ARUCOHIP_FORK_AFTER", 3);
    t.quad_blocks = std::max(1, geti("ARUCOHIP_QUAD_BLOCKS", 12));
    t.quad_dual = geti("ARUCOHIP_QUAD_DUAL", 1) != 0;
    t.seg_skip = geti("ARUCOHIP_SEG_SKIP", 1) != 0;
    t.gen_xcd = geti("ARUCOHIP_GEN_XCD", 1) != 0;
    t.threshold_wide = geti("ARUCOHIP_THRESHOLD_WIDE", 1) != 0;
    t.threshold_eo = geti("ARUCOHIP_THRESHOLD_EO", 1) != 0;
#ifdef ARUCOHIP_STAGE_EXPERIMENT
    t.stop_after = geti("ARUCOHIP_STOP_AFTER", 99);   // truncates the pipeline: results are meaningless, only the step time is
#endif
    t.thres_lazy = geti("ARUCOHIP_THRES_BYTES", 0) == 0;
    if (const char* e = getenv("ARUCOHIP_GENS")) {
        for (const char* q = e; *q && t.ngens < 32;) {
            const int v = atoi(q);
            if (v > 0) t.gens[t.ngens++] = v;
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
    return t;
}
}  // namespace ah

using namespace ah;

enum { STAGE_THRESHOLD = 0, STAGE_RECTANGLES, STAGE_IDENTIFY, STAGE_SUBPIXEL, STAGE_FILTERING, STAGE_COUNT };
static const char* kStageNames[STAGE_COUNT] = {"Threshold", "Rectangles", "Identify", "Subpixel", "Filtering"};
// one event after every kernel of a batch; a ring of TSETS batches so that asynchronous steps can be averaged
// slot k = the interval between mark k and mark k + 1. walker_long = the generations of long walks up to the fork of the side
// stream; contour_quad = both passes including the wait for the side stream's late generations.
enum { K_THRESHOLD = 0, K_FILTER, K_WALKERS, K_WALKERS_LONG, K_CONTOUR_QUADS, K_FRAME_CANDS, K_DECODE, K_REFINE_LINES, K_REFINE_PIXELS, K_FINALIZE, K_POSE, K_COUNT };
static const char* kKernelNames[K_COUNT] = {"threshold_kernel", "candidates_kernel", "walker_kernel", "walker_long_kernel", "contour_quad_kernel",
                                            "frame_candidates_kernel", "decode_kernel", "refine_lines_kernel", "refine_pixels_kernel", "finalize_kernel",
                                            "pose_kernel"};
static const int kKernelStage[K_COUNT] = {STAGE_THRESHOLD, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES, STAGE_RECTANGLES,
                                          STAGE_IDENTIFY, STAGE_IDENTIFY, STAGE_SUBPIXEL, STAGE_FILTERING, STAGE_FILTERING};
constexpr int TSETS = 32;

// Memory the handle owns: device memory, or pinned host memory for staging the host reads. reserve() replaces the allocation only when
// `need` exceeds the capacity (exact size, no slack, never shrinks) and then bumps `epoch`, the handle's alloc_epoch: the single-frame
// graph compares it with its capture's, since its launches carry the pointers by value. The destructor frees.
template <typename T>
struct Mem {
    T* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    explicit Mem(bool pinned_ = false) : pinned(pinned_) {}
    Mem(Mem&& o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned) { o.p = nullptr, o.bytes = 0; }
    ~Mem() { (void)release(); }
    operator T*() const { return p; }
    hipError_t reserve(size_t need, uint64_t& epoch) {
        if (need <= bytes) return hipSuccess;
        epoch++;
        hipError_t e = release();
        if (e == hipSuccess) e = pinned ? hipHostMalloc((void**)&p, need) : hipMalloc((void**)&p, need);
        if (e == hipSuccess)
            bytes = need;
        else
            p = nullptr;
        return e;
    }

private:
    hipError_t release() {
        const hipError_t e = p ? (pinned ? hipHostFree(p) : hipFree(p)) : hipSuccess;
        p = nullptr, bytes = 0;
        return e;
    }
};

constexpr int MAX_WORKERS = 8;   // chunk workers of a handle, itself included (ARUCOHIP_STREAMS)

// A batch as the workers hold it: chunk c of its frames ran on worker c (chunk_worker). The handle the caller holds keeps the last one
// (arucohip_handle::last): every call that replaces the device lists sets it whole, from plan_batch, or clears it when they no longer
// hold a batch; a waited ticket adopts its lane's. The getters, board poses, calibration and ChromaticMask read it and nothing else.
struct Span { arucohip_handle* w; int first, count; };   // worker w holds frames [first, first + count)
struct Batch {
    int nspan = 0, frames = 0;
    Span span[MAX_WORKERS] = {};
    int W = 0, H = 0, nthr = 1;
    int board_frames = 0;   // frames whose board poses arucohip_board_detect_batch left in the workers' d_board
    const Span* begin() const { return span; }
    const Span* end() const { return span + nspan; }
    // the worker that holds frame `frame` and the frame's index there; nullptr: the batch has no such frame
    arucohip_handle* holder(int frame, int* local) const {
        for (const Span& s : *this)
            if (frame >= s.first && frame < s.first + s.count) return *local = frame - s.first, s.w;
        return nullptr;
    }
    // the spans of the first nframes frames
    Batch cut(int nframes) const {
        Batch b = *this;
        b.nspan = 0, b.frames = std::min(frames, nframes);
        for (const Span& s : *this)
            if (s.first < nframes) b.span[b.nspan++] = {s.w, s.first, std::min(s.count, nframes - s.first)};
        return b;
    }
};

// highly reliable markers (arucohip_set_dictionary); count 0: none
struct Dictionary {
    int n = 0, count = 0, tau0 = 0;
    float rate = 1.f;
    std::vector<uint64_t> codes;   // kept on the host as well: a new child takes them without reading the device copy back
};

struct arucohip_handle {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    arucohip_params_t params;
    arucohip_limits_t lim;
    Buffers buf{};                    // views: the create-time arrays live in `held`, walk_scratch and patches below
    uint64_t alloc_epoch = 0;         // replacements of owned memory so far (Mem::reserve)
    std::vector<Mem<void>> held;      // create-time memory, held for the handle's life: the Buffers arrays, zero_block, d_small_*, d_patch, pinned staging
    Mem<uint32_t> walk_scratch;       // buf.walk_scratch
    Mem<uint8_t> patches;             // buf.patches
    Mem<uint8_t> d_gray;              // staging for host frames (gray) and the converted BGR frames
    Mem<uint8_t> d_bgr;               // staging for host BGR frames
    arucohip_marker_t* wt_out = nullptr;   // set around detect_core by chunk_enqueue: finalize_kernel writes the results there too
    int32_t* wt_n = nullptr;
    int wt_cap = 0;
    Mem<uint8_t> d_erode;             // eroded planes (params.erode)
    Mem<uint64_t> d_canny;            // CANNY: survivor tiles, edge tiles, changed flag
    // frame undistortion (arucohip_undistort): the map of the last camera is kept (umap_nd = -1: none)
    Mem<short2> d_umap_xy;
    Mem<uint16_t> d_umap_f;
    int umap_w = 0, umap_h = 0, umap_nd = -1;
    float umap_K[9] = {}, umap_d[8] = {};
    Mem<uint8_t> d_undist;            // undistorted frames when the caller wants them on the host
    Dictionary hrm;
    Mem<uint64_t> d_hrm;              // hrm.codes on the device
    // caller's own decoder (arucohip_set_decoder_callback)
    arucohip_decoder_fn decoder_fn = nullptr;
    void* decoder_user = nullptr;
    Mem<int2> d_user_dec;             // [cap_flat] {id, nRotations} returned by the callback
    Mem<uint32_t> hu_list{true};      // pinned staging of the callback path: candidate list, decoder results, call order
    Mem<uint8_t> hu_patches{true};    // pinned staging: the canonical patches handed to the callback (+ one scratch patch)
    size_t bits_bytes = 0;
    int bits_w = 0, bits_h = 0;       // geometry the bit image was last written with (pad words depend on it)
    // pinned host staging
    arucohip_marker_t* h_markers = nullptr;
    int32_t* h_n = nullptr;
    uint32_t* h_counters = nullptr;
    // small device scratch for the stage-level calls
    float* d_small_f = nullptr;       // 4096 floats
    double* d_small_d = nullptr;      // 64 doubles
    int* d_small_i = nullptr;
    uint8_t* d_patch = nullptr;       // MAX_WARP^2
    Mem<arucohip_board_t> d_board;    // batched board results + ids
    uint32_t* zero_block = nullptr;   // counters, gen_cnt, trig_cnt, raw_cnt, ring_cnt: zeroed together at the start of a batch
    size_t zero_words = 0;
    Mem<double> d_gl;                 // batched GL modelview matrices
    Mem<uint8_t> d_calib;             // camera calibration: solver state, per-view systems and poses, correspondences (calib_carve)
    Mem<CalibState> hc_calib{true};   // pinned copy of the solver state, read once per iteration
    Batch last;                       // the last batch (kept on the handle the caller holds)
    bool timing = false;
    hipEvent_t ev[TSETS][K_COUNT + 1] = {};
    int tsets = 0;                       // batches recorded since the last reset
    float kernel_ms[K_COUNT] = {};       // averages over the recorded batches
    // Sub-batch pipelining: a batch larger than cap_frames is cut into up to nsub chunks; chunk 0 runs on this handle and
    // the caller's stream, chunk i on chunk worker i (chunk_worker) and its own stream, so the latency-bound kernels of one chunk (border
    // following, Otsu) overlap the bandwidth-bound ones of another and host frames are copied while earlier chunks compute.
    int nsub = 1, cap_frames = 1;        // workers, frames each worker's buffers hold
    std::vector<arucohip_handle*> kids;
    hipEvent_t ev_fork = nullptr, ev_join[MAX_WORKERS] = {};
    hipStream_t side_stream = nullptr;   // late walker generations (k_contours.hip)
    hipEvent_t ev_wfork = nullptr, ev_wjoin = nullptr;
    hipEvent_t ev_thr = nullptr;         // this worker's threshold kernel has finished (staggers the chunks, see detect_batch)
    bool thres_bytes = true;             // buf.thres holds the last batch's byte image (else: tiles + buf.thres_edge, expanded on demand)
    hipEvent_t wait_thr = nullptr;       // set by detect_batch: event the next threshold kernel waits for
    Mem<uint8_t> d_em;                   // arucohip_em_fit scratch, with its own allocation counter (not alloc_epoch)
    uint64_t em_epoch = 0;
    Mem<uint8_t> d_hrm_gen;              // HRM dictionary / board generation scratch (k_hrm.hip), its own counter too (not alloc_epoch)
    uint64_t hrm_epoch = 0;
    int32_t hrm_stats[4] = {};           // the last arucohip_hrm_create_dictionary: windows, host synchronisations, acceptances, tau decrements
    // One frame per call (the reference's call shape, arucohip_detect): the chain of ~20 dependent dispatches of a frame is captured once per
    // (geometry, parameters, camera) into a hipGraph and replayed with ONE launch per call; the frame's H2D copy stays outside (its source
    // pointer changes with every call), the results land in the handle's pinned staging inside the graph.
    struct FrameGraph {
        hipGraphExec_t exec = nullptr;
        uint64_t key = 0;          // digest of everything the captured launches carry by value
        uint64_t seen = 0;         // key of the previous eager call: the second call with the same key captures (buffers are sized by then)
        uint64_t epoch = 0;        // alloc_epoch at the capture: the buffers the launches point into are still the captured ones while it holds
        bool thres_bytes = false;  // what the captured threshold left in buf.thres (a replay sets thres_bytes to it)
        int disabled = 0;          // ARUCOHIP_GRAPH=0, or a capture failed once
    } fgraph;
    // Batches in flight (arucohip_set_pipeline_depth / _submit / _wait): every pipeline lane is a complete worker (own
    // buffers, own stream); ticket t runs on lane t mod depth, so the latency-bound tail of batch t (border following,
    // decoding) overlaps the bandwidth-bound head of batch t+1.
    std::vector<arucohip_handle*> lanes;
    int next_ticket = 0;
    arucohip_handle* retry = nullptr;    // one-frame handle with larger lists for frames that overflowed (arucohip_detect_batch_retry_overflowed)
    int retry_mult = 0;
    hipEvent_t ev_submit = nullptr;
    struct Pending {
        bool active = false;
        int ticket = -1, cap = 0, out_on_device = 0;
        arucohip_marker_t* out = nullptr;
        int32_t* n_out = nullptr;
    } pend;
    std::string err;
};

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
    b.nspan = chunks, b.frames = nframes, b.W = W, b.H = H, b.nthr = nthr;
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

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            char buf_[256];                                                                     \
            snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            (h)->err = buf_;                                                                    \
            return ARUCOHIP_E_HIP;                                                              \
        }                                                                                       \
    } while (0)

static int fail(arucohip_handle* h, int code, const char* msg) {
    if (h) h->err = msg;
    return code;
}

// create-time memory: held by the handle for its whole life, `view` is the pointer the code uses
template <typename T>
static hipError_t hold(arucohip_handle* h, T*& view, size_t bytes, bool pinned = false) {
    Mem<void>& m = h->held.emplace_back(pinned);
    const hipError_t e = m.reserve(bytes, h->alloc_epoch);
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
    if (h->ev_thr) hipEventDestroy(h->ev_thr);
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
        HIPCHK(h, w->d_hrm.reserve((size_t)d.count * sizeof(uint64_t), w->alloc_epoch));
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
        w->decoder_fn = parent->decoder_fn, w->decoder_user = parent->decoder_user;
        w->timing = parent->timing;
        arm_stamps(w, parent->buf.thr_stamp_on != 0);
        return load_dictionary(parent, w, parent->hrm);
    });
}

// is_kid: the handle is one of another's chunk workers and gets none of its own
static int create_handle(const arucohip_params_t* params, int device, const arucohip_limits_t* lim, bool is_kid, arucohip_handle** out);

// a new child of `parent` with limits `lim`, holding the parent's settings (errors are reported on the parent)
static int create_child(arucohip_handle* parent, const arucohip_limits_t& lim, bool is_kid, arucohip_handle** out) {
    int rc = create_handle(&parent->params, parent->device, &lim, is_kid, out);
    if (rc == ARUCOHIP_OK && (rc = inherit(parent, *out)) != ARUCOHIP_OK) {
        arucohip_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

static int create_handle(const arucohip_params_t* params, int device, const arucohip_limits_t* lim, bool is_kid, arucohip_handle** out) {
    if (!out || !lim) return ARUCOHIP_E_INVALID;
    *out = nullptr;
    if (lim->max_width < 32 || lim->max_height < 32 || lim->max_width > 16383 || lim->max_height > 16383 || lim->max_batch < 1 ||
        lim->max_thres_planes < 1 || lim->max_thres_planes > 16 || lim->candidates_per_frame > 512 || lim->markers_per_frame > 256 ||
        (long)lim->max_width * lim->max_height > (1L << 26) /* Quad::key holds a 26-bit raster index */)
        return ARUCOHIP_E_INVALID;
    arucohip_handle* h = new arucohip_handle();
    h->device = device;
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
    {
        // workers: one by default; ARUCOHIP_STREAMS = 2..8 cuts large batches into chunks on separate streams (copies of host
        // frames then overlap the kernels). With the late walker generations on their own side stream a second chunk stream
        // no longer gains anything for device-resident frames (1 stream 208 k fps, 2 streams 208 k at 1024 1080p frames).
        int ns = 1;
        if (const char* es = getenv("ARUCOHIP_STREAMS")) ns = std::min(MAX_WORKERS, std::max(1, atoi(es)));
        if (is_kid) ns = 1;
        h->nsub = std::min(ns, lim->max_batch);
        h->cap_frames = (lim->max_batch + h->nsub - 1) / h->nsub;
    }
    const size_t F = h->cap_frames, P = F * lim->max_thres_planes, px = (size_t)lim->max_width * lim->max_height;
    Buffers& b = h->buf;
    b.tune = read_tuning();
    {
        const char* eg = getenv("ARUCOHIP_GRAPH");
        h->fgraph.disabled = (eg && *eg && atoi(eg) == 0) ? 1 : 0;
    }
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
    ALLOC(b.tile_bits, P * (size_t)tiles_y(lim->max_height) * 2 * tile_strips(lim->max_width) * sizeof(uint64_t));
    h->bits_bytes = bits_bytes;
    ALLOC(b.trig, P * (size_t)b.cap_trig * sizeof(uint2));
    {
        // contour pipeline: ARUCOHIP_CONTOURS = walkers | segments; default by handle shape. The per-candidate walkers win on
        // batches; a single small frame is a chain of up to max-contour dependent border steps for them, which the waypoint
        // segments cut (bench.py latency leg, 1000 calls: 640x480 stills 0.67-0.72 ms vs 0.49-0.52 ms; one 1080p frame 0.80 vs 0.51 since round 4:
        // per-plane workgroup counts scaled for one frame, the run rule read from the lane's block)
        const char* mode = getenv("ARUCOHIP_CONTOURS");
        b.seg_mode = mode ? std::string(mode) == "segments" : (lim->max_batch == 1 && (long)lim->max_width * lim->max_height <= 2048L * 1536L);
        const char* gs = getenv("ARUCOHIP_GRID");
        int grid = gs ? atoi(gs) : 16;
        if (grid != 1 && grid != 2 && grid != 4 && grid != 8 && grid != 16 && grid != 32) grid = 8;
        b.grid_mask = grid - 1;
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
    b.cap_flat = (uint32_t)std::min<size_t>(F * (size_t)std::min(b.cap_cands, 96), 65535u * 16u);
    ALLOC(b.cand_list, (size_t)b.cap_flat * sizeof(uint32_t));
    ALLOC(b.iM, (size_t)b.cap_flat * 9 * sizeof(double));
    ALLOC(b.hist, (size_t)b.cap_flat * 256 * sizeof(uint16_t));
    ALLOC(b.othr, (size_t)b.cap_flat * sizeof(int32_t));
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
    if ((e = hipEventCreateWithFlags(&h->ev_thr, hipEventDisableTiming)) != hipSuccess) return bail(e);
    if ((e = hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e);
    if ((e = hipEventCreateWithFlags(&h->ev_wfork, hipEventDisableTiming)) != hipSuccess) return bail(e);
    if ((e = hipEventCreateWithFlags(&h->ev_wjoin, hipEventDisableTiming)) != hipSuccess) return bail(e);
    if (h->nsub > 1) {
        if ((e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)) != hipSuccess) return bail(e);
        for (int i = 0; i < h->nsub - 1; i++) {
            if ((e = hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming)) != hipSuccess) return bail(e);
            arucohip_limits_t kl = *lim;
            kl.max_batch = h->cap_frames;
            arucohip_handle* kid = nullptr;
            const int krc = create_child(h, kl, true, &kid);
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
    return create_handle(params, device, lim, false, out);
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
static int make_detect_params(arucohip_handle* h, int W, int H, DetectParams* dp) {
    const arucohip_params_t& p = h->params;
    std::memset(dp, 0, sizeof(*dp));
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
    dp->min_contour = (int)(p.min_size * std::max(W, H) * 4);   // :500-501, float arithmetic
    dp->max_contour = (int)(p.max_size * std::max(W, H) * 4);
    if (dp->max_contour > 16383) dp->max_contour = 16383;       // offsets inside a border are 14-bit fields
    // :433-434 Rect(Point(size)*t, Point(size)*(1-t)) with cvRound
    int x1 = (int)lrintf((float)W * p.border_dist), y1 = (int)lrintf((float)H * p.border_dist);
    int x2 = (int)lrintf((float)W * (1.0f - p.border_dist)), y2 = (int)lrintf((float)H * (1.0f - p.border_dist));
    dp->bx0 = std::min(x1, x2), dp->by0 = std::min(y1, y2);
    dp->bx1 = std::max(x1, x2), dp->by1 = std::max(y1, y2);
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
    std::memset(cam, 0, sizeof(*cam));
    if (ndist < 0 || ndist > 8) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0..8");
    cam->has_K = K != nullptr;
    if (K)
        for (int i = 0; i < 9; i++) cam->K[i] = K[i];
    cam->has_dist = dist != nullptr && ndist > 0;
    if (cam->has_dist)
        for (int i = 0; i < ndist; i++) cam->k[i] = (double)dist[i];
    cam->marker_size = marker_size;
    cam->y_perp = y_perp;
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

// the pad word of every bit-image row must be zero; its position depends on the frame width
static int ensure_bits_geometry(arucohip_handle* h, int W, int H) {
    if (h->bits_w == W && h->bits_h == H) return ARUCOHIP_OK;
    HIPCHK(h, hipMemsetAsync(h->buf.tiles, 0, h->bits_bytes, h->stream));
    h->bits_w = W, h->bits_h = H;
    return ARUCOHIP_OK;
}

// the long walks keep their checkpoint rings in HBM; (re)size the space for this batch
static int ensure_walk_scratch(arucohip_handle* h, int nplanes, const DetectParams& dp) {
    size_t need = walk_scratch_words(nplanes, dp, h->buf.long_cap);
    if (need > 0xFFFFFFF0ull) return fail(h, ARUCOHIP_E_CAPACITY, "batch too large for 32-bit checkpoint offsets: fewer frames per batch or a smaller max size");
    HIPCHK(h, h->walk_scratch.reserve(need * sizeof(uint32_t), h->alloc_epoch));
    h->buf.walk_scratch = h->walk_scratch;
    return ARUCOHIP_OK;
}

// Host-side work in front of a batch's enqueued work (detect_core), which a captured graph does not repeat: the eager path and every graph
// replay run it first. In steady state it only compares integers.
static int batch_prologue(arucohip_handle* h, const FrameGeom& g, int nframes, const DetectParams& dp) {
    int rc;
    if ((rc = ensure_walk_scratch(h, nframes * dp.nthr, dp))) return rc;
    if ((rc = ensure_bits_geometry(h, g.width, g.height))) return rc;
    // canonical patches of the decode stage: cap_flat * warp_size^2 bytes
    HIPCHK(h, h->patches.reserve((size_t)h->buf.cap_flat * dp.warp_size * dp.warp_size, h->alloc_epoch));
    h->buf.patches = h->patches;
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
    HIPCHK(h, h->hu_list.reserve((size_t)b.cap_flat * (sizeof(uint32_t) + sizeof(int2) + sizeof(uint32_t)) + sizeof(uint32_t), h->alloc_epoch));
    uint32_t* list = h->hu_list;                                   // [cap_flat] frame << 16 | index
    int2* dec = (int2*)(list + b.cap_flat);                        // [cap_flat] {id, nRotations}
    uint32_t* order = (uint32_t*)(dec + b.cap_flat);               // [cap_flat] + the candidate count behind it
    uint32_t* ncand_p = order + b.cap_flat;
    HIPCHK(h, hipMemcpyAsync(ncand_p, b.counters + CNT_NCAND, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const uint32_t n = std::min(*ncand_p, b.cap_flat);
    if (!n) return ARUCOHIP_OK;
    HIPCHK(h, h->hu_patches.reserve((size_t)n * npx + npx, h->alloc_epoch));
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
    HIPCHK(h, h->d_user_dec.reserve((size_t)b.cap_flat * sizeof(int2), h->alloc_epoch));   // once per handle
    HIPCHK(h, hipMemcpyAsync(h->d_user_dec, dec, n * sizeof(int2), hipMemcpyHostToDevice, s));
    launch_set_decoded(s, b, n, h->d_user_dec);
    // no synchronise: the staging belongs to the handle, and the next call that touches it synchronises the stream first (the count above)
    return ARUCOHIP_OK;
}

static void run_walkers_and_quads(arucohip_handle* h, hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& dp) {
    WalkFork fk{h->buf.tune.walk_fork ? h->side_stream : nullptr, h->ev_wfork, h->ev_wjoin, nullptr};
    const bool forked = launch_walkers(s, fk, g, nframes * dp.nthr, dp, h->buf);
    launch_contour_quads(s, g, nframes, dp, h->buf, forked ? 1 : 0);
    if (forked) {
        (void)hipStreamWaitEvent(s, h->ev_wjoin, 0);
        launch_contour_quads(s, g, nframes, dp, h->buf, 2);
    }
}

// runs kernels 2..8 after the masks and start candidates exist
static void run_rectangles(arucohip_handle* h, const FrameGeom& g, int nframes, const DetectParams& dp) {
    if (h->buf.seg_mode) {
        launch_start_candidates(h->stream, g, nframes * dp.nthr, h->buf);   // also clears the planes' key -> node tables
        launch_segments(h->stream, g, nframes * dp.nthr, dp, h->buf);
    } else {
        launch_start_candidates(h->stream, g, nframes * dp.nthr, h->buf, dp.min_contour);
        run_walkers_and_quads(h, h->stream, g, nframes, dp);
    }
    if (h->buf.seg_mode) launch_contour_quads(h->stream, g, nframes, dp, h->buf);
    launch_frame_candidates(h->stream, g, nframes, dp, h->buf);
}

// threshold stage of any method into buf.thres / buf.tiles (+ bitmap). CANNY (markerdetector.cpp:667-676) blocks the host while its
// hysteresis converges.
// want_bytes: the caller reads buf.thres right away (stage entry point, erosion); otherwise the byte image may be left as tiles + border
// lines (h->thres_bytes says which) and arucohip_get_thresholded expands the plane it is asked for.
static int run_threshold(arucohip_handle* h, hipStream_t s, const uint8_t* gray_dev, const FrameGeom& g, int nframes, const DetectParams& dp, bool want_bytes) {
    const Buffers& b = h->buf;
    h->thres_bytes = true;
    if (dp.thres_method != ARUCOHIP_THRES_CANNY) {
        const bool lazy = launch_threshold(s, gray_dev, g, nframes, dp, b, b.tune.thres_lazy && !want_bytes);
        h->thres_bytes = !lazy;
        return ARUCOHIP_OK;
    }
    const size_t ntiles = (size_t)nframes * dp.nthr * ((g.width + 7) / 8) * ((g.height + 7) / 8);
    HIPCHK(h, h->d_canny.reserve(2 * ntiles * sizeof(uint64_t) + 64, h->alloc_epoch));
    uint64_t* surv = h->d_canny;
    uint64_t* edge = surv + ntiles;
    if (launch_canny(s, gray_dev, g, nframes, dp.nthr, b, surv, edge, (uint32_t*)(edge + ntiles))) return fail(h, ARUCOHIP_E_HIP, "CANNY kernels failed");
    FrameGeom tg = g;
    tg.row_stride = (size_t)g.width, tg.frame_stride = (size_t)g.width * g.height;
    launch_binary_planes(s, b.thres, tg, nframes * dp.nthr, b);   // contour tiles + bitmap from the edge image
    return ARUCOHIP_OK;
}

static int detect_core(arucohip_handle* h, const uint8_t* gray_dev, const FrameGeom& g, int nframes, const DetectParams& dp, const CamModel& cam) {
    hipStream_t s = h->stream;
    Buffers& b = h->buf;
    HIPCHK(h, hipMemsetAsync(h->zero_block, 0, h->zero_words * sizeof(uint32_t), s));
    hipEvent_t* ev = h->ev[h->tsets % TSETS];
    const bool tm = h->timing;
#define MARK(i) do { if (tm) (void)hipEventRecord(ev[i], s); } while (0)
    if (h->wait_thr) HIPCHK(h, hipStreamWaitEvent(s, h->wait_thr, 0));   // threshold kernels of the lanes run one after the other
    MARK(K_THRESHOLD);   // after that wait: the interval is this batch's own threshold kernel
    {
        const int rc_ = run_threshold(h, s, gray_dev, g, nframes, dp, false);
        if (rc_) return rc_;
    }
    if (h->params.erode) {
        // on the bit tiles where the byte image was left out (the default path), on the bytes otherwise
        const bool on_tiles = !h->thres_bytes;
        HIPCHK(h, h->d_erode.reserve(on_tiles ? erode_tiles_tmp_bytes(g, nframes * dp.nthr) : (size_t)nframes * dp.nthr * g.width * g.height, h->alloc_epoch));
        if (on_tiles)
            launch_erode_tiles(s, g, nframes * dp.nthr, b, h->d_erode);
        else
            launch_erode(s, g, nframes * dp.nthr, b, h->d_erode);
    }
    if (h->ev_thr) HIPCHK(h, hipEventRecord(h->ev_thr, s));
    MARK(K_FILTER);
    if (b.seg_mode) {
        launch_start_candidates(s, g, nframes * dp.nthr, b);   // also clears the planes' key -> node tables
        MARK(K_WALKERS);
        launch_segments(s, g, nframes * dp.nthr, dp, b);
        MARK(K_WALKERS_LONG);
        MARK(K_CONTOUR_QUADS);
        launch_contour_quads(s, g, nframes, dp, b);
    } else {
        if (RUN_STAGE(b.tune, 1)) launch_start_candidates(s, g, nframes * dp.nthr, b, dp.min_contour);
        MARK(K_WALKERS);
        // walkers; their late generations run on the side stream under the first quad pass (the contour_quad mark sits at the fork)
        WalkFork fk{b.tune.walk_fork ? h->side_stream : nullptr, h->ev_wfork, h->ev_wjoin, tm ? ev[K_WALKERS_LONG] : nullptr};
        const bool forked = RUN_STAGE(b.tune, 2) ? launch_walkers(s, fk, g, nframes * dp.nthr, dp, b) : false;
        MARK(K_CONTOUR_QUADS);
        if (RUN_STAGE(b.tune, 4)) launch_contour_quads(s, g, nframes, dp, b, forked ? 1 : 0);
        if (forked) {
            HIPCHK(h, hipStreamWaitEvent(s, h->ev_wjoin, 0));
            if (RUN_STAGE(b.tune, 4)) launch_contour_quads(s, g, nframes, dp, b, 2);
        }
    }
    MARK(K_FRAME_CANDS);
    if (RUN_STAGE(b.tune, 5)) launch_frame_candidates(s, g, nframes, dp, b);
    MARK(K_DECODE);
    // built-in 5x5 decoder: the cell votes and the Hamming decode of a candidate are the head of its refinement wave (one dispatch less)
    const bool fused_cells = dp.decoder == ARUCOHIP_DECODER_FIDUCIAL_5X5;
    if (RUN_STAGE(b.tune, 6)) launch_decode(s, gray_dev, g, nframes, dp, b, fused_cells);
    if (dp.decoder == ARUCOHIP_DECODER_USER) {
        const int rc_ = user_decode_stage(h, dp);
        if (rc_) return rc_;
    }
    MARK(K_REFINE_LINES);
    if (RUN_STAGE(b.tune, 7)) launch_refine_lines(s, g, nframes, dp, cam, b, fused_cells);
    MARK(K_REFINE_PIXELS);
    if (dp.corner_method == ARUCOHIP_CORNER_HARRIS || dp.corner_method == ARUCOHIP_CORNER_SUBPIX) {
        if (dp.locked) launch_locked_corners(s, gray_dev, g, nframes, dp, b);   // markerdetector.cpp:398-399
        launch_refine_pixels(s, gray_dev, g, nframes, dp, b);
    }
    MARK(K_FINALIZE);
    if (RUN_STAGE(b.tune, 8)) launch_finalize(s, g, nframes, dp, cam, b, h->wt_out, h->wt_cap, h->wt_n);
    MARK(K_POSE);
    if (RUN_STAGE(b.tune, 8) && cam.has_K && cam.marker_size > 0) launch_pose(s, nframes, cam, b);
    MARK(K_COUNT);
#undef MARK
    if (tm) h->tsets++;
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
            HIPCHK(h, h->d_bgr.reserve((size_t)nframes * W * H * 3, h->alloc_epoch));
            for (int f = 0; f < nframes; f++)
                HIPCHK(h, hipMemcpy2DAsync(h->d_bgr + (size_t)f * W * H * 3, (size_t)W * 3, frames + (size_t)f * frame_stride, row_stride, (size_t)W * 3, H,
                                           hipMemcpyHostToDevice, h->stream));
            bgr = h->d_bgr, rs = (size_t)W * 3, fs = (size_t)W * H * 3;
        }
        HIPCHK(h, h->d_gray.reserve((size_t)nframes * W * H, h->alloc_epoch));
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
    HIPCHK(h, h->d_gray.reserve((size_t)nframes * W * H, h->alloc_epoch));
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

extern "C" {

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

// after the worker's stream has drained: copy the chunk's markers from the pinned staging to the caller's arrays
static int chunk_collect_host(arucohip_handle* h, arucohip_handle* w, int nframes, arucohip_marker_t* out, int cap, int32_t* n_out) {
    int ret = check_status(h, w->h_counters[CNT_STATUS] & ~(uint32_t)ST_MARKER_OVERFLOW);
    const Buffers& b = w->buf;
    for (int f = 0; f < nframes; f++) {
        int n = w->h_n[f];
        n_out[f] = n;
        if (n > cap) {
            if (ret == ARUCOHIP_OK) ret = fail(h, ARUCOHIP_E_CAPACITY, "marker output array too small");
            n = cap;
        }
        n = std::min(n, b.cap_markers);
        if (n > 0) std::memcpy(out + (size_t)f * cap, w->h_markers + (size_t)f * b.cap_markers, (size_t)n * sizeof(arucohip_marker_t));
    }
    return ret;
}

// fork: the other workers' streams wait for what the first worker's stream (the batch's own) has queued so far; errors are reported on h
static int fork_workers(arucohip_handle* h, const Batch& b) {
    if (b.nspan <= 1) return ARUCOHIP_OK;
    arucohip_handle* o = b.span[0].w;
    HIPCHK(h, hipEventRecord(o->ev_fork, o->stream));
    for (int c = 1; c < b.nspan; c++) HIPCHK(h, hipStreamWaitEvent(b.span[c].w->stream, o->ev_fork, 0));
    return ARUCOHIP_OK;
}
// join: the first worker's stream waits for the others
static int join_workers(arucohip_handle* h, const Batch& b) {
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
        int r = chunk_collect_host(h, s.w, s.count, out + (size_t)s.first * cap, cap, n_out + s.first);
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
    if (h->fgraph.disabled || h->timing || dp.decoder == ARUCOHIP_DECODER_USER || dp.thres_method == ARUCOHIP_THRES_CANNY || h->params.erode) return ARUCOHIP_OK;
    uint64_t key = 1469598103934665603ull;
    const int geo[4] = {W, H, channels, (int)h->buf.seg_mode};
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
    if (h->fgraph.exec && h->fgraph.epoch != h->alloc_epoch) {   // a buffer was replaced since the capture: start over, like a new configuration
        (void)hipGraphExecDestroy(h->fgraph.exec);
        h->fgraph.exec = nullptr, h->fgraph.seen = key;
        return ARUCOHIP_OK;   // the frame is staged; the eager path stages it again, which is harmless
    }
    if (!h->fgraph.exec) {
        const uint64_t epoch = h->alloc_epoch;
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
        if (rc != ARUCOHIP_OK || e != hipSuccess || e2 != hipSuccess || !graph || h->alloc_epoch != epoch ||
            hipGraphInstantiate(&h->fgraph.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (graph) (void)hipGraphDestroy(graph);
            h->fgraph.exec = nullptr, h->fgraph.disabled = 1;   // this handle stays on the eager path
            return ARUCOHIP_OK;
        }
        (void)hipGraphDestroy(graph);
        h->fgraph.key = key, h->fgraph.epoch = epoch, h->fgraph.thres_bytes = h->thres_bytes;
    }
    *handled = true;
    HIPCHK(h, hipGraphLaunch(h->fgraph.exec, h->stream));
    h->thres_bytes = h->fgraph.thres_bytes;
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
    if ((rc = make_detect_params(h, W, H, &dp))) return rc;
    if ((rc = make_cam(h, K, dist, ndist, marker_size, y_perp, &cam))) return rc;
    if (nframes == 1 && !frames_on_device && !out_on_device && !defer && h->nsub == 1) {
        bool handled = false;
        rc = detect_one_graphed(h, frames, W, H, row_stride, channels, dp, cam, out, cap, n_out, &handled);
        if (handled) return rc;
    }
    h->last = plan_batch(h, nframes, W, H, dp.nthr);
    const Batch& plan = h->last;
    if ((rc = fork_workers(h, plan))) return rc;
    for (int c = 0; c < plan.nspan; c++) {
        const Span& s = plan.span[c];
        // optional stagger (ARUCOHIP_CHAIN=1): the bandwidth-bound threshold kernels of the chunks run one after the other,
        // so that chunk c's threshold overlaps the latency-bound border following / decoding of chunk c-1. Helps with 4
        // streams on some boxes and hurts on others, hence off by default.
        const bool chain = h->buf.tune.chain != 0;
        s.w->wait_thr = (chain && c > 0) ? plan.span[c - 1].w->ev_thr : nullptr;
        rc = chunk_enqueue(s.w, frames + (size_t)s.first * frame_stride, s.count, W, H, row_stride, frame_stride, frames_on_device, channels, dp, cam,
                           out ? out + (size_t)s.first * cap : nullptr, cap, n_out + s.first, out_on_device);
        if (rc) {
            if (s.w != h) h->err = s.w->err;
            // the workers that already have queued work still have to rejoin the caller's stream
            const std::string keep = h->err;
            (void)join_workers(h, plan);
            for (const Span& x : plan) x.w->wait_thr = nullptr;
            h->err = keep;
            h->last = Batch{};   // the lists hold part of a batch
            return rc;
        }
    }
    if ((rc = join_workers(h, plan))) return rc;
    if (out_on_device || defer) return ARUCOHIP_OK;
    return collect_batch_host(h, out, cap, n_out);
}

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
        HIPCHK(h, h->d_umap_xy.reserve(px * sizeof(short2), h->alloc_epoch));
        HIPCHK(h, h->d_umap_f.reserve(px * sizeof(uint16_t), h->alloc_epoch));
        launch_undist_map(s, W, H, K, dist, ndist, h->d_umap_xy, h->d_umap_f);
        HIPCHK(h, hipGetLastError());
        h->umap_w = W, h->umap_h = H, h->umap_nd = ndist;
        std::memcpy(h->umap_K, K, sizeof(h->umap_K));
        if (ndist) std::memcpy(h->umap_d, dist, ndist * sizeof(float));
    }
    const size_t fbytes = (size_t)W * H * channels;
    const uint8_t* sdev = src;
    size_t rs = row_stride, fs = frame_stride;
    if (!src_on_device) {
        HIPCHK(h, h->d_bgr.reserve((size_t)nframes * fbytes, h->alloc_epoch));
        for (int f = 0; f < nframes; f++)
            HIPCHK(h, hipMemcpy2DAsync(h->d_bgr + (size_t)f * fbytes, (size_t)W * channels, src + (size_t)f * frame_stride, row_stride, (size_t)W * channels, H,
                                       hipMemcpyHostToDevice, s));
        sdev = h->d_bgr, rs = (size_t)W * channels, fs = fbytes;
    }
    uint8_t* ddev = dst;
    if (!dst_on_device) {
        HIPCHK(h, h->d_undist.reserve((size_t)nframes * fbytes, h->alloc_epoch));
        ddev = h->d_undist;
    }
    launch_remap(s, sdev, rs, fs, W, H, channels, nframes, h->d_umap_xy, h->d_umap_f, ddev);
    HIPCHK(h, hipGetLastError());
    if (!dst_on_device) {
        HIPCHK(h, hipMemcpyAsync(dst, ddev, (size_t)nframes * fbytes, hipMemcpyDeviceToHost, s));
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

int arucohip_get_thresholded(arucohip_handle* h0, int frame, uint8_t* dst) {
    if (!h0 || !dst) return ARUCOHIP_E_INVALID;
    const Batch& r = h0->last;
    arucohip_handle* h = r.holder(frame, &frame);
    if (!h) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    size_t px = (size_t)r.W * r.H;
    int plane = frame * r.nthr + r.nthr / 2;   // thres = thres_images[n_param1 / 2]
    if (!h->thres_bytes) {   // the batch kept the image as tiles + border lines: rebuild this plane's bytes
        FrameGeom g;
        g.width = r.W, g.height = r.H, g.row_stride = (size_t)r.W, g.frame_stride = px;
        launch_expand_thres(h->stream, g, plane, h->buf);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(dst, h->buf.thres + plane * px, px, hipMemcpyDeviceToHost, h->stream));
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
        uint32_t n = 0;
        HIPCHK(h, hipMemcpyAsync(&n, h->buf.trig_cnt + (size_t)plane * TRIG_CNT_STRIDE + TC_CDESC, sizeof(n), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        n = std::min(n, h->buf.cap_cdesc);
        if (!n) continue;
        const size_t at = all.size();
        all.resize(at + n);
        HIPCHK(h, hipMemcpyAsync(all.data() + at, h->buf.cdesc + (size_t)plane * h->buf.cap_cdesc, n * sizeof(ContourDesc), hipMemcpyDeviceToHost, h->stream));
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

int arucohip_debug_counters(arucohip_handle* h, uint32_t* out8) {
    if (!h || !out8) return ARUCOHIP_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    const Batch& r = h->last;
    uint64_t acc[CNT_FIXED] = {};
    uint64_t ntrig = 0, nraw = 0, nlong = 0;
    for (const Span& s : r) {
        arucohip_handle* w = s.w;
        uint32_t cnt[CNT_FIXED];
        HIPCHK(h, hipMemcpyAsync(cnt, w->buf.counters, sizeof(cnt), hipMemcpyDeviceToHost, w->stream));
        const int planes = s.count * r.nthr;
        std::vector<uint32_t> tc((size_t)planes * TRIG_CNT_STRIDE), rc_((size_t)planes * TRIG_CNT_STRIDE), rg((size_t)planes * TRIG_CNT_STRIDE);
        HIPCHK(h, hipMemcpyAsync(tc.data(), w->buf.trig_cnt, tc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(rc_.data(), w->buf.raw_cnt, rc_.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(rg.data(), w->buf.ring_cnt, rg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipStreamSynchronize(w->stream));
        for (int i = 0; i < CNT_FIXED; i++)
            if (i != 1 && i != 2) acc[i] = (i == CNT_STATUS) ? (acc[i] | cnt[i]) : acc[i] + cnt[i];   // [1], [2] come from the planes' own counters below
        for (int p = 0; p < planes; p++) {
            ntrig += tc[(size_t)p * TRIG_CNT_STRIDE] + tc[(size_t)p * TRIG_CNT_STRIDE + 1];
            acc[1] += tc[(size_t)p * TRIG_CNT_STRIDE + TC_CDESC], acc[2] += tc[(size_t)p * TRIG_CNT_STRIDE + TC_POOL];
            nraw += rc_[(size_t)p * TRIG_CNT_STRIDE];
            nlong += rg[(size_t)p * TRIG_CNT_STRIDE] + rg[(size_t)p * TRIG_CNT_STRIDE + 1];
        }
    }
    for (int i = 0; i < CNT_FIXED; i++) out8[i] = (uint32_t)std::min<uint64_t>(acc[i], 0xFFFFFFFFu);
    out8[0] = (uint32_t)std::min<uint64_t>(ntrig, 0xFFFFFFFFu);   // start candidates after the run rule (all planes)
    const bool seg = r.nspan > 0 && r.span[0].w->buf.seg_mode;
    out8[4] = (uint32_t)std::min<uint64_t>(seg ? nraw : nlong, 0xFFFFFFFFu);   // waypoint records (segment mode) / long walks = checkpoint rings handed out
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
    run_rectangles(h, g, 1, dp);
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
    // every worker solves the boards of the frames it detected, on its own stream
    const Batch b = h->last.cut(nframes);
    if ((rc = fork_workers(h, b))) return rc;
    for (const Span& s : b) {
        arucohip_handle* w = s.w;
        HIPCHK(h, w->d_board.reserve((size_t)w->cap_frames * (sizeof(arucohip_board_t) + sizeof(float)) + 8192 * sizeof(int32_t), w->alloc_epoch));
        arucohip_board_t* d_out = w->d_board;
        float* d_prob = (float*)(d_out + w->cap_frames);
        int32_t* d_ids = (int32_t*)(d_prob + w->cap_frames);
        HIPCHK(h, hipMemcpyAsync(d_ids, ids, (size_t)nboard * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
        HIPCHK(h, hipMemcpyAsync(w->d_small_f, obj, (size_t)nboard * 12 * sizeof(float), hipMemcpyHostToDevice, w->stream));
        launch_board_pose(w->stream, s.count, w->buf, d_ids, w->d_small_f, nboard, info_type, marker_size, repj_err_thres, cam, d_out, d_prob);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out + s.first, d_out, (size_t)s.count * sizeof(arucohip_board_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(h, hipMemcpyAsync(prob + s.first, d_prob, (size_t)s.count * sizeof(float), hipMemcpyDeviceToHost, w->stream));
    }
    if ((rc = join_workers(h, b))) return rc;
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

// ---- camera calibration (k_calib.hip) ----
// Byte offsets into h->d_calib for V views, npts points, nframes gather slots and a board of nboard markers.
struct CalibCarve {
    size_t st, off, npt, init, red, bs, pose, vcost, vchg, obj, img, nmark, bids, bobj, total;
};
static CalibCarve calib_carve(int V, size_t npts, int nframes, int nboard) {
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

// Levenberg-Marquardt on views whose points are already on the device (d.obj / d.img, offsets off[], counts npt[]): start values, then
// one host synchronisation per iteration for the stop flag.
static int calib_solve(arucohip_handle* h, CalibDev d, const CalibCarve& c, const std::vector<int32_t>& off, const std::vector<int32_t>& npt,
                       int W, int H, int flags, double* K, double* dist, double* rvecs, double* tvecs, double* per_view_rms, double* rms) {
    const int V = d.nviews;
    uint8_t* base = h->d_calib;
    d.off = (const int32_t*)(base + c.off), d.npt = (const int32_t*)(base + c.npt);
    d.init = (double*)(base + c.init), d.red = (double*)(base + c.red), d.bs = (double*)(base + c.bs);
    d.pose = (double*)(base + c.pose), d.vcost = (double*)(base + c.vcost), d.vchg = (double*)(base + c.vchg);
    d.st = (CalibState*)(base + c.st);
    const bool guess = flags & ARUCOHIP_CALIB_USE_INTRINSIC_GUESS;
    CalibState st;
    std::memset(&st, 0, sizeof(st));
    st.flags = flags, st.max_iter = 30, st.lg = -3;
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
    hipStream_t s = h->stream;
    HIPCHK(h, h->hc_calib.reserve(sizeof(CalibState), h->alloc_epoch));
    CalibState* hs = h->hc_calib;
    *hs = st;
    HIPCHK(h, hipMemcpyAsync(d.st, hs, sizeof(st), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync((void*)d.off, off.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync((void*)d.npt, npt.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, s));
    launch_calib_init(s, d, guess);
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
    const double* in = st.intr;
    const double Ko[9] = {in[0], 0, in[2], 0, in[1], in[3], 0, 0, 1};
    for (int i = 0; i < 9; i++) K[i] = Ko[i];
    for (int i = 0; i < 5; i++) dist[i] = in[4 + i];
    double e2 = 0, np = 0;
    for (int v = 0; v < V; v++) {
        e2 += vcost[v], np += npt[v];
        if (per_view_rms) per_view_rms[v] = std::sqrt(vcost[v] / npt[v]);
        for (int k = 0; k < 3; k++) {
            if (rvecs) rvecs[3 * v + k] = pose[6 * v + k];
            if (tvecs) tvecs[3 * v + k] = pose[6 * v + 3 + k];
        }
    }
    if (rms) *rms = std::sqrt(e2 / np);
    return ARUCOHIP_OK;
}

int arucohip_calibrate_camera(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, int W,
                              int H, int flags, double* K, double* dist, double* rvecs, double* tvecs, double* per_view_rms, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!obj || !img || !npoints || !K || !dist || nviews < 1 || W <= 0 || H <= 0)
        return fail(h, ARUCOHIP_E_INVALID, "calibrate_camera: NULL argument, no views or an empty image size");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int32_t> npt((size_t)nviews), off((size_t)nviews);
    if (on_device)
        HIPCHK(h, hipMemcpy(npt.data(), npoints, (size_t)nviews * sizeof(int32_t), hipMemcpyDeviceToHost));
    else
        std::memcpy(npt.data(), npoints, (size_t)nviews * sizeof(int32_t));
    size_t total = 0;
    for (int v = 0; v < nviews; v++) {
        if (npt[v] < 4) return fail(h, ARUCOHIP_E_INVALID, "a calibration view has fewer than 4 points");
        if (npt[v] > CALIB_MAX_POINTS) return fail(h, ARUCOHIP_E_CAPACITY, "a calibration view has more than ARUCOHIP_CALIB_MAX_VIEW_POINTS points");
        off[v] = (int32_t)total, total += (size_t)npt[v];
    }
    if (total > (size_t)INT32_MAX) return fail(h, ARUCOHIP_E_CAPACITY, "too many calibration points");
    const CalibCarve c = calib_carve(nviews, on_device ? 0 : total, 0, 0);
    HIPCHK(h, h->d_calib.reserve(c.total, h->alloc_epoch));
    CalibDev d{};
    d.nviews = nviews;
    if (on_device) {
        d.obj = obj, d.img = img;
    } else {
        float* dobj = (float*)((uint8_t*)h->d_calib + c.obj);
        float* dimg = (float*)((uint8_t*)h->d_calib + c.img);
        HIPCHK(h, hipMemcpyAsync(dobj, obj, total * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(dimg, img, total * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        d.obj = dobj, d.img = dimg;
    }
    return calib_solve(h, d, c, off, npt, W, H, flags, K, dist, rvecs, tvecs, per_view_rms, rms);
}

int arucohip_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                   float marker_size, int min_markers, int W, int H, int flags, double* K, double* dist, int32_t* used,
                                   double* rvecs, double* tvecs, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!K || !dist || W <= 0 || H <= 0) return fail(h, ARUCOHIP_E_INVALID, "calibrate_board_batch: NULL K / dist or an empty image size");
    if (nboard <= 0 || !ids || !obj) return fail(h, ARUCOHIP_E_BOARD_CONFIG, "invalid BoardConfig that is empty");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    arucohip_handle* o = b.span[0].w;   // the worker of the batch's first chunk: the calibration runs on its stream, in its scratch
    // the metres-per-unit factor of board_pose_kernel for PIX boards (marker side from the first edge of marker 0)
    const float dx = obj[0] - obj[3], dy = obj[1] - obj[4], dz = obj[2] - obj[5];
    const double side = std::sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    const double mpp = (info_type == ARUCOHIP_BOARD_PIX && marker_size > 0) ? (double)marker_size / side : 1.0;
    const CalibCarve c = calib_carve(nframes, (size_t)nframes * CALIB_MAX_POINTS, nframes, nboard);
    HIPCHK(h, o->d_calib.reserve(c.total, o->alloc_epoch));
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
    std::vector<int32_t> off, npt;
    for (int f = 0; f < nframes; f++) {
        const bool take = fnmark[f] >= std::max(min_markers, 1) && fnpt[f] != 0;
        if (take && fnpt[f] < 0) return fail(h, ARUCOHIP_E_CAPACITY, "a frame has more board points than ARUCOHIP_CALIB_MAX_VIEW_POINTS");
        if (used) used[f] = take ? 1 : 0;
        if (take) off.push_back(f * CALIB_MAX_POINTS), npt.push_back(fnpt[f]);
    }
    if (off.empty()) return fail(h, ARUCOHIP_E_INVALID, "no frame holds min_markers board markers");
    CalibDev d{};
    d.nviews = (int)off.size(), d.obj = dobj, d.img = dimg;
    // the per-view arrays are carved for nframes >= views; the off / npt arrays are rewritten with the views
    rc = calib_solve(o, d, c, off, npt, W, H, flags, K, dist, rvecs, tvecs, nullptr, rms);
    if (rc && o != h) h->err = o->err;
    return rc;
}

// ---- board occlusion mask (k_chromatic.hip) ----
// The object's buffers are its own (Mem with its own counter, never the handle's alloc_epoch): a chromatic call cannot invalidate the
// handle's single-frame graph. Calls run on the handle's current stream and return after it has drained.
struct arucohip_chromatic {
    arucohip_handle* h = nullptr;
    int device = 0;           // destroy() may run after the handle's
    ChromaCam cam{};
    int ncell = 0;
    double thresh = 0;
    bool valid = false;       // isValid(): a train has run
    int last_batch = 0;       // frames of the last classify_batch (debug_geometry)
    uint64_t epoch = 0;       // the object's own allocation counter
    Mem<uint8_t> d_frame, d_cellmap, d_mask, d_inside, d_bframes, d_bmasks;
    Mem<uint32_t> d_raw, d_hcount;
    Mem<int32_t> d_fitted, d_trained, d_npix;
    Mem<double> d_prob;
    Mem<ChromaGeom> d_geom, d_bgeom;
};

// setParams(mc, nc, threshProb, CP, BC, markersize), src/chromaticmask.cpp:122-165: the min / max scan (x <= min.x && y <= min.y), the
// pixel size from the first edge of marker 0, then min and max scaled in x and y (z as found)
int arucohip_chromatic_board_corners(const float* obj, int nboard, int info_type, float marker_size, float corners[12]) {
    if (!obj || !corners || nboard < 1) return ARUCOHIP_E_INVALID;
    if (info_type != ARUCOHIP_BOARD_METERS && marker_size == -1) return ARUCOHIP_E_INVALID;
    auto P = [&](int i, int j) { return obj + ((size_t)i * 4 + j) * 3; };
    if (info_type == ARUCOHIP_BOARD_METERS) {   // cv::norm(objPoints[0][0] - objPoints[0][1])
        const float dx = P(0, 0)[0] - P(0, 1)[0], dy = P(0, 0)[1] - P(0, 1)[1], dz = P(0, 0)[2] - P(0, 1)[2];
        marker_size = (float)std::sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    }
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) mn[k] = mx[k] = P(0, 0)[k];
    for (int i = 0; i < nboard; i++)
        for (int j = 0; j < 4; j++) {
            const float* p = P(i, j);
            if (p[0] <= mn[0] && p[1] <= mn[1]) mn[0] = p[0], mn[1] = p[1], mn[2] = p[2];
            if (p[0] >= mx[0] && p[1] >= mx[1]) mx[0] = p[0], mx[1] = p[1], mx[2] = p[2];
        }
    const double pix = std::fabs(marker_size / (P(0, 1)[0] - P(0, 0)[0]));
    mn[0] = (float)(mn[0] * pix), mn[1] = (float)(mn[1] * pix);
    mx[0] = (float)(mx[0] * pix), mx[1] = (float)(mx[1] * pix);
    const float c[12] = {mn[0], mn[1], mn[2], mn[0], mx[1], 0, mx[0], mx[1], mx[2], mx[0], mn[1], 0};
    for (int i = 0; i < 12; i++) corners[i] = c[i];
    return ARUCOHIP_OK;
}

int arucohip_chromatic_create(arucohip_handle* h, int mc, int nc, double thresh_prob, const float* K, const float* dist, int ndist, int W, int H,
                              const float corners[12], arucohip_chromatic** out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!out || !K || !corners || W <= 0 || H <= 0 || ndist < 0 || ndist > 8 || (ndist > 0 && !dist))
        return fail(h, ARUCOHIP_E_INVALID, "chromatic_create: NULL argument, empty frame size or ndist outside 0..8");
    *out = nullptr;
    if (mc <= 0 || nc <= 0 || nc > mc || mc * nc > 255)
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "chromatic_create: needs 1 <= nc <= mc and mc * nc <= 255 (other grids are undefined in the reference)");
    HIPCHK(h, hipSetDevice(h->device));
    std::unique_ptr<arucohip_chromatic> m(new arucohip_chromatic());
    m->h = h, m->device = h->device, m->ncell = mc * nc, m->thresh = thresh_prob;
    ChromaCam& c = m->cam;
    for (int i = 0; i < 9; i++) c.K[i] = K[i];
    for (int i = 0; i < 8; i++) c.k[i] = i < ndist ? (double)dist[i] : 0.0;
    for (int i = 0; i < 12; i++) c.corners3d[i] = corners[i];
    c.mc = mc, c.nc = nc, c.W = W, c.H = H;
    const size_t px = (size_t)W * H, tab = (size_t)m->ncell * 256;
    uint64_t& e = m->epoch;
    HIPCHK(h, m->d_frame.reserve(px, e));
    HIPCHK(h, m->d_cellmap.reserve(px, e));
    HIPCHK(h, m->d_mask.reserve(px, e));
    HIPCHK(h, m->d_raw.reserve(tab * sizeof(uint32_t), e));
    HIPCHK(h, m->d_hcount.reserve(tab * sizeof(uint32_t), e));
    HIPCHK(h, m->d_fitted.reserve(m->ncell * sizeof(int32_t), e));
    HIPCHK(h, m->d_trained.reserve(m->ncell * sizeof(int32_t), e));
    HIPCHK(h, m->d_prob.reserve(tab * sizeof(double), e));
    HIPCHK(h, m->d_inside.reserve(tab, e));
    HIPCHK(h, m->d_geom.reserve(sizeof(ChromaGeom), e));
    // a fresh EMClassifier: _prob = 0.5, and _inside (uninitialised in the reference) = 0.5 > threshProb
    std::vector<double> p(tab, 0.5);
    std::vector<uint8_t> in(tab, 0.5 > thresh_prob ? 1 : 0);
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(m->d_cellmap, 0, px, s));
    HIPCHK(h, hipMemsetAsync(m->d_mask, 0, px, s));
    HIPCHK(h, hipMemsetAsync(m->d_raw, 0, tab * sizeof(uint32_t), s));
    HIPCHK(h, hipMemsetAsync(m->d_hcount, 0, tab * sizeof(uint32_t), s));
    HIPCHK(h, hipMemsetAsync(m->d_fitted, 0, m->ncell * sizeof(int32_t), s));
    HIPCHK(h, hipMemsetAsync(m->d_trained, 0, m->ncell * sizeof(int32_t), s));
    HIPCHK(h, hipMemsetAsync(m->d_geom, 0, sizeof(ChromaGeom), s));
    HIPCHK(h, hipMemcpyAsync(m->d_prob, p.data(), tab * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(m->d_inside, in.data(), tab, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *out = m.release();
    return ARUCOHIP_OK;
}

void arucohip_chromatic_destroy(arucohip_chromatic* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

// the plane on the device: the caller's, or a copy into the object's staging
static int chroma_plane(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride, const uint8_t** dev, size_t* dev_stride) {
    arucohip_handle* h = m->h;
    if (!plane || row_stride < (size_t)m->cam.W) return fail(h, ARUCOHIP_E_INVALID, "chromatic: NULL plane or row stride below the width");
    HIPCHK(h, hipSetDevice(h->device));
    if (on_device) {
        *dev = plane, *dev_stride = row_stride;
        return ARUCOHIP_OK;
    }
    HIPCHK(h, hipMemcpy2DAsync(m->d_frame, m->cam.W, plane, row_stride, m->cam.W, m->cam.H, hipMemcpyHostToDevice, h->stream));
    *dev = m->d_frame, *dev_stride = m->cam.W;
    return ARUCOHIP_OK;
}

// one frame's raw-sample histograms (under the mask for update) and the EM of every cell
static int chroma_fit(arucohip_chromatic* m, const uint8_t* in, size_t stride, const uint8_t* mask, uint32_t min_raw) {
    arucohip_handle* h = m->h;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(m->d_raw, 0, (size_t)m->ncell * 256 * sizeof(uint32_t), s));
    launch_chroma_hist(s, m->cam.W, m->cam.H, in, stride, m->d_cellmap, mask, m->d_raw);
    launch_chroma_em(s, m->ncell, m->d_raw, min_raw, m->thresh, m->d_hcount, m->d_fitted, m->d_prob, m->d_inside, m->d_trained);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_chromatic_train(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride, const double rvec[3], const double tvec[3]) {
    if (!m) return ARUCOHIP_E_INVALID;
    if (!rvec || !tvec) return fail(m->h, ARUCOHIP_E_INVALID, "chromatic_train: NULL pose");
    const uint8_t* in;
    size_t stride;
    int rc = chroma_plane(m, plane, on_device, row_stride, &in, &stride);
    if (rc) return rc;
    hipStream_t s = m->h->stream;
    launch_chroma_geometry(s, m->cam, 1, nullptr, nullptr, 0.f, rvec, tvec, m->d_geom);
    launch_chroma_grid(s, m->cam, m->d_geom, m->d_cellmap);
    if ((rc = chroma_fit(m, in, stride, nullptr, 0))) return rc;
    m->valid = true;
    return ARUCOHIP_OK;
}

int arucohip_chromatic_classify(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride, const double rvec[3], const double tvec[3],
                                int method) {
    if (!m) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = m->h;
    if (!rvec || !tvec) return fail(h, ARUCOHIP_E_INVALID, "chromatic_classify: NULL pose");
    if (method != 1 && method != 2) return fail(h, ARUCOHIP_E_INVALID, "chromatic_classify: method is 1 (classify) or 2 (classify2)");
    const uint8_t* in;
    size_t stride;
    int rc = chroma_plane(m, plane, on_device, row_stride, &in, &stride);
    if (rc) return rc;
    hipStream_t s = h->stream;
    launch_chroma_geometry(s, m->cam, 1, nullptr, nullptr, 0.f, rvec, tvec, m->d_geom);
    if (method == 1) launch_chroma_grid(s, m->cam, m->d_geom, m->d_cellmap);   // classify refreshes the cell map, classify2 does not
    launch_chroma_classify(s, m->cam, method, m->thresh, 1, in, stride, 0, m->d_geom, m->d_prob, m->d_inside, m->d_mask, nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_chromatic_update(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride) {
    if (!m) return ARUCOHIP_E_INVALID;
    const uint8_t* in;
    size_t stride;
    int rc = chroma_plane(m, plane, on_device, row_stride, &in, &stride);
    if (rc) return rc;
    return chroma_fit(m, in, stride, m->d_mask, CHROMA_UPDATE_MIN);
}

// calculateGridImage(board) on its own (:222-268): the geometry of the pose and the cell map
int arucohip_chromatic_grid(arucohip_chromatic* m, const double rvec[3], const double tvec[3]) {
    if (!m) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = m->h;
    if (!rvec || !tvec) return fail(h, ARUCOHIP_E_INVALID, "chromatic_grid: NULL pose");
    HIPCHK(h, hipSetDevice(h->device));
    launch_chroma_geometry(h->stream, m->cam, 1, nullptr, nullptr, 0.f, rvec, tvec, m->d_geom);
    launch_chroma_grid(h->stream, m->cam, m->d_geom, m->d_cellmap);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_chromatic_reset_mask(arucohip_chromatic* m) {
    if (!m) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = m->h;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(m->d_mask, 0, (size_t)m->cam.W * m->cam.H, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

static int chroma_copy_out(arucohip_chromatic* m, const void* src, void* dst, size_t bytes, int on_device) {
    arucohip_handle* h = m->h;
    if (!dst) return fail(h, ARUCOHIP_E_INVALID, "chromatic: NULL destination");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

int arucohip_chromatic_get_mask(arucohip_chromatic* m, uint8_t* dst, int on_device) {
    if (!m) return ARUCOHIP_E_INVALID;
    return chroma_copy_out(m, m->d_mask, dst, (size_t)m->cam.W * m->cam.H, on_device);
}

int arucohip_chromatic_get_cell_map(arucohip_chromatic* m, uint8_t* dst, int on_device) {
    if (!m) return ARUCOHIP_E_INVALID;
    return chroma_copy_out(m, m->d_cellmap, dst, (size_t)m->cam.W * m->cam.H, on_device);
}

int arucohip_chromatic_is_valid(arucohip_chromatic* m) { return m && m->valid ? 1 : 0; }

int arucohip_chromatic_get_model(arucohip_chromatic* m, double* prob, int32_t* trained) {
    if (!m) return ARUCOHIP_E_INVALID;
    if (!prob || !trained) return fail(m->h, ARUCOHIP_E_INVALID, "chromatic_get_model: NULL argument");
    int rc = chroma_copy_out(m, m->d_prob, prob, (size_t)m->ncell * 256 * sizeof(double), 0);
    return rc ? rc : chroma_copy_out(m, m->d_trained, trained, (size_t)m->ncell * sizeof(int32_t), 0);
}

int arucohip_chromatic_set_model(arucohip_chromatic* m, const double* prob, const int32_t* trained) {
    if (!m) return ARUCOHIP_E_INVALID;
    arucohip_handle* h = m->h;
    if (!prob || !trained) return fail(h, ARUCOHIP_E_INVALID, "chromatic_set_model: NULL argument");
    const size_t tab = (size_t)m->ncell * 256;
    std::vector<uint8_t> in(tab);
    for (size_t i = 0; i < tab; i++) in[i] = prob[i] > m->thresh ? 1 : 0;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(m->d_prob, prob, tab * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(m->d_inside, in.data(), tab, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(m->d_trained, trained, (size_t)m->ncell * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ARUCOHIP_OK;
}

// EMClassifier::train of one cell by chroma_em_kernel, in a small scratch of the handle's that is outside alloc_epoch
int arucohip_em_fit(arucohip_handle* h, const uint32_t samples_hist[256], double thresh_prob, double prob[256], uint8_t inside[256], int* trained) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!samples_hist || !prob || !inside || !trained) return fail(h, ARUCOHIP_E_INVALID, "em_fit: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t o_hc = 1024, o_fit = 2048, o_tr = 2056, o_prob = 2064, o_in = o_prob + 2048, total = o_in + 256;
    HIPCHK(h, h->d_em.reserve(total, h->em_epoch));   // kept for the handle's life; never moves alloc_epoch
    uint8_t* b = h->d_em;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(b, samples_hist, 1024, hipMemcpyHostToDevice, s));
    launch_chroma_em(s, 1, (const uint32_t*)b, 0, thresh_prob, (uint32_t*)(b + o_hc), (int32_t*)(b + o_fit), (double*)(b + o_prob), b + o_in,
                     (int32_t*)(b + o_tr));
    HIPCHK(h, hipGetLastError());
    int32_t fitted = 0;
    HIPCHK(h, hipMemcpyAsync(&fitted, b + o_fit, sizeof(fitted), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *trained = fitted == 1;
    if (fitted == 1) {
        HIPCHK(h, hipMemcpyAsync(prob, b + o_prob, 256 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(inside, b + o_in, 256, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    return ARUCOHIP_OK;
}

int arucohip_chromatic_debug_geometry(arucohip_chromatic* m, int frame, float corners2d[8], double H_train[9], double H_classify[9]) {
    if (!m) return ARUCOHIP_E_INVALID;
    if (frame >= m->last_batch) return fail(m->h, ARUCOHIP_E_INVALID, "chromatic_debug_geometry: frame outside the last batch");
    ChromaGeom g;
    int rc = chroma_copy_out(m, frame < 0 ? (const ChromaGeom*)m->d_geom : (const ChromaGeom*)m->d_bgeom + frame, &g, sizeof(g), 0);
    if (rc) return rc;
    for (int i = 0; i < 9; i++) {
        if (corners2d && i < 8) corners2d[i] = g.corners[i];
        if (H_train) H_train[i] = g.Ht[i];
        if (H_classify) H_classify[i] = g.Hc[i];
    }
    return ARUCOHIP_OK;
}

int arucohip_chromatic_debug_hist(arucohip_chromatic* m, uint32_t* raw, uint32_t* hist_count, int32_t* fitted) {
    if (!m) return ARUCOHIP_E_INVALID;
    const size_t tab = (size_t)m->ncell * 256;
    int rc = raw ? chroma_copy_out(m, m->d_raw, raw, tab * sizeof(uint32_t), 0) : 0;
    if (!rc && hist_count) rc = chroma_copy_out(m, m->d_hcount, hist_count, tab * sizeof(uint32_t), 0);
    if (!rc && fitted) rc = chroma_copy_out(m, m->d_fitted, fitted, (size_t)m->ncell * sizeof(int32_t), 0);
    return rc;
}

int arucohip_chromatic_classify_batch(arucohip_chromatic* m, arucohip_handle* h, const uint8_t* frames, int nframes, int W, int H, size_t row_stride,
                                      size_t frame_stride, int frames_on_device, int method, float min_prob, uint8_t* masks, int masks_on_device,
                                      int32_t* npix) {
    if (!m) return ARUCOHIP_E_INVALID;
    arucohip_handle* mh = m->h;
    if (!h || !frames || !masks || nframes < 1) return fail(mh, ARUCOHIP_E_INVALID, "chromatic_classify_batch: NULL argument or no frames");
    if (W != m->cam.W || H != m->cam.H || row_stride < (size_t)W || frame_stride < row_stride * (H - 1) + W)
        return fail(mh, ARUCOHIP_E_INVALID, "chromatic_classify_batch: frame size differs from the object's, or strides too small");
    if (method != 1 && method != 2) return fail(mh, ARUCOHIP_E_INVALID, "chromatic_classify_batch: method is 1 (classify) or 2 (classify2)");
    if (h->device != mh->device) return fail(mh, ARUCOHIP_E_INVALID, "chromatic_classify_batch: the handle is on another device");
    if (h->last.board_frames != nframes) return fail(mh, ARUCOHIP_E_INVALID, "chromatic_classify_batch: no arucohip_board_detect_batch of nframes frames before");
    HIPCHK(mh, hipSetDevice(mh->device));
    hipStream_t s = mh->stream;
    const size_t px = (size_t)W * H;
    HIPCHK(mh, m->d_bgeom.reserve((size_t)nframes * sizeof(ChromaGeom), m->epoch));
    if (npix) {
        HIPCHK(mh, m->d_npix.reserve((size_t)nframes * sizeof(int32_t), m->epoch));
        HIPCHK(mh, hipMemsetAsync(m->d_npix, 0, (size_t)nframes * sizeof(int32_t), s));
    }
    // the poses where the board batch left them: each worker holds its own frames' boards
    for (const Span& sp : h->last.cut(nframes)) {
        const arucohip_board_t* boards = sp.w->d_board;
        launch_chroma_geometry(s, m->cam, sp.count, boards, (const float*)(boards + sp.w->cap_frames), min_prob, nullptr, nullptr, m->d_bgeom + sp.first);
    }
    HIPCHK(mh, hipGetLastError());
    m->last_batch = nframes;
    // frames and masks where they are; host sides go through staging, 64 MB of frames at a time (and at most 65535 per launch)
    const bool direct = frames_on_device && masks_on_device;
    const int piece = direct ? 65535 : (int)std::max<size_t>(1, std::min<size_t>(65535, ((size_t)64 << 20) / px));
    if (!frames_on_device) HIPCHK(mh, m->d_bframes.reserve(std::min(nframes, piece) * px, m->epoch));
    if (!masks_on_device) HIPCHK(mh, m->d_bmasks.reserve(std::min(nframes, piece) * px, m->epoch));
    for (int first = 0; first < nframes; first += piece) {
        const int cnt = std::min(piece, nframes - first);
        const uint8_t* src = frames + (size_t)first * frame_stride;
        size_t rs = row_stride, fs = frame_stride;
        if (!frames_on_device) {
            for (int f = 0; f < cnt; f++)
                HIPCHK(mh, hipMemcpy2DAsync(m->d_bframes + (size_t)f * px, W, src + (size_t)f * frame_stride, row_stride, W, H, hipMemcpyHostToDevice, s));
            src = m->d_bframes, rs = W, fs = px;
        }
        uint8_t* dst = masks_on_device ? masks + (size_t)first * px : (uint8_t*)m->d_bmasks;
        launch_chroma_classify(s, m->cam, method, m->thresh, cnt, src, rs, fs, m->d_bgeom + first, m->d_prob, m->d_inside, dst,
                               npix ? (int32_t*)m->d_npix + first : nullptr);
        HIPCHK(mh, hipGetLastError());
        if (!masks_on_device) HIPCHK(mh, hipMemcpyAsync(masks + (size_t)first * px, dst, (size_t)cnt * px, hipMemcpyDeviceToHost, s));
    }
    if (npix) HIPCHK(mh, hipMemcpyAsync(npix, m->d_npix, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(mh, hipStreamSynchronize(s));
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
    HIPCHK(h, w->d_gl.reserve(need, w->alloc_epoch));
    launch_gl_modelview(w->stream, nframes, cap, w->buf, w->d_gl);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(modelview, w->d_gl, need, hipMemcpyDeviceToHost, w->stream));
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
    auto onorm = [&](int a, int b) {
        // Point3f difference in float, cv::norm in double
        float dx = obj[3 * a] - obj[3 * b], dy = obj[3 * a + 1] - obj[3 * b + 1], dz = obj[3 * a + 2] - obj[3 * b + 2];
        return std::sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    };
    float ssize = -1;
    if (info_type == ARUCOHIP_BOARD_PIX && marker_size > 0)
        ssize = marker_size;
    else if (info_type == ARUCOHIP_BOARD_METERS)
        ssize = (float)onorm(0, 1);
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
    double mpp = info_type == ARUCOHIP_BOARD_PIX ? marker_size / onorm(0, 1) : 1;
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
        const int rc = create_child(h, h->lim, false, &l);
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
                const int crc = create_child(h, l, false, &h->retry);
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

// ---------------------------------------------------------------------------------------------
// Highly reliable marker dictionaries and boards (k_hrm.hip): HighlyReliableMarkers::createDicitionary and createBoardImage
// (src/highlyreliablemarkers.cpp:498-608). The scratch is the handle's d_hrm_gen, outside alloc_epoch: these calls never invalidate the
// single-frame graph.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int S31 = ah::HRM_STATE;
typedef std::vector<uint32_t> M31;   // 31 x 31, row-major, mod 2^32 (uint32 arithmetic wraps)

M31 m31_mul(const M31& A, const M31& B) {
    M31 C(S31 * S31, 0);
    for (int i = 0; i < S31; i++)
        for (int k = 0; k < S31; k++) {
            const uint32_t a = A[i * S31 + k];
            if (!a) continue;
            for (int j = 0; j < S31; j++) C[i * S31 + j] += a * B[k * S31 + j];
        }
    return C;
}

// M^k, M the step (r[i-31] .. r[i-1]) -> (r[i-30] .. r[i])
M31 m31_pow(uint64_t k) {
    M31 R(S31 * S31, 0), P(S31 * S31, 0);
    for (int i = 0; i < S31; i++) R[i * S31 + i] = 1;
    for (int j = 0; j + 1 < S31; j++) P[j * S31 + j + 1] = 1;
    P[30 * S31 + 0] = P[30 * S31 + 28] = 1;
    for (; k; k >>= 1) {
        if (k & 1) R = m31_mul(R, P);
        if (k > 1) P = m31_mul(P, P);
    }
    return R;
}

// srand(seed): r[0] = seed as int32 (0 -> 1), r[1..30] by the 16807 LCG (Schrage, C division), r[31..33] = r[0..2], then the recurrence
// up to r[343]. The state at output 0 is r[313..343].
void hrm_state0(uint32_t seed, uint32_t out[S31]) {
    int64_t r0 = (int32_t)seed;
    if (r0 == 0) r0 = 1;
    std::vector<uint32_t> r(344);
    r[0] = (uint32_t)r0;
    int64_t word = r0;
    for (int i = 1; i < 31; i++) {
        const int64_t hi = word / 127773, lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (uint32_t)word;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int i = 34; i < 344; i++) r[i] = r[i - 31] + r[i - 3];
    for (int i = 0; i < S31; i++) out[i] = r[313 + i];
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

extern "C" {

int arucohip_hrm_create_dictionary(arucohip_handle* h, int n, int dict_size, uint32_t seed, uint64_t* codes_out, int* tau0,
                                   int64_t* candidates_examined) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (n < 3 || n > 8) return fail(h, ARUCOHIP_E_INVALID, "hrm_create_dictionary: n must be 3..8 (n = 2 divides by zero in the reference)");
    if (dict_size < 1 || dict_size > 4096) return fail(h, ARUCOHIP_E_INVALID, "hrm_create_dictionary: dict_size must be 1..4096");
    if (!codes_out) return fail(h, ARUCOHIP_E_INVALID, "hrm_create_dictionary: NULL codes_out");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t jbytes = (size_t)(HRM_LANE_BITS + 1) * S31 * S31 * sizeof(uint32_t);
    const size_t o_state = align256(jbytes), o_ctl = o_state + 256, o_code = o_ctl + 256, o_self = o_code + (size_t)HRM_WINDOW * 8,
                 o_dmin = o_self + HRM_WINDOW, o_dict = o_dmin + HRM_WINDOW, total = o_dict + (size_t)4096 * 4 * sizeof(uint64_t);
    HIPCHK(h, h->d_hrm_gen.reserve(total, h->hrm_epoch));
    uint8_t* b = h->d_hrm_gen;
    HrmBufs bufs{(uint32_t*)(b + o_state), (uint32_t*)b, (uint64_t*)(b + o_code), b + o_self, b + o_dmin, (uint64_t*)(b + o_dict),
                 (HrmCtl*)(b + o_ctl)};
    // J_b = M^(HRM_LANE_CANDS n^2 2^b): lane l starts at J applied for the bits of l; the last one is a whole window
    std::vector<uint32_t> jumps;
    M31 J = m31_pow((uint64_t)HRM_LANE_CANDS * n * n);
    for (int bit = 0; bit <= HRM_LANE_BITS; bit++) {
        jumps.insert(jumps.end(), J.begin(), J.end());
        if (bit < HRM_LANE_BITS) J = m31_mul(J, J);
    }
    uint32_t st[S31];
    hrm_state0(seed, st);
    const int tau_init = 2 * ((4 * ((n * n) / 4)) / 3);
    HrmCtl c{};
    c.tau = tau_init, c.count = 0, c.limit = HRM_LIMIT, c.dsize = 0, c.base = 0, c.status = HRM_RUNNING;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(bufs.jumps, jumps.data(), jbytes, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(bufs.state, st, sizeof(st), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(bufs.ctl, &c, sizeof(c), hipMemcpyHostToDevice, s));
    // the reference examines at most (dict_size + tau) * 100000 candidates: every acceptance and every decrement resets the count
    const int64_t max_windows = ((int64_t)(dict_size + tau_init) * HRM_LIMIT + HRM_WINDOW - 1) / HRM_WINDOW + 1;
    int syncs = 0;
    for (int64_t w = 0; w < max_windows; w++) {
        launch_hrm_window(s, n, dict_size, bufs);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&c, bufs.ctl, sizeof(c), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));   // the one host synchronisation of a window
        syncs++;
        if (c.status != HRM_RUNNING) break;
    }
    h->hrm_stats[0] = c.windows, h->hrm_stats[1] = syncs, h->hrm_stats[2] = c.accepted, h->hrm_stats[3] = c.decrements;
    if (c.status == HRM_TAU_ZERO)
        return fail(h, ARUCOHIP_E_INVALID, "hrm_create_dictionary: tau reached 0 (too many markers for this marker size; CV_Error in the reference)");
    if (c.status != HRM_DONE) return fail(h, ARUCOHIP_E_HIP, "hrm_create_dictionary: the window walk did not finish");
    std::vector<uint64_t> rot((size_t)dict_size * 4);
    HIPCHK(h, hipMemcpyAsync(rot.data(), bufs.dict, rot.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < dict_size; i++) codes_out[i] = rot[(size_t)i * 4];
    if (tau0) *tau0 = c.tau;
    if (candidates_examined) *candidates_examined = c.examined;
    return ARUCOHIP_OK;
}

int arucohip_debug_hrm_counters(arucohip_handle* h, int32_t out[4]) {
    if (!h || !out) return ARUCOHIP_E_INVALID;
    for (int i = 0; i < 4; i++) out[i] = h->hrm_stats[i];
    return ARUCOHIP_OK;
}

int arucohip_debug_hrm_stream(arucohip_handle* h, uint32_t seed, uint64_t offset, int count, uint32_t* out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!out || count < 0 || count > (1 << 24) || offset + (uint64_t)count >= (1ull << HRM_POW_BITS))
        return fail(h, ARUCOHIP_E_INVALID, "debug_hrm_stream: count must be 0..2^24 and offset + count below 2^48");
    if (count == 0) return ARUCOHIP_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t pbytes = (size_t)HRM_POW_BITS * S31 * S31 * sizeof(uint32_t), o_state = align256(pbytes), o_out = o_state + 256,
                 total = o_out + (size_t)count * sizeof(uint32_t);
    HIPCHK(h, h->d_hrm_gen.reserve(total, h->hrm_epoch));
    uint8_t* b = h->d_hrm_gen;
    std::vector<uint32_t> pow2;
    M31 P = m31_pow(1);
    for (int bit = 0; bit < HRM_POW_BITS; bit++) {
        pow2.insert(pow2.end(), P.begin(), P.end());
        P = m31_mul(P, P);
    }
    uint32_t st[S31];
    hrm_state0(seed, st);
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(b, pow2.data(), pbytes, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(b + o_state, st, sizeof(st), hipMemcpyHostToDevice, s));
    launch_hrm_stream(s, (const uint32_t*)(b + o_state), (const uint32_t*)b, offset, count, (uint32_t*)(b + o_out));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, b + o_out, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_hrm_board_size(int n, int grid_w, int grid_h, int chromatic, int* width, int* height, int* channels) {
    if (n < 3 || n > 8 || grid_w < 1 || grid_h < 1 || grid_w > 128 || grid_h > 128 || !width || !height || !channels) return ARUCOHIP_E_INVALID;
    const int ms = (n + 2) * 20, gap = ms / 5, margin = chromatic ? 2 * gap : 0;
    *width = grid_w * ms + (grid_w - 1) * gap + margin;
    *height = grid_h * ms + (grid_h - 1) * gap + margin;
    *channels = chromatic ? 3 : 1;
    return ARUCOHIP_OK;
}

int arucohip_hrm_board_image(arucohip_handle* h, int n, int count, const uint64_t* codes, int grid_w, int grid_h, int chromatic, uint8_t* image,
                             size_t row_stride, int image_on_device, int32_t* ids, float* obj) {
    if (!h) return ARUCOHIP_E_INVALID;
    int W = 0, H = 0, ch = 0;
    if (arucohip_hrm_board_size(n, grid_w, grid_h, chromatic, &W, &H, &ch) != ARUCOHIP_OK)
        return fail(h, ARUCOHIP_E_INVALID, "hrm_board_image: n must be 3..8 and the grid 1..128 x 1..128");
    const int nb = grid_w * grid_h;
    if (!codes || !image || row_stride < (size_t)W * ch) return fail(h, ARUCOHIP_E_INVALID, "hrm_board_image: NULL codes / image or row_stride too small");
    if (count < nb) return fail(h, ARUCOHIP_E_INVALID, "hrm_board_image: fewer codes than grid cells (the reference reads past the dictionary)");
    if (ids && n >= 6)
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "hrm_board_image: getId() shifts past 32 bits for n >= 6 (undefined in the reference); pass ids = NULL");
    const uint64_t valid = n == 8 ? ~0ull : (1ull << (n * n)) - 1;
    for (int i = 0; i < nb; i++)
        if (codes[i] & ~valid) return fail(h, ARUCOHIP_E_INVALID, "hrm_board_image: a code has bits past n * n");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t stride = ((size_t)W * ch + 15) & ~(size_t)15, o_img = align256((size_t)nb * sizeof(uint64_t)), total = o_img + stride * H;
    HIPCHK(h, h->d_hrm_gen.reserve(total, h->hrm_epoch));
    uint8_t* b = h->d_hrm_gen;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(b, codes, (size_t)nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    launch_hrm_board(s, (const uint64_t*)b, n, grid_w, grid_h, chromatic ? 1 : 0, W, H, ch, stride, b + o_img);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy2DAsync(image, row_stride, b + o_img, stride, (size_t)W * ch, H, image_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    // BC.ids (getId(): sum of 2 << pos) and BC.objPoints, on the host in the reference's float arithmetic
    const unsigned ms = (unsigned)(n + 2) * 20, gap = ms / 5;
    const int sx = grid_w * (int)ms + (grid_w - 1) * (int)gap, sy = grid_h * (int)ms + (grid_h - 1) * (int)gap;
    const float cx = (float)(sx / 2.), cy = (float)(sy / 2.);
    for (int y = 0, idp = 0; y < grid_h; y++)
        for (int x = 0; x < grid_w; x++, idp++) {
            if (ids) {
                uint32_t id = 0;
                for (int p = 0; p < n * n; p++)
                    if ((codes[idp] >> p) & 1) id |= 2u << p;
                ids[idp] = (int32_t)id;
            }
            if (obj) {
                const unsigned ox = (unsigned)x * (gap + ms), oy = (unsigned)y * (gap + ms);
                const unsigned px[4] = {ox, ox + ms, ox + ms, ox}, py[4] = {oy, oy, oy + ms, oy + ms};
                for (int k = 0; k < 4; k++) {
                    float* o = obj + (size_t)idp * 12 + 3 * k;
                    o[0] = (float)px[k] - cx;
                    o[1] = -((float)py[k] - cy);
                    o[2] = 0.f;
                }
            }
        }
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
