// Private host-side header of libarucohip's C ABI (capi*.hip): the handle, the memory it owns and the helpers those files share.
// Kernel files never include it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "border_rect.h"
#include "fisheye_device.h"
#include "frames_host.h"
#include "internal.h"
#include "thr_plan.h"

using namespace ah;

// one event after every kernel of a batch; a ring of TSETS batches so that asynchronous steps can be averaged
// slot k = the interval between mark k and mark k + 1. With a side stream: walker_long = the generations of long walks up to the fork,
// contour_quad = both passes including the wait for the side stream's late generations. On a pipeline lane (no side stream):
// walker_long = every generation, contour_quad = its one pass.
enum { K_THRESHOLD = 0, K_FILTER, K_WALKERS, K_WALKERS_LONG, K_CONTOUR_QUADS, K_FRAME_CANDS, K_DECODE, K_REFINE_LINES, K_REFINE_PIXELS, K_FINALIZE, K_POSE, K_COUNT };
constexpr int TSETS = 32;

// Memory the handle owns: device memory, or pinned host memory for staging the host reads. reserve() replaces the allocation only when
// `need` exceeds the capacity (exact size, no slack, never shrinks). The destructor frees.
template <typename T>
struct Mem {
    T* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;
    explicit Mem(bool pinned_ = false) : pinned(pinned_) {}
    Mem(Mem&& o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned) { o.p = nullptr, o.bytes = 0; }
    ~Mem() { (void)release(); }
    operator T*() const { return p; }
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
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
// hold a batch; a waited ticket adopts its lane's. The getters, board poses, planar poses, calibration and ChromaticMask read it and nothing else.
struct Span { arucohip_handle* w; int first, count; };   // worker w holds frames [first, first + count)
struct Batch {
    int nspan = 0, frames = 0;
    Span span[MAX_WORKERS] = {};
    int W = 0, H = 0, nthr = 1;   // W x H: the thresholded image (the frame reduced by the pyrDown level)
    int frame_w = 0, frame_h = 0;   // the frames themselves
    int board_frames = 0;   // frames whose board poses arucohip_board_detect_batch left in the workers' d_board
    bool ideal = false;     // arucohip_fisheye_undistort_markers_batch replaced the corners by those of an ideal pinhole camera: they no
                            // longer match the frames' pixels. Every detection sets the record whole and so clears it
    const Span* begin() const { return span; }
    const Span* end() const { return span + nspan; }
    int index(const Span& s) const { return (int)(&s - span); }   // s is one of this batch's own spans, as on_workers hands them out
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
    std::vector<Mem<void>> held;      // create-time memory, held for the handle's life: the Buffers arrays, zero_block, d_small_*, d_patch, pinned staging
    Mem<uint32_t> walk_scratch;       // buf.walk_scratch
    Mem<uint8_t> patches;             // buf.patches
    bool cells_valid = false;         // buf.cells holds the last batch's cell medians (decode_from_cells; arucohip_debug_cells)
    Mem<uint8_t> d_gray;              // staging for host frames (gray) and the converted BGR frames
    Mem<uint8_t> d_bgr;               // staging for host BGR frames
    // The call-scratch arena: the device memory an entry point needs for the length of one call, carved by carve_scratch (below).
    // Every handle has one, chunk workers and lanes too, allocated at the first call that needs it.
    // - It belongs to the entry point that is running; what it holds is dead to the host when the entry point returns.
    // - An entry point reserves the arena of a given handle AT MOST ONCE, before it takes any pointer from it: one layout names all it
    //   needs from that handle (records, staged sources and counts, staged host images, the images a host caller gets back). A call
    //   spread over workers carves each worker's arena once, on that worker's stream, between fork and join.
    // - w's arena is used only on w->stream, or on streams forked from it and joined to it again within the call. A call whose every
    //   side is on the device returns without synchronising, so queued work may still read the arena; the next user is safe because it
    //   queues on that same stream, and a growing reserve() goes through hipFree, which waits for the device. (A caller who changes
    //   streams orders them: INTEGRATION.md.)
    // What is not in it, and why:
    // - memory a later call reads: d_board (resident board poses, read by ChromaticMask), d_charuco (resident corners), d_hrm (the
    //   dictionary), d_umap_* / d_fmap_* (cached maps), hc_solver (pinned);
    // - the detection pipeline's own memory: d_gray, d_bgr, walk_scratch, patches, d_erode, d_canny, d_pyr, d_user_dec, hu_list,
    //   hu_patches and everything in `held`. The one-frame graph's address check (FrameGraph below) is about d_gray, walk_scratch and
    //   patches, so nothing else may ever grow them;
    // - d_charuco_views: the one buffer that lives across a nested entry point, which carves the arena itself.
    Mem<uint8_t> scratch;
    arucohip_marker_t* wt_out = nullptr;   // set around detect_core by chunk_enqueue: finalize_kernel writes the results there too
    int32_t* wt_n = nullptr;
    int wt_cap = 0;
    Mem<uint8_t> d_erode;             // eroded planes (params.erode)
    Mem<uint64_t> d_canny;            // CANNY: survivor tiles, edge tiles, changed flag
    int pyr = 0;                      // MarkerDetector::pyrDown level (arucohip_set_pyr_down), the same on every worker of the tree
    Mem<uint8_t> d_pyr;               // the reduced frames of a level above 0: two halves, the levels go to and fro between them (PyrPlan)
    // frame undistortion (arucohip_undistort): the map of the last camera is kept (umap_nd = -1: none)
    Mem<short2> d_umap_xy;
    Mem<uint16_t> d_umap_f;
    int umap_w = 0, umap_h = 0, umap_nd = -1;
    float umap_K[9] = {}, umap_d[8] = {};
    // fisheye lenses (capi_fisheye.hip): a map slot of its own, so that a fisheye camera never evicts the pinhole map above
    Mem<short2> d_fmap_xy;
    Mem<uint16_t> d_fmap_f;
    int fmap_w = 0, fmap_h = 0;       // fmap_w = 0: none
    double fmap_key[18] = {};         // K (4), D (4), Knew (9), max_angle
    std::vector<FisheyeCam> fisheye_cams;   // the models of the last marker call as they were copied to the workers
    Dictionary hrm;
    Mem<uint64_t> d_hrm;              // hrm.codes on the device
    // caller's own decoder (arucohip_set_decoder_callback)
    arucohip_decoder_fn decoder_fn = nullptr;
    void* decoder_user = nullptr;
    Mem<int2> d_user_dec;             // [cap_flat] {id, nRotations} returned by the callback
    Mem<uint32_t> hu_list{true};      // pinned staging of the callback path: candidate list, decoder results, call order
    Mem<uint8_t> hu_patches{true};    // pinned staging: the canonical patches handed to the callback (+ one scratch patch)
    size_t bits_bytes = 0, tile_bits_bytes = 0;
    int bits_w = 0, bits_h = 0;       // geometry the bit image was last written with (pad words depend on it)
    // pinned host staging
    arucohip_marker_t* h_markers = nullptr;
    int32_t* h_n = nullptr;
    uint32_t* h_counters = nullptr;
    // small device scratch for the stage-level calls
    float* d_small_f = nullptr;       // 8192 floats
    double* d_small_d = nullptr;      // 64 doubles
    int* d_small_i = nullptr;
    uint8_t* d_patch = nullptr;       // MAX_WARP^2
    Mem<arucohip_board_t> d_board;    // batched board results + ids
    uint32_t* zero_block = nullptr;   // counters, gen_cnt, trig_cnt, raw_cnt, ring_cnt: zeroed together at the start of a batch
    size_t zero_words = 0;
    Mem<uint8_t> hc_solver{true};     // pinned copy of the state of whichever solver runs (lm_drive), read once per iteration: the calls are synchronous, so one serves all
    // arucohip_charuco_corners_batch (capi_charuco.hip), on the handle the caller holds: the corner records of the last call and their counts stay in
    // d_charuco for the calibration and the pose; the host keeps the layout and the counts
    Mem<uint8_t> d_charuco;           // records [frames][corners], then n_found [frames], then the layout's ids
    Mem<uint8_t> d_charuco_views;     // arucohip_charuco_calibrate_batch's gathered views: arucohip_calibrate_camera reads them and carves `scratch` itself
    struct Charuco {
        arucohip_charuco_t layout = {};
        int frames = 0;               // 0: no resident corners
        std::vector<int32_t> n_found;
    } charuco;
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
    // Late walker generations (k_contours.hip, WalkFork). A pipeline lane and its chunk workers (in_lane) have neither the stream nor
    // the events: their batch runs on `stream` alone, so `depth` lanes are `depth` streams.
    bool in_lane = false;
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_wfork = nullptr, ev_wjoin = nullptr;
    bool thres_bytes = true;             // buf.thres holds the last batch's byte image (else: tiles + buf.thres_edge, expanded on demand)
    ThrPlan thr_plan_done{};             // the plan the last launch_threshold of this worker executed (arucohip_debug_threshold_plan)
    int thr_plan_planes = 0;             // its planes; 0: none yet, or the last threshold was CANNY
    int32_t hrm_stats[4] = {};           // the last arucohip_hrm_create_dictionary: windows, host synchronisations, acceptances, tau decrements
    // One frame per call (the reference's call shape, arucohip_detect): the chain of ~20 dependent dispatches of a frame is captured once per
    // (geometry, parameters, camera) into a hipGraph and replayed with ONE launch per call; the frame's H2D copy stays outside (its source
    // pointer changes with every call), the results land in the handle's pinned staging inside the graph.
    // The captured launches carry device addresses by value; a replay needs every one of them to be live and as large as at the capture:
    // - in the value key: dp.hrm_codes (d_hrm), and buf.thr_stamp_on, which picks the threshold kernel's stamp pointer;
    // - compared with `addrs` before a replay and after a capture: gray_dev (d_gray for host gray and BGR frames), buf.walk_scratch and
    //   buf.patches, which calls of other shapes grow. An equal address is enough, since reserve() never shrinks. The captured chain is that of
    //   ONE frame, which always stores its patches (decode_from_cells is false below three frames), so batch_prologue reserves them before every
    //   capture and replay; batches that decode from cell medians neither touch nor move buf.patches, and buf.cells is create-time memory;
    // - neither: the other Buffers arrays, zero_block and h_markers are create-time memory (`held`); d_erode, d_canny and the user decoder's
    //   staging and d_pyr belong to configurations that are not graphed; wt_out is set only inside chunk_enqueue, which does not run this path.
    //   Memory no captured launch reads may be replaced at any time: the call-scratch arena (`scratch`), d_bgr, the cached undistortion and
    //   fisheye maps, hc_solver, d_board, d_charuco and d_charuco_views, and what ChromaticMask objects own.
    struct FrameGraph {
        hipGraphExec_t exec = nullptr;
        uint64_t key = 0;          // digest of everything the captured launches carry by value
        uint64_t seen = 0;         // key of the previous eager call: the second call with the same key captures (buffers are sized by then)
        std::array<const void*, 3> addrs{};   // gray_dev, buf.walk_scratch and buf.patches at the capture
        bool thres_bytes = false;  // what the captured threshold left in buf.thres (a replay sets thres_bytes to it)
        ThrPlan thr_plan{};        // ... and the plan it executed (a replay sets thr_plan_done / thr_plan_planes to it)
        int thr_plan_planes = 0;
        int disabled = 0;          // ARUCOHIP_GRAPH=0, or a capture failed once
    } fgraph;
    // Batches in flight (arucohip_set_pipeline_depth / _submit / _wait): every pipeline lane is a complete worker (own
    // buffers, ONE stream: no side stream); ticket t runs on lane t mod depth, so the latency-bound tail of batch t (border following,
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
    double render_ms[2] = {};            // with timing: build and raster kernel time summed over render_calls calls (arucohip_render_times)
    int render_calls = 0;
};

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

inline int fail(arucohip_handle* h, int code, const char* msg) {
    if (h) h->err = msg;
    return code;
}

// Frame formats (capi_ingest.hip), shared by arucohip_convert_batch and arucohip_export_batch.
// the caller's record as the host code carries it; bits and chroma_offset only where the format has them
int take_format(arucohip_handle* h, const arucohip_frame_format_t* fmt, FrameFmt* f);
// a format against a geometry, with the limits of the detection calls (check_geometry of capi.hip): one message per refusal
int check_frame_format(arucohip_handle* h, const FrameFmt& fmt, int nframes, int W, int H, size_t row_stride, size_t frame_stride);

// A call's scratch, laid out once: take() hands out consecutive 256-byte aligned arrays of `base`. A layout function names every
// buffer in one take(); it runs twice, with a null base to size the memory (every take() is then null, and `at` ends as the bytes it
// needs) and, after reserve(), with the memory of the handle that owns the scratch to bind the pointers.
struct Carver {
    uint8_t* base;
    size_t at = 0;
    // the offset of `bytes` more bytes: what stage_input / stage_output take for staged images
    size_t take_at(size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    }
    template <class T>
    T* take(size_t count) {
        const size_t here = take_at(count * sizeof(T));
        return base ? (T*)(base + here) : nullptr;
    }
};

// The one reservation of w's call-scratch arena (arucohip_handle::scratch) by the entry point that is running: layout(Carver&) takes
// everything the call needs from w. Errors are reported on h.
template <class Layout>
int carve_scratch(arucohip_handle* w, arucohip_handle* h, Layout layout) {
    Carver size{nullptr};
    layout(size);
    HIPCHK(h, w->scratch.reserve(size.at));
    Carver bind{w->scratch.p};
    layout(bind);
    return ARUCOHIP_OK;
}

// Image batches of the caller (frames_host.h) as the kernels take them. A batch on the device is used where it lies, at the caller's
// strides. A host batch is staged packed at mem + at, image i at i * staged_frame (0: the images back to back), in the arena of the
// handle the call runs on, at an offset its layout carved (Carver::take_at): stage_input queues the upload on s, stage_output queues
// nothing, unstage queues the way back of an output or of a batch changed in place (nothing for a device batch). None of them
// synchronises. These and the checks below are static, so the library's exported symbols stay the C ABI's and the older inline helpers'.
struct DevImages {
    uint8_t* p;
    size_t row, frame;
};
static inline int stage_output(arucohip_handle* h, const Images& im, const Mem<uint8_t>& mem, size_t at, DevImages* v, size_t staged_frame = 0) {
    *v = {im.p, im.row, im.frame};
    if (im.on_device) return ARUCOHIP_OK;
    const size_t frame = staged_frame ? staged_frame : im.packed_frame();
    if (!mem.p || at + (size_t)(im.n - 1) * frame + im.packed_frame() > mem.bytes)
        return fail(h, ARUCOHIP_E_HIP, "staging memory is smaller than the images it is to hold");
    *v = {mem.p + at, im.packed_row(), frame};
    return ARUCOHIP_OK;
}
static inline int stage_input(arucohip_handle* h, hipStream_t s, const Images& im, const Mem<uint8_t>& mem, size_t at, DevImages* v, size_t staged_frame = 0) {
    if (const int rc = stage_output(h, im, mem, at, v, staged_frame)) return rc;
    if (im.on_device) return ARUCOHIP_OK;
    return im.for_each_copy(
        [&](size_t from, size_t pitch, size_t to, size_t packed_pitch, size_t bytes, size_t rows) -> int {
            HIPCHK(h, hipMemcpy2DAsync(v->p + to, packed_pitch, im.p + from, pitch, bytes, rows, hipMemcpyHostToDevice, s));
            return ARUCOHIP_OK;
        },
        v->frame);
}
static inline int unstage(arucohip_handle* h, hipStream_t s, const Images& im, const DevImages& v) {
    if (im.on_device) return ARUCOHIP_OK;
    return im.for_each_copy(
        [&](size_t to, size_t pitch, size_t from, size_t packed_pitch, size_t bytes, size_t rows) -> int {
            HIPCHK(h, hipMemcpy2DAsync(im.p + to, pitch, v.p + from, packed_pitch, bytes, rows, hipMemcpyDeviceToHost, s));
            return ARUCOHIP_OK;
        },
        v.frame);
}

// The refusals every image entry point words the same way: `call` is its prefix ("rectify", "draw", ...), `arg` what precedes
// row_stride / frame_stride in the argument's name ("", "dst_", "tex->").
static inline int check_strides(arucohip_handle* h, const char* call, const char* arg, const Images& im) {
    const Images::Strides bad = im.check_strides();
    if (bad == Images::STRIDES_OK) return ARUCOHIP_OK;
    const std::string msg = std::string(call) + ": " + arg +
                            (bad == Images::ROW_BELOW_ROW_BYTES ? "row_stride is smaller than a row of the image" : "frame_stride is smaller than an image");
    return fail(h, ARUCOHIP_E_INVALID, msg.c_str());
}
static inline int check_disjoint(arucohip_handle* h, const char* call, const char* a_name, const Images& a, const char* b_name, const Images& b) {
    if (!a.overlaps(b)) return ARUCOHIP_OK;
    const std::string msg = std::string(call) + ": " + a_name + " overlaps " + b_name;
    return fail(h, ARUCOHIP_E_INVALID, msg.c_str());
}

// The camera arguments of the plane calls (rectify, composite): K only where the call needs it, dist only with K.
static inline int check_plane_camera(arucohip_handle* h, const char* call, bool need_K, const float* K, const float* dist, int ndist) {
    const char* bad = need_K && !K                                                ? "K is NULL (the board call needs the camera)"
                      : !(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8) ? "ndist must be 0, 4, 5 or 8"
                      : ndist > 0 && !dist                                        ? "dist is NULL with ndist > 0"
                      : ndist > 0 && !K                                           ? "dist without K"
                                                                                  : nullptr;
    if (!bad) return ARUCOHIP_OK;
    const std::string msg = std::string(call) + ": " + bad;
    return fail(h, ARUCOHIP_E_INVALID, msg.c_str());
}

// The plane maps of one rectify or composite call, carved by the call's one layout from the arena: one 3 x 3 map and one valid word
// per frame, and the staged boards of a board call.
struct PlaneMaps {
    double* maps;
    int32_t* valid;
    arucohip_board_t* boards;
};
static inline void carve_plane_maps(Carver& cv, int n, PlaneMaps* m) {
    m->maps = cv.take<double>((size_t)n * 9);
    m->valid = cv.take<int32_t>((size_t)n);
    m->boards = cv.take<arucohip_board_t>((size_t)n);
}
// the caller's own maps and valid words: where they are on the device, else uploaded to m on h's stream and *maps / *valid repointed
static inline int stage_plane_maps(arucohip_handle* h, const PlaneMaps& m, int n, int on_device, const double** maps, const int32_t** valid) {
    if (on_device) return ARUCOHIP_OK;
    HIPCHK(h, hipMemcpyAsync(m.maps, *maps, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    *maps = m.maps;
    if (*valid) {
        HIPCHK(h, hipMemcpyAsync(m.valid, *valid, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        *valid = m.valid;
    }
    return ARUCOHIP_OK;
}
// the maps of a board call: host boards go up, `launch` (launch_plane_maps / launch_plane_inverse_maps) writes maps and valid words
static inline int plane_maps_of_boards(arucohip_handle* h, const PlaneMaps& m, decltype(launch_plane_maps)* launch, const arucohip_board_t* boards,
                                int boards_on_device, int n, const arucohip_rectify_t& win) {
    if (!boards_on_device) {
        HIPCHK(h, hipMemcpyAsync(m.boards, boards, (size_t)n * sizeof(arucohip_board_t), hipMemcpyHostToDevice, h->stream));
        boards = m.boards;
    }
    launch(h->stream, boards, n, win, m.maps, m.valid);
    HIPCHK(h, hipGetLastError());
    return ARUCOHIP_OK;
}
// ... and what a board call hands back of them, queued behind the call's own work
static inline int read_plane_maps(arucohip_handle* h, const PlaneMaps& m, int n, int32_t* status, double* maps_out) {
    if (status) HIPCHK(h, hipMemcpyAsync(status, m.valid, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (maps_out) HIPCHK(h, hipMemcpyAsync(maps_out, m.maps, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return ARUCOHIP_OK;
}

// whether a window of a board plane (arucohip_rectify_t) spans it: finite, with u and v steps that are neither zero nor parallel
inline bool window_spans_plane(const arucohip_rectify_t& win) {
    const double cross = (double)win.ux * win.vy - (double)win.uy * win.vx;
    return std::fabs(cross) > 0 && std::isfinite(cross) && std::isfinite(win.x0) && std::isfinite(win.y0);
}

// fork: the other workers' streams wait for what the first worker's stream (the batch's own) has queued so far; errors are reported on h
int fork_workers(arucohip_handle* h, const Batch& b);
// join: the first worker's stream waits for the others
int join_workers(arucohip_handle* h, const Batch& b);

// per_span(span) for every span of the batch between fork and join, each on its worker's stream. The workers rejoin the first worker's
// stream whether or not every span was taken; then the first failure is returned: a span's own, a refused launch, the join's.
template <class F>
int on_workers(arucohip_handle* h, const Batch& b, F per_span) {
    int rc = fork_workers(h, b);
    if (rc) return rc;
    hipError_t launched = hipSuccess;
    for (const Span& s : b) {
        const int r = per_span(s);
        if (!rc) rc = r;
        if (launched == hipSuccess) launched = hipGetLastError();
    }
    const int joined = join_workers(h, b);
    if (rc) return rc;
    HIPCHK(h, launched);
    return joined;
}

// The host side of a Levenberg-Marquardt run on o's stream (lm_device.h): *st goes up to dev through the pinned hc_solver, init()
// launches the start values, and started(state) turns the solver's err bits into its own message and code. Then iter() launches
// one attempt at a time, with one copy of the state and one synchronisation each for the stop flag: at most 30 accepted steps; every
// rejected step raises lambda tenfold, and lambda above 1e16 stops. *st returns the final state.
// lm_start is its first phase alone (the start-value hook stops after it): the state up, init(), the state back in the pinned copy,
// which it returns in *hs.
template <class State, class Init>
int lm_start(arucohip_handle* o, State* dev, const State* st, Init init, State** hs_out) {
    hipStream_t s = o->stream;
    HIPCHK(o, o->hc_solver.reserve(sizeof(State)));
    State* hs = (State*)(uint8_t*)o->hc_solver;
    *hs = *st;
    hs->lm.max_iter = 30, hs->lm.lg = -3;
    HIPCHK(o, hipMemcpyAsync(dev, hs, sizeof(State), hipMemcpyHostToDevice, s));
    init();
    HIPCHK(o, hipGetLastError());
    HIPCHK(o, hipMemcpyAsync(hs, dev, sizeof(State), hipMemcpyDeviceToHost, s));
    HIPCHK(o, hipStreamSynchronize(s));
    *hs_out = hs;
    return ARUCOHIP_OK;
}
template <class State, class Init, class Started, class Iter>
int lm_drive(arucohip_handle* o, State* dev, State* st, Init init, Started started, Iter iter) {
    hipStream_t s = o->stream;
    State* hs = nullptr;
    if (const int rc = lm_start(o, dev, st, init, &hs)) return rc;
    if (const int rc = started(*hs)) return rc;
    for (int it = 0; it < 256 && !hs->lm.done; it++) {
        iter();
        HIPCHK(o, hipGetLastError());
        HIPCHK(o, hipMemcpyAsync(hs, dev, sizeof(State), hipMemcpyDeviceToHost, s));
        HIPCHK(o, hipStreamSynchronize(s));
    }
    *st = *hs;
    return ARUCOHIP_OK;
}

// fx fy cx cy k1 k2 p1 p2 k3, as the solvers take a camera, from a 3 x 3 K and five distortion coefficients
template <class TK, class Tk>
inline void intr9(const TK* K, const Tk* k, double in[9]) {
    const double v[9] = {(double)K[0], (double)K[4], (double)K[2], (double)K[5], (double)k[0], (double)k[1], (double)k[2], (double)k[3], (double)k[4]};
    for (int i = 0; i < 9; i++) in[i] = v[i];
}

// Observations given as arrays (owner = the frame or view of each, id, 8 corner coordinates): where they are when they are on the device
// already, else copied into the staging arrays on h's stream.
struct ObsArrays {
    const int32_t *owner, *id;
    const float* corners;
};
inline int stage_obs(arucohip_handle* h, ObsArrays in, int nobs, int on_device, int32_t* d_owner, int32_t* d_id, float* d_corners, ObsArrays* out) {
    *out = in;
    if (!on_device) {
        if (nobs > 0) {
            HIPCHK(h, hipMemcpyAsync(d_owner, in.owner, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(d_id, in.id, (size_t)nobs * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(d_corners, in.corners, (size_t)nobs * 8 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        }
        *out = ObsArrays{d_owner, d_id, d_corners};
    }
    if (!out->owner) out->owner = d_owner;   // nobs == 0: nothing is read, but a null owner array means the strided layout of a batch
    return ARUCOHIP_OK;
}

// A board given as a host BoardDef: ids and obj go up to d_ids / d_obj on stream s; *dev is the record with the device arrays.
inline int upload_board(arucohip_handle* h, const BoardDef& bd, hipStream_t s, int32_t* d_ids, float* d_obj, BoardDef* dev) {
    HIPCHK(h, hipMemcpyAsync(d_ids, bd.ids, (size_t)bd.nboard * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_obj, bd.obj, (size_t)bd.nboard * 12 * sizeof(float), hipMemcpyHostToDevice, s));
    *dev = bd, dev->ids = d_ids, dev->obj = d_obj;
    return ARUCOHIP_OK;
}

// The caller's camera as the kernels take it. Every entry point keeps its own argument checks (which ndist, whether K is required)
// and fills the record here: zeroed whole first, padding included, because the one-frame graph's key digests its bytes.
inline void fill_cam(CamModel* cam, const float* K, const float* dist, int ndist, float marker_size, int y_perp) {
    std::memset(cam, 0, sizeof(*cam));
    cam->has_K = K != nullptr, cam->has_dist = K && dist && ndist > 0;
    for (int i = 0; K && i < 9; i++) cam->K[i] = K[i];
    for (int i = 0; cam->has_dist && i < ndist; i++) cam->k[i] = (double)dist[i];
    cam->marker_size = marker_size, cam->y_perp = y_perp;
}

// A span's marker lists to the caller's out [frames][cap] / n_out [frames], queued on the worker's stream. Device arrays take the
// lists as they are (rows cut to the smaller of cap and the worker's cap_markers). Host arrays take them in two steps: the worker's
// whole lists and counts go to *staged and n_host [s.count] here, and collect_markers finishes once the stream has drained.
inline int enqueue_markers(arucohip_handle* h, const Span& s, arucohip_marker_t* out, int cap, int32_t* n_out, int out_on_device,
                           std::vector<arucohip_marker_t>* staged, int32_t* n_host) {
    const Buffers& wb = s.w->buf;
    const size_t row = (size_t)wb.cap_markers * sizeof(arucohip_marker_t), counts = (size_t)s.count * sizeof(int32_t);
    hipStream_t st = s.w->stream;
    if (out_on_device) {
        HIPCHK(h, hipMemcpy2DAsync(out + (size_t)s.first * cap, (size_t)cap * sizeof(arucohip_marker_t), wb.markers, row,
                                   (size_t)std::min(cap, wb.cap_markers) * sizeof(arucohip_marker_t), (size_t)s.count, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(n_out + s.first, wb.nmarkers, counts, hipMemcpyDeviceToDevice, st));
        return ARUCOHIP_OK;
    }
    staged->resize((size_t)s.count * wb.cap_markers);
    HIPCHK(h, hipMemcpyAsync(staged->data(), wb.markers, (size_t)s.count * row, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(n_host, wb.nmarkers, counts, hipMemcpyDeviceToHost, st));
    return ARUCOHIP_OK;
}
// The second step, on the host: staged [s.count][cap_markers] and n_host [s.count], the span's own, to its rows of out / n_out. n_out
// gets the true counts; a list longer than cap is cut and reported.
inline int collect_markers(arucohip_handle* h, const Span& s, int cap, arucohip_marker_t* out, int32_t* n_out, const arucohip_marker_t* staged,
                           const int32_t* n_host) {
    const int capM = s.w->buf.cap_markers;
    int ret = ARUCOHIP_OK;
    for (int f = 0; f < s.count; f++) {
        int n = n_host[f];
        n_out[s.first + f] = n;
        if (n > cap) {
            if (ret == ARUCOHIP_OK) ret = fail(h, ARUCOHIP_E_CAPACITY, "marker output array too small");
            n = cap;
        }
        n = std::min(n, capM);
        if (n > 0) std::memcpy(out + (size_t)(s.first + f) * cap, staged + (size_t)f * capM, (size_t)n * sizeof(arucohip_marker_t));
    }
    return ret;
}

// Camera calibration (capi_calib.hip), shared by the pinhole and the fisheye entry points.
// The views of one run, bound in the arena of the handle the run is on: the solver's arrays (d; d.obj / d.img may be the caller's
// own device arrays), the staging of points and of a batch's gather, each view's offset and count.
struct CalibViews {
    CalibDev d{};
    float *obj = nullptr, *img = nullptr;             // [npts][3], [npts][2]
    int32_t *off_dev = nullptr, *npt_dev = nullptr;   // d.off and d.npt, writable: the solve uploads off / npt, a gather counts into npt_dev
    int32_t* nmark = nullptr;                         // [nframes] board markers of a frame
    int32_t* bids = nullptr;                          // [nboard]
    float* bobj = nullptr;                            // [nboard][12]
    std::vector<int32_t> off, npt;
};
int calib_views_of_points(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device, CalibViews* v);
int calib_views_of_batch(arucohip_handle* h, int nframes, const BoardDef& board, int min_markers, int32_t* used, arucohip_handle** owner,
                         CalibViews* v);
int calib_solve(arucohip_handle* h, const CalibViews& v, CalibState st, bool focal_start, double intr[9], double* rvecs, double* tvecs,
                double* per_view_rms, double* rms);
// the fisheye run's start state from (model, flags) (capi_fisheye.hip)
int calib_fisheye_state(arucohip_handle* h, int W, int H, int flags, const arucohip_fisheye_t* model, CalibState* st);
