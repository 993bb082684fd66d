// Internal device-side data layout of libarucohip (MI355X / gfx950). Not part of the C ABI.
//
// HBM layout per handle (F = frames in the batch, T = threshold planes per frame, P = F*T planes):
//   thres [P][H][W] u8   thresholded image (API-visible product, MarkerDetector::getThresholdedImage)
//   tiles [P][H/8+1][W/8+1] u64 binary image cv::findContours works on, 8x8-pixel tiles (1-px frame cleared, zero pad row/col)
//   raw   [P][capR] u32x2 segment mode only: waypoint cracks {start candidate, pos << 2 | code}
//   trig  [P][capT] u32x2 candidates that pass the run rule
//   cdesc [P][capC]      borders that passed the size filter {plane, start, hole, n, key, pool offset}
//   pool  [P][capPts] short2 contour points (checkpoints in front of each border's points)
//   quads [F][capQ]      4-vertex convex polygons
//   cands [F][capC]      ordered candidates with decode result and refined corners
//   markers [F][capM]    arucohip_marker_t
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arucohip.h"
#include "lm_device.h"

namespace ah {

constexpr int WAVE = 64;
constexpr int TRIG_CNT_STRIDE = 32;   // uint32 words between per-plane counters (one 128-byte line per plane)
constexpr int TC_CDESC = 2;           // words of a plane's trig_cnt line: 0 / 1 = outer / hole start candidates,
constexpr int TC_POOL = 3;
constexpr int TC_STATUS = 5;          // 5 = overflow bits (StatusBits) of THIS plane: a frame whose planes carry any is reported with n = -1
constexpr int TC_SNAP = 4;            // 4 = descriptors that existed when the late walker generations were forked            // 2 = contour descriptors, 3 = contour points allocated (per plane: no global hot counter)
constexpr int TC_LATE = 6;            // 6 = descriptors of the plane's late list (from the top of its cdesc array downwards): the borders a pipeline
                                      //     lane's late walks keep while contour_quad's first pass runs (k_contours.hip: late_quad_kernel)
constexpr int WALK_BLOCKS = 16;       // 64-lane walker workgroups per plane
constexpr int MAX_CANDS_PER_FRAME = 512;   // the largest candidates_per_frame a handle is created with: per-frame LDS arrays of the tail are this long


enum Counter {
    CNT_NMARK = 0,     // entries of the flat marker list (all frames)
    CNT_UNUSED1 = 1,
    CNT_UNUSED2 = 2,
    CNT_STATUS = 3,    // overflow bit flags
    CNT_NCAND = 5,     // entries of the flat candidate list (all frames)
    CNT_FIXED = 8      // per-frame counters follow: [CNT_FIXED + f] = quads of frame f
};

enum StatusBits {
    ST_TRIG_OVERFLOW = 1,
    ST_CDESC_OVERFLOW = 2,
    ST_POOL_OVERFLOW = 4,
    ST_QUAD_OVERFLOW = 8,
    ST_CAND_OVERFLOW = 16,
    ST_MARKER_OVERFLOW = 32,
    ST_SEGMENT_ERROR = 64,
};

// a device list overflowed while working on `plane`: the batch-wide status word (the call's return code) and the plane's own word (which
// frame to give up on: the other frames' results stay valid; the reference has no limits, src/markerdetector.cpp:496-635)
__device__ __forceinline__ void flag_overflow(uint32_t* counters, uint32_t* trig_cnt, int plane, uint32_t bit) {
    atomicOr(&counters[CNT_STATUS], bit);
    atomicOr(&trig_cnt[(size_t)plane * TRIG_CNT_STRIDE + TC_STATUS], bit);
}

struct ContourDesc {
    int32_t plane;     // frame*T + t
    int16_t x0, y0;    // start pixel
    int32_t hole;
    int32_t n;         // number of points
    uint32_t key;      // raster index of the scan transition (y*W + x_trigger)
    uint32_t pool_off; // first point in pool
    uint32_t ck_off;   // checkpoints of the border: word offset into walk_scratch, or 0xFFFFFFFF = in front of the points
    uint32_t pad_;
};

struct Quad {
    int16_t x[4], y[4];
    int32_t cdesc;     // index into cdesc list
    uint32_t key;      // ordering key inside the frame: t << 26 | (0x3FFFFFF - raster)  (ascending = reference order)
    int32_t pad_;
};

struct Cand {
    float c[8];        // current corners (x0,y0,...)
    int16_t qx[4], qy[4];  // integer corners after orientation normalisation (detectRectangles output)
    int32_t cdesc;
    int32_t swapped;   // contour must be read reversed
    int32_t id;        // -1 = not a marker
    int32_t nrot;
};

struct FrameGeom {
    int width, height;
    size_t row_stride, frame_stride;   // of the input gray frames
};

struct CamModel {
    int has_K, has_dist;
    float K[9];
    double k[8];       // k1,k2,p1,p2,k3,k4,k5,k6 (zero padded)
    float marker_size;
    int y_perp;
};

struct DetectParams {
    int thres_method;
    int block[16];      // per threshold plane: block size (ADPT) (already fixed up to odd >= 3)
    double p1[16];      // per plane param1 (FIXED uses it as the threshold)
    int idelta;         // floor(param2)
    int nthr;           // planes per frame
    int corner_method;
    int warp_size;
    int min_contour, max_contour;   // contour length bounds (exclusive)
    int bx0, by0, bx1, by1;         // valid region of the border filter [bx0,bx1) x [by0,by1)
    int subpix_win;
    int locked, locked_wsize;       // _useLockedCorners and the window of findCornerMaxima (int(_thresParam1))
    // decoder: 0 = 5x5 fiducial, 1 = highly reliable markers with the handle's dictionary, 2 = host callback (the device
    // only warps; ids come back through launch_set_decoded)
    int decoder;
    int hrm_n, hrm_count;
    uint32_t hrm_correction;        // largest Hamming distance that is still corrected
    const uint64_t* hrm_codes;      // device
    int pyr;                        // MarkerDetector::pyrDown level: threshold, contours and quads run on the frame reduced pyr times (0: on the frame itself)
};

// Environment switches (INTEGRATION.md "Environment knobs"). read_env() (capi.hip) reads them once, when the caller creates a handle;
// its chunk workers, pipeline lanes and retry handle take that record instead of reading the environment again, so a handle and
// everything made for it behave the same for their whole life whatever the environment does later. Each switch stays because
// callers or tests need it; no kernel launcher touches the environment.
struct EnvSettings {
    int streams = 1;       // ARUCOHIP_STREAMS: chunk workers per handle
    int graph = 1;         // ARUCOHIP_GRAPH=0: no single-frame graph (the eager reference of the graph path)
    int contours = -1;     // ARUCOHIP_CONTOURS: 0 walkers, 1 waypoint segments, -1 by handle shape (create_handle)
    int grid = 16;         // ARUCOHIP_GRID: waypoint spacing of the segment pipeline
    int thres_lazy = 1;    // ARUCOHIP_THRES_BYTES=1 clears it: the threshold kernel always writes the byte image
    int quad_dual = 1;     // ARUCOHIP_QUAD_DUAL=0: one border per wave in contour_quad (round 3), the reference of two borders of <= 512 points per wave
#ifdef ARUCOHIP_STAGE_EXPERIMENT
    int stop_after = 99;   // stage-cost experiment (tools/stage_cost.sh builds a variant library with this flag and reads ARUCOHIP_STOP_AFTER):
                           // 1 threshold, 2 start candidates, 3 first walker pass, 4 generations, 5 contour_quad, 6 frame_candidates, 7 warp + Otsu, 8 LINES
#endif
};
// RUN_STAGE(env, n): does the pipeline run past stage n? Always, except in the stage-cost experiment's variant build, where the pipeline is cut
// behind the stage ARUCOHIP_STOP_AFTER names (results are then meaningless; arucohip_build_info() names the flag and bench.py prints no headline).
#ifdef ARUCOHIP_STAGE_EXPERIMENT
#define RUN_STAGE(env, n) ((env).stop_after > (n))
#else
#define RUN_STAGE(env, n) true
#endif

// Border lines of a thresholded plane kept beside the bit tiles (lazy byte image): row 0 at 0, row H-1 at Wp, column 0 at 2 Wp, column W-1
// at 2 Wp + Hp, with Wp / Hp = width / height rounded up to 16 so that every line starts 16-byte aligned (the kernels store 16 and 4 bytes
// at a time) and the virtual rows that complete the last tile row have somewhere to go.
__host__ __device__ inline size_t thres_edge_wp(int W) { return (size_t)((W + 15) & ~15); }
__host__ __device__ inline size_t thres_edge_hp(int H) { return (size_t)((H + 15) & ~15); }
__host__ __device__ inline size_t thres_edge_stride(int W, int H) { return 2 * thres_edge_wp(W) + 2 * thres_edge_hp(H); }

// device pointers + capacities handed to kernels
struct Buffers {
    EnvSettings env;
    uint8_t* thres;
    uint64_t* tiles;       // [P][tiles_y(H)][tiles_x(W)] binary image in 8x8-pixel tiles (bits_tiles.h)
    uint64_t* tile_bits;   // [P][tiles_y(H)][2 * tile_strips(W)] non-empty-tile bitmap: per 128-tile strip one word for the even
                           // tiles (bit i = tile 128 s + 2 i) and one for the odd ones (tile 128 s + 2 i + 1)
    uint2* raw;            // [P][cap_raw] waypoint cracks per plane (segment mode)
    uint32_t* raw_cnt;     // [P * TRIG_CNT_STRIDE] fill level of each plane's raw list (one counter per 128-byte line)
    uint2* trig;           // [P][cap_trig] candidates that pass the run rule
    uint32_t* trig_cnt;    // [P * TRIG_CNT_STRIDE]
    uint2* gen_buf;        // [P][cap_trig] storage of the long-walk generation lists (states + ring ids)
    uint32_t* ring_cnt;    // [P * TRIG_CNT_STRIDE] checkpoint rings handed out per plane (outer, hole)
    uint32_t* gen_cnt;     // counters of the long-walk generation lists (k_contours.hip), zeroed per batch
    ContourDesc* cdesc;
    short2* pool;
    uint8_t* thres_edge;    // [P][thres_edge_stride(W, H)] border lines of the thresholded planes when the byte image is left out (k_threshold.hip)
    uint64_t* thr_stamps;   // timing: per-wave device-clock stamps of the wide threshold kernel [2 * waves]
    uint64_t* thr_acc;      // timing: {clock ticks, launches} accumulated by stamp_reduce_kernel
    int thr_stamp_on;       // stamps are taken (arucohip_enable_timing)
    uint32_t* walk_scratch; // checkpoint rings of the long walks [P][2][LONG_CAP][max_contour/16]
    uint4* node;            // [P][cap_raw] waypoint records of the segment pipeline
    uint4* skipn;           // [P][cap_raw] a node's 8th successor, smallest key and visits of the 8 segments up to it (one frame per call: k_segments.hip)
    unsigned long long* stamp; // [P][cap_raw] (start key, start node, offset) of the start that owns the node
    uint32_t* hash;         // [P][hash_mask+1] node index by waypoint key
    uint32_t hash_mask;
    Quad* quads;
    Cand* cands;
    int32_t* ncands;       // [F]
    uint32_t* cand_list;   // flat list over all frames: frame << 16 | index, counters[CNT_NCAND] entries
    double* iM;            // [cap_flat][9] inverse homographies
    uint16_t* hist;        // [cap_flat][256] patch histograms
    int32_t* othr;         // [cap_flat] Otsu thresholds
    uint8_t* patches;      // [cap_flat][warp_size^2] canonical patches, where something reads them (decode_from_cells: nothing does)
    uint8_t* cells;        // [cap_flat][64] medians of the 7 x 7 cells of a 56 x 56 patch, 8 to a row (decode_from_cells)
    uint32_t cap_flat;
    arucohip_marker_t* markers;
    int32_t* nmarkers;     // [F]
    uint32_t* marker_list; // flat list over all frames: frame << 16 | index, counters[CNT_NMARK] entries (the pose kernel's work list)
    uint32_t* counters;
    uint32_t cap_raw, cap_trig;   // per plane
    uint32_t long_cap;            // checkpoint rings (long walks) per plane and kind
    int seg_mode, grid_mask;      // contour pipeline: 0 = walkers, 1 = waypoint segments (grid spacing = grid_mask + 1)
    uint32_t cap_cdesc, cap_pool;   // per plane: cdesc [P][cap_cdesc], pool [P][cap_pool]
    int cap_quads, cap_cands, cap_markers;   // per frame
};

// Every kernel after the threshold pass is a chain of dependent steps on few wavefronts. With batches in flight its waves
// share SIMDs with the next batch's streaming threshold waves, which are always ready to issue; at equal priority the
// dependent chain only gets every n-th issue slot. Raised priority lets the sparse chains issue whenever they can — they leave
// most slots to the streaming waves anyway.
#ifndef LBP_PRIO
#define LBP_PRIO 3
#endif
__device__ __forceinline__ void latency_bound_priority() { if (LBP_PRIO > 0) __builtin_amdgcn_s_setprio(LBP_PRIO); }
// The kernels with many busy waves (contour_quad, warp_hist, start candidates): between the streaming pass and the sparse chains
#ifndef LBP_PRIO_HEAVY
#define LBP_PRIO_HEAVY LBP_PRIO
#endif
__device__ __forceinline__ void throughput_bound_priority() { if (LBP_PRIO_HEAVY > 0) __builtin_amdgcn_s_setprio(LBP_PRIO_HEAVY); }

// ---- kernel launchers (host side, defined in the .hip files)
void launch_bgr2gray(hipStream_t s, const uint8_t* bgr, size_t row_stride, size_t frame_stride, int width, int height, int nframes, uint8_t* gray);
// How a caller's frames are stored (arucohip_frame_format_t as the host code carries it): format is an arucohip_pixel_format, bits belongs to
// GRAY16, chroma_offset to NV12 (0: the U,V plane follows the Y plane's last row)
struct FrameFmt {
    int format, bits;
    size_t chroma_offset;
};
// camera-native frames (k_ingest.hip) -> dst_channels = 1 (grey) or 3 (B,G,R) at dst_row_stride / dst_frame_stride; fmt and the geometry are valid
void launch_ingest(hipStream_t s, const FrameFmt& fmt, const uint8_t* src, size_t row_stride, size_t frame_stride, int width, int height, int nframes,
                   int dst_channels, uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride);
// frames out (k_egress.hip): 8-bit frames of src_channels = 1 (grey) or 3 (B,G,R) -> the format fmt at dst_row_stride / dst_frame_stride;
// fmt is one of the accepted destinations and the geometry is valid. grey_is_luma: a grey source is the Y of a YUV destination as it lies
void launch_egress(hipStream_t s, const uint8_t* src, int src_channels, size_t src_row_stride, size_t src_frame_stride, int width, int height, int nframes,
                   const FrameFmt& fmt, bool grey_is_luma, uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride);
// cv::pyrDown of nframes 8-bit frames (k_pyrdown.hip): W x H at src_row / src_frame -> (W + 1) / 2 x (H + 1) / 2 at dst_row / dst_frame
void launch_pyr_down(hipStream_t s, const uint8_t* src, size_t src_row, size_t src_frame, int W, int H, int nframes, uint8_t* dst, size_t dst_row,
                     size_t dst_frame);
struct ThrPlan;   // thr_plan.h
// executed (optional): the plan the launch executed, for the handle to keep (arucohip_debug_threshold_plan)
bool launch_threshold(hipStream_t s, const uint8_t* gray, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b, bool lazy,
                      ThrPlan* executed = nullptr);
void launch_expand_thres(hipStream_t s, const FrameGeom& g, int plane, const Buffers& b);
void launch_undist_map(hipStream_t s, int W, int H, const float* K, const float* dist, int ndist, short2* xy, uint16_t* fxy);
void launch_remap(hipStream_t s, const uint8_t* src, size_t row_stride, size_t frame_stride, int W, int H, int cn, int nframes, const short2* xy,
                  const uint16_t* fxy, uint8_t* dst);
// Plane rectification (k_rectify.hip): dst pixel (u, v) of frame f = src frame f sampled at cam(maps[f] * (u, v, 1)), the rule arucohip.h
// states at arucohip_warp_plane_batch. The camera: px = fx * x' + cx with the Brown polynomial k (dist: all of it, else skipped);
// no camera is fx = fy = 1, cx = cy = 0. valid may be null (every frame valid).
struct PlaneWarp {
    const uint8_t* src;
    size_t row_stride, frame_stride;
    int width, height;
    const double* maps;     // [nframes][9], row-major
    const int32_t* valid;   // [nframes]
    double fx, fy, cx, cy, k[8];
    uint8_t* dst;
    size_t dst_row_stride, dst_frame_stride;
    int out_width, out_height;
};
void launch_plane_warp(hipStream_t s, const PlaneWarp& a, int cn, bool dist, int nframes);
// maps[f] / valid[f] of the window `win` on the plane of boards[f]
void launch_plane_maps(hipStream_t s, const arucohip_board_t* boards, int nframes, const arucohip_rectify_t& win, double* maps, int32_t* valid);
// Plane compositing (k_composite.hip): frame pixel (u, v) of frame f is blended, in place, with the texture sampled at
// maps[f] * ray(u, v), the rule arucohip.h states at arucohip_composite_plane_batch. K: the caller's, or the identity without a camera
// (the ray is then (u, v) bit for bit); k: the Brown coefficients (dist: five iterations of undistort_point, else none). valid and masks
// may be null. Everything is a device address.
struct PlaneComposite {
    uint8_t* frames;
    size_t row_stride, frame_stride;
    int width, height;
    const uint8_t* tex;
    size_t tex_row_stride, tex_frame_stride;   // tex_frame_stride 0: one texture for every frame
    int tex_width, tex_height, opacity;
    const double* maps;     // [nframes][9], row-major
    const int32_t* valid;   // [nframes]
    const uint8_t* masks;   // [nframes][height][width]
    float K[9];
    double k[8];
};
void launch_plane_composite(hipStream_t s, const PlaneComposite& a, int cn, bool alpha, bool dist, int nframes);
// maps[f] / valid[f]: the signed adjugate of the map of `win` on the plane of boards[f]
void launch_plane_inverse_maps(hipStream_t s, const arucohip_board_t* boards, int nframes, const arucohip_rectify_t& win, double* maps, int32_t* valid);
// fisheye lenses (k_fisheye.hip; the model is fisheye_device.h's)
struct FisheyeCam;
void launch_fisheye_points(hipStream_t s, const FisheyeCam& cam, const float* src, int n, int undistort, float* dst, uint8_t* valid);
void launch_fisheye_markers(hipStream_t s, const FisheyeCam* cams, int nmodels, int first, int nframes, const Buffers& b, int32_t* dropped);
void launch_fisheye_map(hipStream_t s, const FisheyeCam& cam, int W, int H, short2* xy, uint16_t* fxy);
int launch_canny(hipStream_t s, const uint8_t* gray, const FrameGeom& g, int nframes, int nthr, const Buffers& b, uint64_t* surv, uint64_t* edge, uint32_t* changed);
void launch_erode(hipStream_t s, const FrameGeom& g, int nplanes, const Buffers& b, uint8_t* tmp);
size_t erode_tiles_tmp_bytes(const FrameGeom& g, int nplanes);
void launch_erode_tiles(hipStream_t s, const FrameGeom& g, int nplanes, const Buffers& b, uint8_t* tmp);   // on the lazy byte image (tiles + border lines)
void launch_tile_bitmap(hipStream_t s, const FrameGeom& g, int nplanes, const Buffers& b);
void launch_binary_planes(hipStream_t s, const uint8_t* thres_in, const FrameGeom& g, int nframes, const Buffers& b);
void launch_start_candidates(hipStream_t s, const FrameGeom& g, int nplanes, const Buffers& b, int min_contour = 0);
// Where a batch's late walker generations run. A handle that has the GPU to itself while its batch runs (a synchronous call, one frame per call and
// its graph, a chunk worker) owns a side stream and forks them onto it; a pipeline lane owns none (create_handle decides, once per handle): the
// other lanes' batches fill the chip while its chain runs, and its whole batch stays on the lane's one stream.
struct WalkFork {
    hipStream_t side;            // stream of the late walker generations; null: no fork, every generation on the batch's stream
    hipEvent_t forked, joined;   // used only with a side stream
    hipEvent_t after_first;      // recorded behind the first pass (per-kernel timing), may be null
};
enum WalkTail { WALKS_DONE = 0, WALKS_FORKED = 1, WALKS_LATE = 2 };   // what launch_walkers leaves to its caller (k_contours.hip)
int launch_walkers(hipStream_t s, const WalkFork& fk, const FrameGeom& g, int nplanes, const DetectParams& p, const Buffers& b);
size_t walk_scratch_words(int nplanes, const DetectParams& p, uint32_t long_cap);   // capacity launch_walkers needs in Buffers::walk_scratch
constexpr int GEN_FORK_AFTER = 3;   // generations in front of the fork; a walk that enters generation GEN_FORK_AFTER + 1 is a "late" one
size_t gen_cnt_word(int kind, int gen, int sublist);   // index into Buffers::gen_cnt of the entry count of a generation list (kind 0 outer, 1 hole; sublist 0..7)
constexpr size_t GEN_CNT_WORDS = 2 * 32 * 32 * 8;                 // words of Buffers::gen_cnt: [2 kinds][GEN_MAX + 2 generations][8 sublists] lines of 32 words
void launch_segments(hipStream_t s, const FrameGeom& g, int nplanes, const DetectParams& p, const Buffers& b);
void launch_contour_quads(hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b, int pass = 0);
void launch_late_quads(hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b);   // behind WALKS_LATE: late walks + every quad pass
void launch_frame_candidates(hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b);
// p.pyr > 0, behind launch_frame_candidates: kept borders (points, start pixels) and candidates (integer quads, corners) times 1 << p.pyr, in place
void launch_lift(hipStream_t s, int nframes, const DetectParams& p, const Buffers& b);
// warp + histogram, Otsu threshold, id / rotation of every candidate (left in Cand; the caller's decoder: warp only). decode_from_cells: the batch
// takes the variant that keeps 49 cell medians per candidate instead of the stored patch and decodes in otsu_kernel (k_decode.hip).
// fused_cells: the built-in 5x5 decoder on a stored patch runs as the head of refine_lines_kernel (launch_refine_lines with the same flag) instead of
// a kernel of its own; never together with decode_from_cells
bool decode_from_cells(const FrameGeom& g, int nframes, const DetectParams& p);
void launch_decode(hipStream_t s, const uint8_t* gray, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b, bool fused_cells = false);
// test hook: the inverse homographies (b.iM) of the first n entries of the flat candidate list, from the candidates' integer corners
void launch_stage_quads(hipStream_t s, const Buffers& b, uint32_t n, int ws);
void launch_set_decoded(hipStream_t s, const Buffers& b, uint32_t n, const int2* id_nrot_dev);
void launch_refine_lines(hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& p, const CamModel& cam, const Buffers& b, bool fused_cells = false);
void launch_locked_corners(hipStream_t s, const uint8_t* gray, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b);
void launch_refine_pixels(hipStream_t s, const uint8_t* gray, const FrameGeom& g, int nframes, const DetectParams& p, const Buffers& b);
void launch_finalize(hipStream_t s, const FrameGeom& g, int nframes, const DetectParams& p, const CamModel& cam, const Buffers& b, arucohip_marker_t* out = nullptr,
                     int out_cap = 0, int32_t* n_out = nullptr);   // out / n_out: the caller's device arrays, written as well (no pose to add later)
void launch_pose(hipStream_t s, int nframes, const CamModel& cam, const Buffers& b);
void launch_warp_only(hipStream_t s, const uint8_t* gray, const FrameGeom& g, const float* quad_dev, int size, uint8_t* dst_dev);
void launch_pnp_points(hipStream_t s, const float* obj, const float* img, int npts, const CamModel& cam, double* rt_out, int* ok_out);
void launch_project_points(hipStream_t s, const float* obj, int npts, const double* rt, const CamModel& cam, float* img_out);
void launch_gl_modelview(hipStream_t s, int nframes, int cap, const Buffers& b, double* out_dev);
void launch_marker_pose(hipStream_t s, arucohip_marker_t* markers, int n, const CamModel& cam);

// A board, the one record of it: the caller's arrays on the host, the uploaded ones (upload_board, handle.h) where a kernel reads it.
struct BoardDef {
    const int32_t* ids;
    const float* obj;      // nboard * 4 * 3
    int nboard, info_type;
    float marker_size, repj_thres;
};
// metres per unit of the board's object points: a PIX board is scaled by the marker side taken from the first edge of marker 0
// (board_side; a METERS board's marker side is that edge itself). A PIX board without a marker size has no scale: nothing solves it.
__host__ __device__ inline double board_side(const float* obj) {
    const float dx = obj[0] - obj[3], dy = obj[1] - obj[4], dz = obj[2] - obj[5];   // Point3f difference in float, cv::norm in double
    return sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
}
__host__ __device__ inline double board_mpp(const BoardDef& bd) {
    return (bd.info_type == ARUCOHIP_BOARD_PIX && bd.marker_size > 0) ? (double)bd.marker_size / board_side(bd.obj) : 1.0;
}
void launch_board_pose(hipStream_t s, int nframes, const Buffers& b, const BoardDef& bd, const CamModel& cam, arucohip_board_t* out, float* prob);

// Board marker recovery (k_recover.hip; arucohip_board_recover_batch). A worker's scratch: per frame the first entry of its block in the flat
// candidate list, the adoptions of the matching pass, and the lists the refinement and the per-marker solver walk.
struct RecoverRec {
    int32_t board, cand, nrot, old_nrot;   // board entry, candidate index in the frame, rotation adopted, the rotation the decoder had left
};
struct RecoverBufs {
    int32_t* base;        // [F] index in Buffers::cand_list of the frame's candidate 0
    int32_t* nrec;        // [F] adoptions of the matching pass
    RecoverRec* rec;      // [F][cap_markers]
    uint32_t* rlist;      // [F][cap_markers] frame << 16 | candidate: what launch_refine_recovered walks
    uint32_t* plist;      // [F][cap_markers] frame << 16 | marker index of the recovered markers, 0xFFFFFFFF: none (launch_pose_sparse)
    int32_t* recovered;   // [F] markers inserted
    uint32_t* status;     // bit 0: a frame's marker list was full
};
struct RecoverArgs {
    BoardDef bd;          // device arrays
    float max_corner_dist;
    int max_cell_errors, min_markers;
    int cells_valid, ws;             // votes from Buffers::cells, else from the stored patches of side ws
    int bx0, by0, bx1, by1;          // finalize_kernel's border rectangle
};
void launch_recover_match(hipStream_t s, int list_frames, int nframes, const Buffers& b, const RecoverArgs& a, const CamModel& cam, const RecoverBufs& r);
void launch_recover_insert(hipStream_t s, int nframes, const Buffers& b, const RecoverArgs& a, const CamModel& cam, const RecoverBufs& r,
                           arucohip_board_t* boards, float* prob);
// refine_one (k_refine.hip) on the candidates of r.rlist, with this call's camera
void launch_refine_recovered(hipStream_t s, int nframes, int corner_method, const CamModel& cam, const Buffers& b, const uint32_t* rlist,
                             const int32_t* nrec, int stride);
// the per-marker solver (k_finalize.hip) over a list with holes: nlist entries frame << 16 | index, 0xFFFFFFFF = none
void launch_pose_sparse(hipStream_t s, const Buffers& b, const uint32_t* list, uint32_t nlist, const CamModel& cam);

// Both planar pose solutions per marker (k_planar.hip): markers[0 .. n) -> out[0 .. n), or the markers of the first nframes of the list_frames
// frames a worker's lists hold -> out[(first + f) * cap_out + i]
void launch_planar_poses(hipStream_t s, const arucohip_marker_t* markers, int n, const CamModel& cam, int refine, arucohip_planar_poses_t* out);
void launch_planar_poses_list(hipStream_t s, int list_frames, int nframes, int first, const Buffers& b, const CamModel& cam, int refine,
                              arucohip_planar_poses_t* out, int cap_out);

// Overlays (k_overlay.hip). Scratch of one call: a 32-byte record per marker slot (the box of its primitives and their number), then
// OV_SLOTS primitives of 32 bytes per slot, in painting order. A marker needs at most 16 (outline) + 14 ("id=" and eleven characters) +
// 6 (axis) + 12 (cube) = 48 of them; a board takes one slot.
constexpr int OV_SLOTS = 48;
constexpr size_t OV_REC_BYTES = 32, OV_PRIM_BYTES = 32 * OV_SLOTS;
void launch_overlay_build_markers(hipStream_t s, const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap, const CamModel& cam,
                                  int flags, int line_width, uint32_t color, void* recs, void* prims);
void launch_overlay_build_boards(hipStream_t s, const arucohip_board_t* boards, int nframes, const CamModel& cam, int flags, float marker_size, void* recs,
                                 void* prims);
void launch_overlay_raster(hipStream_t s, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride, size_t frame_stride,
                           const void* recs, const void* prims, int cap);

// Mesh rendering (k_render.hip): shaded triangle meshes at marker and board poses, the rule arucohip.h states at
// arucohip_render_markers_batch. Scratch of one chunk of frames, per instance slot (`slots` per frame: cap for markers, 1 for boards):
// one 80-byte instance record (pose, product of the scales, box), nverts 40-byte transformed vertices, ntris 64-byte triangle records.
constexpr size_t RD_INST_BYTES = 80, RD_VERT_BYTES = 40, RD_TRI_BYTES = 64;
struct RdMesh {
    const float* vertices;
    const int32_t* triangles;
    const uint8_t* colors;   // may be null: RdStyle::color
    int nverts, ntris;
};
struct RdStyle {
    int flags, opacity, ambient;
    uint32_t color;      // B | G << 8 | R << 16
    double light[3];     // unit, towards the light, camera frame
    double scale;
};
void launch_render_instances_markers(hipStream_t s, const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap, double scale,
                                     void* insts);
void launch_render_instances_boards(hipStream_t s, const arucohip_board_t* boards, int nframes, double scale, void* insts);
// insts [ninst] -> verts [ninst][nverts], tris [ninst][ntris] and the instances' boxes
void launch_render_build(hipStream_t s, void* insts, int ninst, const CamModel& cam, const RdMesh& mesh, const RdStyle& style, void* verts, void* tris);
// masks: null, or nframes images of `width` bytes a row, mask_row / mask_frame bytes apart
void launch_render_raster(hipStream_t s, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride, size_t frame_stride,
                          const uint8_t* masks, size_t mask_row, size_t mask_frame, const void* insts, const void* tris, int slots, int ntris,
                          const RdStyle& style);

// Camera calibration (k_calib.hip). Views: points obj (xyz) / img (xy) at off[v], npt[v] points each.
constexpr int CALIB_MAX_POINTS = 512;   // points of one view (= the board kernels' MAX_BOARD_POINTS)
constexpr int CALIB_RED = 100;          // doubles per view of the reduced system: S_i (81), diag A_i (9), rhs_i (9), pad
constexpr int CALIB_BS = 60;            // doubles per view for the back-substitution: u (6), M (6 x 9)
enum { CALIB_ERR_DEGENERATE = 1, CALIB_ERR_NONPLANAR = 2 };
enum { CALIB_MODEL_PINHOLE = 0, CALIB_MODEL_FISHEYE = 1 };   // fisheye: intr = fx fy cx cy k1 k2 k3 k4 and a ninth entry that stays 0

struct CalibState {
    LmCtl lm;          // cost at intr / pose[cur]; sdn, spn and solve_failed stay 0: the intrinsic step is in cand / delta
    double intr[9];    // fx fy cx cy k1 k2 p1 p2 k3
    double cand[9], delta[9];
    double aspect;     // fx / fy under ARUCOHIP_CALIB_FIX_ASPECT_RATIO
    int32_t flags, free_mask, model, pad_;   // model: CALIB_MODEL_*
};

struct CalibDev {
    const float* obj;
    const float* img;
    const int32_t* off;
    const int32_t* npt;
    int nviews;
    double* init;      // [V][6] rows of the focal-length least squares
    double* red;       // [V][CALIB_RED]
    double* bs;        // [V][CALIB_BS]
    double* pose;      // [2][V][6] rvec, tvec (current / candidate, swapped by st->cur)
    double* vcost;     // [2][V]
    double* vchg;      // [V][2] |pose step|^2, |pose|^2
    CalibState* st;
};

void launch_calib_init(hipStream_t s, const CalibDev& d, bool guess);
void launch_calib_iteration(hipStream_t s, const CalibDev& d);
// bd: device arrays; mpp: board_mpp of the board
void launch_calib_gather(hipStream_t s, int nframes, const Buffers& b, const BoardDef& bd, double mpp, int first, float* obj, float* img,
                         int32_t* npt, int32_t* nmark);

// Marker mapping (k_map.hip): the rigid placement of nboard markers in the frame of the first, from frames that show several of them.
constexpr int MAP_MAX_MARKERS = 64;     // listed markers (ARUCOHIP_MAP_MAX_MARKERS)
constexpr int MAP_SLOTS = 16;           // listed markers used per frame (ARUCOHIP_MAP_MAX_FRAME_MARKERS): 4 lanes each, one wave per frame
constexpr int MAP_REC = 116;            // doubles per frame and slot: V_m (36), W_m (36), Y_m (36), g_m - W_m u (6), pad
enum { MAP_ERR_NO_REFERENCE = 1, MAP_ERR_TOO_FEW = 2, MAP_ERR_DEGENERATE = 4 };

struct MapState {
    LmCtl lm;          // cost at mpose[cur] / fpose[cur]; the shared block is the markers
    double intr[9];    // fx fy cx cy k1 k2 p1 p2 k3 (fixed)
    int32_t nmapped, nused, nobs, pad_;
};

struct MapDev {
    int nframes, nboard, min_markers;
    float half;                 // half the marker side, in the float rounding of Marker::getObjectPoints
    // observations: obs_frame != nullptr: nobs entries in any order; else frame f owns obs_cnt[f] entries from f * obs_stride
    const int32_t* obs_frame;
    const int32_t* obs_id;
    const float* obs_corners;   // 8 per observation
    const int32_t* obs_cnt;
    int nobs, obs_stride;
    const int32_t* ids;         // [nboard]
    int8_t* slot;               // [F][MAP_MAX_MARKERS] slot of board marker m in frame f, -1: absent
    int8_t* fm;                 // [F][MAP_SLOTS] board marker of a slot
    int32_t* fn;                // [F] slots taken
    int32_t* used;              // [F]
    float* fc;                  // [F][MAP_SLOTS][8] corners
    double* fT;                 // [F][MAP_SLOTS][12] the marker's planar pose in the frame: R (9), t (3)
    double* fq;                 // [F][MAP_SLOTS] its confidence rms[1] / rms[0]
    int32_t* edge_f;            // [MAP_MAX_MARKERS][MAP_MAX_MARKERS] the frame an edge takes its transform from, -1: no edge
    double* edge_q;             // its score
    int32_t* mapped;            // [nboard]
    double* mpose;              // [2][nboard][6] rvec, tvec of every marker in the frame of marker 0 (current / candidate)
    double* fpose;              // [2][F][6] board pose of every frame
    double* rec;                // [F][MAP_SLOTS][MAP_REC]
    double* fu;                 // [F][6] u = U~^-1 g_p
    double* S;                  // [N][N] the reduced system (lower triangle; its Cholesky factor after the solve), N = 6 (nboard - 1)
    double* delta;              // [N] reduced right-hand side, then the marker step
    double* vcost;              // [2][F]
    double* vchg;               // [F][2]
    double* scost;              // [F][MAP_SLOTS] squared residuals of a slot's four corners
    float* obj;                 // [nboard][12]
    MapState* st;
};

void launch_map_gather(hipStream_t s, int nframes, const Buffers& b, int first, int stride, int32_t* obs_id, float* obs_corners, int32_t* obs_cnt);
void launch_map_init(hipStream_t s, const MapDev& d, const CamModel& cam);
void launch_map_iteration(hipStream_t s, const MapDev& d);
void launch_map_finish(hipStream_t s, const MapDev& d);

// Camera rigs (k_rig.hip): the rigid transforms rig -> camera of ncams cameras with fixed intrinsics, and the pose of a board in the rig
// frame from every camera that sees it. View v = instant * ncams + camera.
constexpr int RIG_MAX_CAMERAS = 16;     // ARUCOHIP_RIG_MAX_CAMERAS
constexpr int RIG_MAX_BOARD = 128;      // board markers: a view holds at most RIG_VIEW_POINTS correspondences
constexpr int RIG_VIEW_POINTS = 512;    // = MAX_BOARD_POINTS
constexpr int RIG_MAX_N = 6 * (RIG_MAX_CAMERAS - 1);
constexpr int RIG_J = 13;               // a Jacobian row: 6 camera columns, 6 board-pose columns, the residual
constexpr int RIG_G = RIG_J * (RIG_J + 1) / 2;   // 91 entries of the upper triangle of a view's Gram matrix
constexpr int RIG_REC = 42;             // doubles per view of an eliminated instant: Y_c (36), g_c - W_c u (6)
enum { RIG_ERR_NO_REFERENCE = 1, RIG_ERR_TOO_FEW = 2, RIG_ERR_DEGENERATE = 4 };

struct RigCam {
    CamModel cam;      // for the single-camera start pose
    double in[9];      // fx fy cx cy k1 k2 p1 p2 k3
};

struct RigState {
    LmCtl lm;          // cost at cpose[cur] / ipose[cur]; the shared block is the cameras
    int32_t ncal, nused, npts, pad_;
};

struct RigDev {
    int ncams, ninstants, min_markers;
    BoardDef bd;                // device arrays; repj_thres is not read
    // observations: obs_view != nullptr: nobs entries in any order; else view v owns obs_cnt[v] entries from v * obs_stride
    const int32_t* obs_view;
    const int32_t* obs_id;
    const float* obs_corners;   // 8 per observation
    const int32_t* obs_cnt;
    int nobs, obs_stride;
    const RigCam* cams;         // [ncams]
    int32_t* vn;                // [V] member markers of a view
    int32_t* vok;               // [V] the view counts: >= min_markers member markers and a start pose
    int32_t* vact;              // [V] the view takes part in the solve
    double* vT;                 // [V][12] the view's single-camera board pose: R (9), t (3)
    float* pobj;                // [V][RIG_VIEW_POINTS][3] the view's object points, metres
    float* pimg;                // [V][RIG_VIEW_POINTS][2]
    int32_t* edge_t;            // [RIG_MAX_CAMERAS][RIG_MAX_CAMERAS] the instant an edge takes its transform from, -1: no edge
    int32_t* edge_q;            // its score
    int32_t* calibrated;        // [ncams]
    double* cpose;              // [2][ncams][6] rvec, tvec rig -> camera (current / candidate)
    int32_t* used;              // [T]
    int32_t* lead;              // [T] the first camera of the instant that takes part
    double* ipose;              // [2][T][6] board pose of every instant in the rig frame
    double* gram;               // [V][RIG_G]
    double* rec;                // [V][RIG_REC]
    double* fu;                 // [T][6] u = U~^-1 g_p
    double* S;                  // [N][N] the reduced system (lower triangle; its Cholesky factor after the solve), N = 6 (ncams - 1)
    double* delta;              // [N] reduced right-hand side, then the camera step
    double* vcost;              // [2][V]
    double* vchg;               // [T][2]
    arucohip_board_t* boards;   // [T] rig pose: results
    int32_t* views_used;        // [T]
    RigState* st;
};

void launch_rig_views(hipStream_t s, const RigDev& d);
void launch_rig_calib_init(hipStream_t s, const RigDev& d);
void launch_rig_calib_iteration(hipStream_t s, const RigDev& d);
void launch_rig_calib_finish(hipStream_t s, const RigDev& d);
void launch_rig_pose(hipStream_t s, const RigDev& d);

// Board occlusion mask (k_chromatic.hip): ChromaticMask of the reference, src/chromaticmask.cpp.
constexpr int CHROMA_CELL = 20;       // ChromaticMask::_cellSize
constexpr int CHROMA_MIN_FIT = 10;    // EMClassifier::train fits only when the discretised histogram holds >= 10 samples
constexpr int CHROMA_UPDATE_MIN = 50; // update() retrains the cells with more than 50 raw samples

struct ChromaCam {
    float K[9];
    double k[8];           // k1 k2 p1 p2 k3 (zero padded)
    float corners3d[12];   // the board corners of setParams
    int mc, nc, W, H;
};

// The geometry of one frame (calculateGridImage / classify2), written by chroma_geometry_kernel.
struct ChromaGeom {
    float corners[8];           // projected board corners (projectPoints, float as _imgCornerPoints)
    double Ht[9];               // corners -> (0,0) (20mc-1,0) (20mc-1,20nc-1) (0,20nc-1): calculateGridImage
    double Hc[9];               // corners -> (0,0) (mc-1,0) (mc-1,nc-1) (0,nc-1): classify2, used as float
    int32_t rx0, ry0, rx1, ry1; // classify2's rectangle after fitRectToSize: [rx0, rx1) x [ry0, ry1) (empty when rx1 <= rx0)
    int32_t valid;              // the frame has a pose (and, in a batch, prob > min_prob)
    int32_t pad_;
};

// boards == nullptr: one frame at the pose rvec / tvec; else frame f takes boards[f] (and prob[f] > min_prob when prob != nullptr)
void launch_chroma_geometry(hipStream_t s, const ChromaCam& c, int nframes, const arucohip_board_t* boards, const float* prob, float min_prob,
                            const double* rvec, const double* tvec, ChromaGeom* out);
void launch_chroma_grid(hipStream_t s, const ChromaCam& c, const ChromaGeom* g, uint8_t* cellmap);
// raw[cell][256] += samples of the pixels whose cell-map value (times mask, when given) is not 0; raw must be zeroed by the caller
void launch_chroma_hist(hipStream_t s, int W, int H, const uint8_t* in, size_t row_stride, const uint8_t* cellmap, const uint8_t* mask,
                        uint32_t* raw);
// EMClassifier::train of every cell from its raw-sample histogram; cells with min_raw > 0 and at most min_raw samples are skipped.
// hcount[cell][256]: the discretised histogram; fitted[cell]: 1 fitted, 0 fewer than 10 samples (model kept), -1 skipped.
void launch_chroma_em(hipStream_t s, int ncell, const uint32_t* raw, uint32_t min_raw, double thresh, uint32_t* hcount, int32_t* fitted,
                      double* prob, uint8_t* inside, int32_t* trained);
// classify (method 1) / classify2 (method 2) of nframes frames at geom[f], 3x3 close fused; masks W x H per frame (frame after frame);
// npix[f] += the 1 pixels of frame f (zeroed by the caller) when not null
void launch_chroma_classify(hipStream_t s, const ChromaCam& c, int method, double thresh, int nframes, const uint8_t* frames, size_t row_stride,
                            size_t frame_stride, const ChromaGeom* geom, const double* prob, const uint8_t* inside, uint8_t* masks, int32_t* npix);

// Highly reliable marker dictionaries and boards (k_hrm.hip): createDicitionary / createBoardImage of src/highlyreliablemarkers.cpp.
constexpr int HRM_STATE = 31;           // words of glibc's rand() state (r[i] = r[i-3] + r[i-31])
constexpr int HRM_WINDOW = 65536;       // candidates screened per window
constexpr int HRM_LANE_CANDS = 16;      // consecutive candidates per generating lane
constexpr int HRM_GEN_BLOCK = 256;
constexpr int HRM_LANE_BITS = 12;       // lanes per window = 2^12
constexpr int HRM_DECIDE_BLOCK = 1024;
constexpr int HRM_LIMIT = 100000;       // MAX_UNPRODUCTIVE_ITERATIONS
constexpr int HRM_DBG_RUN = 64;         // outputs per lane of arucohip_debug_hrm_stream
constexpr int HRM_POW_BITS = 48;        // M^(2^b) for b < 48: stream offsets below 2^48
static_assert(HRM_WINDOW == (HRM_LANE_CANDS * HRM_GEN_BLOCK) << (HRM_LANE_BITS - 8), "window = lanes x candidates per lane");
enum { HRM_RUNNING = 0, HRM_DONE = 1, HRM_TAU_ZERO = 2, HRM_INTERNAL = 3 };

// The sequential state of createDicitionary, carried from window to window on the device
struct HrmCtl {
    int32_t tau, count, limit, dsize;
    int64_t base;        // index of the window's first candidate
    int64_t examined;    // index of the last candidate that changed the state (acceptance or tau decrement), plus one
    int32_t status;      // HRM_*
    int32_t windows, accepted, decrements;
};

struct HrmBufs {
    uint32_t* state;     // [31] the stream state at the window's first output
    uint32_t* jumps;     // [HRM_LANE_BITS + 1][31 * 31]: M^(HRM_LANE_CANDS n^2 2^b); the last one advances a whole window
    uint64_t* code;      // [HRM_WINDOW] rotation 0 of every candidate
    uint8_t* selfd;      // [HRM_WINDOW] selfDistance
    uint8_t* dmin;       // [HRM_WINDOW] distance to the dictionary
    uint64_t* dict;      // [dict_size][4] the accepted markers' rotations
    HrmCtl* ctl;
};

// one window: generate, screen against the dictionary, walk the sequential decisions, advance the state
void launch_hrm_window(hipStream_t s, int n, int target, const HrmBufs& b);
// count outputs from `offset` of the stream whose state at output 0 is state0 (pow2: HRM_POW_BITS matrices M^(2^b))
void launch_hrm_stream(hipStream_t s, const uint32_t* state0, const uint32_t* pow2, uint64_t offset, int count, uint32_t* out);
// the board image (gray, or BGR with chromatic) of gw x gh markers; rows of `stride` bytes, a multiple of 16
void launch_hrm_board(hipStream_t s, const uint64_t* codes, int n, int gw, int gh, int chromatic, int W, int H, int channels, size_t stride,
                      uint8_t* out);

// The default 5x5 markers, their boards and marker sets (k_fiducial.hip): src/arucofidmarkers.cpp:214-430, utils/aruco_selectoptimalmarkers.cpp.
// One image of fid_paint_kernel: a gw x gh grid of markers of M pixels (cells of sw = M / 7) at `pitch` on white, GW x GH pixels large,
// at (off, off) of a W x H image. off = 0: the grid is the image (boards, plain markers). off > 0: the "locked" marker, white around the
// grid with a black off x off square in every corner.
// sq > 0: a chessboard of gw x gh squares of sq pixels (arucohip_charuco_board_image): square (sx, sy) is black when sx + sy is even, a white one
// holds the marker of its slot at (moff, moff) inside it; GW, GH, off and pitch are not read.
struct FidLayout {
    int W, H, GW, GH, off;
    int gw, gh, M, pitch, sw;
    int sq, moff;
};
// n images of layout L; slots: [n][gh * gw] marker ids, -1 = the cell stays white. Any row_stride >= W, any alignment.
void launch_fid_paint(hipStream_t s, const FidLayout& L, const int32_t* slots, int nimages, uint8_t* out, size_t row_stride, size_t image_stride);
// dist[1024][1024]: the selection utility's distance of every pair of markers
void launch_fid_distances(hipStream_t s, int32_t* dist);
// the greedy selection of n_markers markers; sel [n_markers] ascending, res [4]: selected, complete, smallest pairwise distance, largest entropy
void launch_fid_select(hipStream_t s, int n_markers, int min_entropy, int32_t* sel, int32_t* res);

// Chessboard-corner boards (k_charuco.hip; capi_charuco.hip).
struct CharucoArgs {
    arucohip_charuco_t L;
    const int32_t* ids;        // device: the layout's marker ids
    const uint8_t* gray;       // the frames of this worker's span
    size_t row_stride, frame_stride;
    int width, height;
    int min_markers, max_win;
};
// one wave per (corner, frame) of the first nframes frames the worker's lists hold; out / n_found: the worker's first frame
void launch_charuco_corners(hipStream_t s, int nframes, const Buffers& b, const CharucoArgs& a, arucohip_charuco_corner_t* out, int32_t* n_found);
// views[v] = {frame, first point}: the found corners of the frame, in corner order, to obj / img from the view's first point; npt[v] = their number
void launch_charuco_gather(hipStream_t s, const arucohip_charuco_t& L, double scale, const arucohip_charuco_corner_t* rec, const int2* views, int nviews,
                           float* obj, float* img, int32_t* npt);
void launch_charuco_pose(hipStream_t s, const arucohip_charuco_t& L, double scale, const arucohip_charuco_corner_t* rec, int nframes, int min_corners,
                         const CamModel& cam, arucohip_board_t* out);

}  // namespace ah
