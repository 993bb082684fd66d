/*
 * arucohip — C ABI of the MI355X-native ArUco marker-detection hot path.
 *
 * This is the drop-in boundary for ONE path of the reference library (paroj/aruco, ArUco 1.3):
 *   aruco::MarkerDetector::detect()   /root/reference/src/markerdetector.h:102-120, .cpp:302-478
 *   aruco::BoardDetector::detect()    /root/reference/src/boarddetector.h:103-108, .cpp:90-205
 * plus the public stage entry points the reference keeps callable (markerdetector.h:255-280).
 * Everything is plain C: pointers, sizes, PODs. No OpenCV, no torch types. The header-only C++ shim in
 * include/aruco_hip_shim.hpp rebuilds the reference's classes on top of these calls.
 *
 * Threading: like the reference object (markerdetector.cpp:334,372-380 mutate members) a handle is not
 * re-entrant. One handle owns one HIP stream and all device buffers; use one handle per host thread.
 */
#ifndef ARUCOHIP_H
#define ARUCOHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARUCOHIP_VERSION 100

/* status codes; mirror the reference's failure modes (CV_Assert -> cv::Exception), SURVEY.md §8b "Errors" */
enum {
    ARUCOHIP_OK = 0,
    ARUCOHIP_E_INVALID = 1,      /* bad argument: what the reference rejects with CV_Assert (markerdetector.cpp:644,685,1032-1034,1048) */
    ARUCOHIP_E_CAPACITY = 2,     /* output array too small; *n_out holds the required count */
    ARUCOHIP_E_UNSUPPORTED = 3,  /* a parameter value outside what the device kernels are built for (warp size > 128, adaptive block > 31,
                                    SUBPIX window > 15, locked-corner window > 31, dictionary markers beyond 8x8 / 4096 entries) */
    ARUCOHIP_E_HIP = 4,          /* HIP runtime failure, see arucohip_last_error_string */
    ARUCOHIP_E_OVERFLOW = 5,     /* an internal device list overflowed for some frame(s): those have n_out = -1, the others are valid
                                    (arucohip_detect_batch_retry_overflowed, or raise the limits with arucohip_create_ex) */
    ARUCOHIP_E_BOARD_CONFIG = 6  /* empty board configuration (boarddetector.cpp:93) */
};

/* MarkerDetector::ThresholdMethods (markerdetector.h:125) */
enum { ARUCOHIP_THRES_FIXED = 0, ARUCOHIP_THRES_ADPT = 1, ARUCOHIP_THRES_CANNY = 2 };
/* MarkerDetector::CornerRefinementMethod (markerdetector.h:192) */
enum { ARUCOHIP_CORNER_NONE = 0, ARUCOHIP_CORNER_HARRIS = 1, ARUCOHIP_CORNER_SUBPIX = 2, ARUCOHIP_CORNER_LINES = 3 };
/* BoardConfiguration::mInfoType (board.h:64) */
enum { ARUCOHIP_BOARD_NONE = -1, ARUCOHIP_BOARD_PIX = 0, ARUCOHIP_BOARD_METERS = 1 };
/* decoder behind MarkerDetector::setMakerDetectorFunction (markerdetector.h:243) */
enum { ARUCOHIP_DECODER_FIDUCIAL_5X5 = 0, ARUCOHIP_DECODER_HRM = 1, ARUCOHIP_DECODER_USER = 2 };

/* 1:1 image of MarkerDetector's private configuration members (markerdetector.h:283-306; defaults .cpp:235-249). */
typedef struct arucohip_params {
    int32_t thres_method;       /* _thresMethod        default ADPT */
    int32_t thres_param1_range; /* _thresParam1_range  default 0    */
    double thres_param1;        /* _thresParam1        default 7    */
    double thres_param2;        /* _thresParam2        default 7    */
    int32_t corner_method;      /* _cornerMethod       default LINES */
    int32_t warp_size;          /* _markerWarpSize     default 56 (>= 10, multiple of 7 recommended) */
    float min_size;             /* _minSize            default 0.04 */
    float max_size;             /* _maxSize            default 0.5  */
    float border_dist;          /* _borderDistThres    default 0.025 */
    int32_t use_locked_corners; /* _useLockedCorners   default 0; with HARRIS / SUBPIX: findCornerMaxima before the refinement */
    int32_t decoder_kind;       /* markerIdDetectorFunc: ARUCOHIP_DECODER_FIDUCIAL_5X5, ARUCOHIP_DECODER_HRM after
                                   arucohip_set_dictionary, ARUCOHIP_DECODER_USER after arucohip_set_decoder_callback */
    int32_t erode;              /* north_star's "optional erosion": != 0 erodes the thresholded image with a 3x3 structuring
                                   element (cv::erode(thres, thres, Mat()) semantics, outside pixels do not erode) before the
                                   contour stage. Default 0: this snapshot of the reference dropped its enableErosion() as a
                                   no-op (PortingManual.md:5-7), so there is no reference result to match */
} arucohip_params_t;

/* aruco::Marker (marker.h:46-53): id, 4 corners (x0,y0,..), ssize, Rvec/Tvec as double. 96 bytes. */
typedef struct arucohip_marker {
    int32_t id;
    float corners[8];
    float ssize;
    int32_t has_pose;
    int32_t pad_;
    double rvec[3];
    double tvec[3];
} arucohip_marker_t;

/* aruco::Board pose part (board.h:99-104); the member markers are returned in a caller array. */
typedef struct arucohip_board {
    int32_t n_markers;
    int32_t has_pose;
    double rvec[3];
    double tvec[3];
} arucohip_board_t;

/* Both pose solutions of one marker (arucohip_planar_poses): solution j is rvec[j] / tvec[j] with reprojection error rms[j]. 120 bytes. */
typedef struct arucohip_planar_poses {
    double rvec[2][3], tvec[2][3];
    double rms[2];                        /* pixels, rms[0] <= rms[1] */
    int32_t n_solutions;                  /* 0 or 2 */
    int32_t pad_;
} arucohip_planar_poses_t;

/* device-side limits of one handle */
typedef struct arucohip_limits {
    int32_t max_width, max_height;
    int32_t max_batch;             /* frames per arucohip_detect_batch call */
    int32_t max_thres_planes;      /* 2*range+1 supported per frame */
    int32_t triggers_per_frame;    /* border-start candidates (average per frame) */
    int32_t contours_per_frame;    /* borders that pass the size filter */
    int32_t points_per_frame;      /* contour-point pool (average per frame) */
    int32_t candidates_per_frame;  /* quads per frame */
    int32_t markers_per_frame;     /* device-side marker slots per frame */
    int32_t long_walks_per_plane;  /* borders followed beyond the first 64 steps, per threshold plane and kind (outer /
                                      hole); each holds a checkpoint ring of max contour length / 16 words in HBM */
} arucohip_limits_t;

typedef struct arucohip_handle arucohip_handle;

int arucohip_version(void);
/* "src=<digest of the library's sources> flags=[<extra compiler flags of a variant build>]": which build is loaded. An experiment build
 * (tools/stage_cost.sh: -DARUCOHIP_STAGE_EXPERIMENT truncates the pipeline) says so here, and bench.py refuses to print a headline for it. */
const char* arucohip_build_info(void);
void arucohip_default_params(arucohip_params_t* p);
void arucohip_default_limits(arucohip_limits_t* l, int max_width, int max_height, int max_batch);

/* Create a detector on HIP device `device` able to take frames up to max_width x max_height, `max_batch` at a time.
 * params may be NULL (reference defaults). Geometry: a handle is at least 32 x 32 and at most 16383 x 16383 (14-bit coordinates in the
 * border checkpoints) with max_width * max_height <= 2^26 (raster keys); a frame is 1 x 1 up to the handle's size, the limits hold per
 * dimension (a frame may be smaller than the handle, not wider or taller). Anything outside is ARUCOHIP_E_INVALID; the reference has no
 * upper limits. */
int arucohip_create(const arucohip_params_t* params, int device, int max_width, int max_height, int max_batch,
                    arucohip_handle** out);
int arucohip_create_ex(const arucohip_params_t* params, int device, const arucohip_limits_t* limits, arucohip_handle** out);
void arucohip_destroy(arucohip_handle* h);
/* setters of MarkerDetector (markerdetector.h:129-245) collapse into one call; validates like setMinMaxSize /
 * setWarpSize (markerdetector.cpp:1031-1051). */
int arucohip_set_params(arucohip_handle* h, const arucohip_params_t* p);
int arucohip_get_params(const arucohip_handle* h, arucohip_params_t* p);
const char* arucohip_last_error_string(const arucohip_handle* h);

/* Run the handle's work on an existing HIP stream (hipStream_t passed as void*); NULL restores the handle's own. */
int arucohip_set_stream(arucohip_handle* h, void* hip_stream);
void* arucohip_get_stream(arucohip_handle* h);
int arucohip_synchronize(arucohip_handle* h);
/* Frames produced on ANOTHER stream: everything the handle enqueues from now on (the next arucohip_detect_batch with device frames, the
 * lane that takes the next arucohip_detect_batch_submit) first waits for `hip_event` (hipEvent_t passed as void*), which the producer
 * recorded on its stream behind the last write to the frames. This is the stream-ordered alternative to synchronising the producer. */
int arucohip_wait_event(arucohip_handle* h, void* hip_event);

/* MarkerDetector::detect (markerdetector.h:102-103) for one 8-bit gray frame in HOST memory.
 * K: 9 floats row-major or NULL (no pose); dist: ndist (0,4,5,8) floats or NULL; marker_size <= 0 -> no pose.
 * out/cap: caller array; *n_out = number of markers (sorted by id). */
int arucohip_detect(arucohip_handle* h, const uint8_t* gray, int width, int height, size_t row_stride, const float* K,
                    const float* dist, int ndist, float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap,
                    int* n_out);

/* Same for a batch of nframes equally sized frames (frame f at frames + f*frame_stride).
 * frames_on_device != 0: `frames` is a device pointer (frames already resident in HBM). The kernels read it on the
 *                       handle's stream: frames produced on another stream must be ordered before the call — record an event
 *                       behind the producer and pass it to arucohip_wait_event, run the handle on the producer's stream
 *                       (arucohip_set_stream), or synchronise the producer.
 * out_on_device   != 0: `out` (nframes*cap markers) and `n_out` (nframes int32) are device pointers, the call is
 *                       asynchronous on the handle's stream and reports only launch errors; otherwise host arrays and
 *                       the call returns when the results are there. */
int arucohip_detect_batch(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                          size_t frame_stride, int frames_on_device, const float* K, const float* dist, int ndist,
                          float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out,
                          int out_on_device);
/* SURVEY §8 row f1 — highly reliable markers: HighlyReliableMarkers::loadDictionary (src/highlyreliablemarkers.cpp:311-329).
 * codes[i] = marker i of the dictionary as n*n bits, bit y*n+x = cell (y, x) ('1' in aruco::Dictionary's bit strings),
 * n <= 8, count <= 4096; tau0 = Dictionary::tau0,
 * correction_rate = correctionDistanceRate (the reference's default is 1). With params.decoder_kind = ARUCOHIP_DECODER_HRM
 * the candidates are then decoded like HighlyReliableMarkers::detect (:332-383) — id = position in the dictionary — which
 * is what MarkerDetector::setMakerDetectorFunction(HighlyReliableMarkers::detect) selects in the reference; the warp size
 * should be a multiple of n + 2 (the reference's apps use (n + 2) * 8). count = 0 drops the dictionary.
 * For n >= 6 the reference's exact-match shortcut compares 32-bit ids built with `2 << bit` (:137-138), which overflow;
 * the nearest-entry search it falls back to — the intended behaviour, identical whenever the ids are unique — is what runs
 * here for every n. */
int arucohip_set_dictionary(arucohip_handle* h, int n, int count, const uint64_t* codes, int tau0, float correction_rate);

/* HighlyReliableMarkers::createDicitionary (src/highlyreliablemarkers.cpp:567-608, MarkerGenerator::generateMarker :58-116) as the
 * reference computes it right after srand(seed) with glibc's rand(): the same dict_size codes in the same order, in the layout of
 * arucohip_set_dictionary (bit y * n + x = cell (y, x)), so a result loads straight into a detector; *tau0 = the final tau (D.tau0);
 * *candidates_examined = index of the last candidate the sequential walk looked at, plus one (either may be NULL). Runs on the
 * device a window of candidates at a time (DESIGN.md "HRM dictionary and board generation"); at most (dict_size + tau0) * 100000
 * candidates. 3 <= n <= 8 (n = 2 divides by zero in the reference, n > 8 passes 64 bits) and 1 <= dict_size <= 4096, else
 * ARUCOHIP_E_INVALID; ARUCOHIP_E_INVALID naming it too when tau reaches 0 (the reference's CV_Error). Uses its own scratch: the
 * handle's single-frame graph stays valid. */
int arucohip_hrm_create_dictionary(arucohip_handle* h, int n, int dict_size, uint32_t seed, uint64_t* codes_out, int* tau0,
                                   int64_t* candidates_examined);
/* HighlyReliableMarkers::createBoardImage (:498-565): the image size of a grid_w x grid_h board of n x n markers: marker size
 * (n + 2) * 20, gap marker size / 5; chromatic adds a gap-wide margin and 3 channels (BGR). 3 <= n <= 8, grid 1..128 each. */
int arucohip_hrm_board_size(int n, int grid_w, int grid_h, int chromatic, int* width, int* height, int* channels);
/* The board image itself, made on the device: white background, getImg (:234-260) markers (white = bit 1, black border) of codes[0 ..
 * grid_w * grid_h - 1] row by row; chromatic: (250,134,4) with the black pixels (0,255,0), B G R. image: height rows of row_stride
 * bytes (host, or device with image_on_device). obj (may be NULL): grid_w * grid_h * 4 * 3 floats, BC.objPoints (pixels, centred,
 * y up). ids (may be NULL): BC.ids = getId() = sum of 2 << pos over the 1 bits; ARUCOHIP_E_UNSUPPORTED for n >= 6, where that shifts
 * past 32 bits (undefined in the reference). Note that HRM detection reports a marker's position in the dictionary, not getId(): to
 * find the board with arucohip_board_detect use ids[i] = i. count < grid_w * grid_h is ARUCOHIP_E_INVALID (the
 * reference reads past the dictionary). */
int arucohip_hrm_board_image(arucohip_handle* h, int n, int count, const uint64_t* codes, int grid_w, int grid_h, int chromatic, uint8_t* image,
                             size_t row_stride, int image_on_device, int32_t* ids, float* obj);

/* ---- The default 5x5 Hamming markers: images, boards and marker sets (DESIGN.md "Fiducial marker, board and marker-set generation").
 * The image calls paint on the device with scratch of their own: the handle's single-frame graph stays valid. Ids are 0..1023.
 *
 * FiducidalMarkers::createMarkerImage(id, size, false, locked) (src/arucofidmarkers.cpp:214-260) for n ids in one launch. An image is
 * side x side bytes, side = arucohip_fiducial_marker_side(size, locked): `size`, or size + 2 * int(float(size) * 0.25f) for the locked
 * form (white, a black square of that quarter in every corner, the marker in the middle). Cells are size / 7 wide (integer); the
 * remainder at the right and the bottom stays black. Image i starts at images + i * image_stride, its rows are row_stride bytes apart
 * (any value >= side, no alignment needed), in host memory or, with images_on_device, device memory. The "#id" watermark of
 * addWaterMark is not drawn. 7 <= size, side <= 16383, 1 <= n <= 1024, and for a host destination at most 2^30 bytes
 * of images (rows padded to 16) per call; else ARUCOHIP_E_INVALID, as for an id outside 0..1023 (CV_Assert in the reference). */
int arucohip_fiducial_marker_images(arucohip_handle* h, const int32_t* ids, int n, int size, int locked, uint8_t* images, size_t row_stride,
                                    size_t image_stride, int images_on_device);
/* The side of such an image; 0 when size < 7 or the side would pass 16383. Host arithmetic. */
int arucohip_fiducial_marker_side(int size, int locked);
/* FiducidalMarkers::getMarkerMat (:264-282): out25[5 * y + x] = cell (y, x) as 0 / 1. Host arithmetic. */
int arucohip_fiducial_marker_mat(int id, uint8_t* out25);
/* getListOfValidMarkersIds_random (:40-61): the first n entries that are not excluded of the list 0..1023 after
 * std::random_shuffle(list, list + 1024, cv::theRNG()) as libstdc++ runs it on cv::RNG (multiply with carry, 4164903690).
 * *rng_state is cv::theRNG().state, read and written, so consecutive calls continue one stream as consecutive createBoardImage*
 * calls do in the reference. n + nexcluded > 1024 or an excluded id outside 0..1023 is ARUCOHIP_E_INVALID. Host arithmetic. */
int arucohip_fiducial_shuffle_ids(uint64_t* rng_state, int n, const int32_t* excluded, int nexcluded, int32_t* ids_out);
/* The three board layouts (:290-430). type 0: createBoardImage (a panel of grid_w x grid_h markers, marker_distance apart);
 * 1: createBoardImage_ChessBoard (markers on every other cell, no distance: marker_distance is ignored); 2: createBoardImage_Frame
 * (the outermost ring of the panel's cells). *width / *height: the image; *ids_drawn: how many ids the reference takes from the
 * shuffle for it (w h, 3 (w h) / 4, 2 h 2 w); *markers: how many it places - it uses the first *markers of the drawn ids, in
 * row-major order of the cells. Any output may be NULL. grid 1..128 each, 7 <= marker_size, 0 <= marker_distance, image at most
 * 16383 x 16383, at most 1024 markers; a chessboard that places more markers than it draws (1 x 1, for one) trips a CV_Assert in the
 * reference (:362): all ARUCOHIP_E_INVALID. Host arithmetic. */
int arucohip_fiducial_board_size(int type, int grid_w, int grid_h, int marker_size, int marker_distance, int* width, int* height, int* ids_drawn,
                                 int* markers);
/* The board image, painted by one launch: white, marker k of the layout = createMarkerImage(ids[k], marker_size). image: *height rows
 * of row_stride bytes (>= *width, no alignment needed), host or device. obj (may be NULL): markers * 4 * 3 floats, TInfo.objPoints in
 * pixels (mInfoType PIX), y down; the panel is always centred on (width / 2, height / 2) (integer halves), the other two when
 * `centered`. nids below the layout's marker count is ARUCOHIP_E_INVALID. */
int arucohip_fiducial_board_image(arucohip_handle* h, int type, int grid_w, int grid_h, int marker_size, int marker_distance, int centered,
                                  const int32_t* ids, int nids, uint8_t* image, size_t row_stride, int image_on_device, float* obj);
/* utils/aruco_board_pix2meters.cpp:54-63: obj_out = obj * (marker_size_m / float(int(norm of the first marker's first side))), float
 * products. obj_out may be obj. A first side shorter than one pixel is ARUCOHIP_E_INVALID (the reference divides by zero). Host. */
int arucohip_board_pix_to_meters(const float* obj, int nmarkers, float marker_size_m, float* obj_out);
/* A board's corners moved by a rigid transform: obj_out = R(rvec) * p + tvec for each of the nmarkers * 4 corners (Rodrigues vector,
 * computed in double, rounded once to float; obj_out may be obj). No reference counterpart: a marker cube or a folded board is the
 * concatenation of placed arucohip_fiducial_board_image panels, and arucohip_board_detect poses any such rigid point set. Host
 * arithmetic, no handle. ARUCOHIP_E_INVALID on a null pointer or a negative count. */
int arucohip_board_place(const float* obj, int nmarkers, const double rvec[3], const double tvec[3], float* obj_out);
/* utils/aruco_selectoptimalmarkers.cpp:53-74, :128-131: dist[1024 * i + j] = the minimum over the four rotations of marker i of its
 * 25-cell Hamming distance to marker j (symmetric, zero diagonal). dist: 1024 * 1024 int32, host or device. */
int arucohip_fiducial_distances(arucohip_handle* h, int32_t* dist, int on_device);
/* The selection of that utility (:76-205) without its files: the first marker of the largest entropy (:76-95), then n_markers - 1
 * rounds that each take, among the markers of entropy >= min_entropy, the one whose smallest distance to the selected set is largest
 * (the lowest id on ties). ids_out (n_markers entries): the selection in ascending order; *n_selected its size; *min_dist the smallest
 * pairwise distance in it (INT_MAX for a single marker, as the reference prints). One launch, no host round trip per round. When a
 * round finds no marker at a distance above 1 the reference prints "COUDL NOT ADD ANY MARKER" and exits: ARUCOHIP_E_INVALID here,
 * with the markers found so far in ids_out / *n_selected. 1 <= n_markers <= 1024. */
int arucohip_fiducial_select(arucohip_handle* h, int n_markers, int min_entropy, int32_t* ids_out, int* n_selected, int* min_dist);

/* SURVEY §8b, plugin boundary — MarkerDetector::setMakerDetectorFunction (src/markerdetector.h:243-245) with a function of
 * the caller's own: typedef int (*MarkerdetectorFunc)(const cv::Mat& in, int& nRotations) (:78; contract :65-77: `in` is
 * the square canonical view of a candidate, the return value is the marker id or -1, nRotations the number of 90-degree
 * clockwise turns that bring the candidate to its canonical orientation). With params.decoder_kind =
 * ARUCOHIP_DECODER_USER the device still warps every candidate (MarkerDetector::warp, :353), the size x size patches come
 * back to the host, `fn` is called once per candidate in the reference's order (frame by frame, candidates in
 * detectRectangles order, *n_rotations preset to 0) and the rest of the pipeline — corner refinement, rotation of the
 * corners, sorting, duplicate and border filters, pose — continues on the device with the ids it returned. `patch` is a
 * scratch copy the function may overwrite (FiducidalMarkers::detect thresholds its input in place, arucofidmarkers.cpp:446).
 * A batch call then blocks until the decoders have run, also with out_on_device. fn = NULL removes the callback. */
typedef int (*arucohip_decoder_fn)(void* user, uint8_t* patch, int size, int* n_rotations);
int arucohip_set_decoder_callback(arucohip_handle* h, arucohip_decoder_fn fn, void* user);

/* SURVEY §8 row f3 — frames with three interleaved 8-bit channels in B,G,R order (what cv::imread / cv::VideoCapture
 * deliver; row_stride >= 3*width): MarkerDetector::detect converts them with cv::cvtColor(CV_BGR2GRAY)
 * (src/markerdetector.cpp:307-310); here the conversion runs on the device, bit-identical to OpenCV's 8-bit fixed-point
 * form (B*1868 + G*9617 + R*4899 + 8192) >> 14, and the gray frames then take the path of arucohip_detect_batch. */
int arucohip_detect_bgr(arucohip_handle* h, const uint8_t* bgr, int width, int height, size_t row_stride, const float* K,
                        const float* dist, int ndist, float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap,
                        int* n_out);
int arucohip_detect_batch_bgr(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                              size_t frame_stride, int frames_on_device, const float* K, const float* dist, int ndist,
                              float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out,
                              int out_on_device);
/* The conversion alone: one host BGR frame -> host gray frame (width*height bytes). */
int arucohip_bgr_to_gray(arucohip_handle* h, const uint8_t* bgr, int width, int height, size_t row_stride, uint8_t* gray);

/* Camera-native input (k_ingest.hip, capi_ingest.hip) - frames as cameras and decoders deliver them, converted on the device
 * (arucohip_convert_batch) to the 8-bit grey image the pipeline reads or to interleaved B,G,R for the colour consumers (arucohip_chromatic_*, arucohip_draw_*_batch,
 * arucohip_board_composite_batch, arucohip_warp_plane_batch, arucohip_undistort). All arithmetic is integer; >> of a negative value is
 * the floor shift; sat clamps to 0..255; gray_of(b, g, r) = (b*1868 + g*9617 + r*4899 + 8192) >> 14 as for arucohip_detect_bgr.
 * The YUV and Bayer definitions are this library's own and have no reference counterpart (the reference takes what cv::VideoCapture
 * hands it); nothing here claims bit-identity with OpenCV beyond what arucohip_detect_bgr claims.
 *   GRAY8                  1 byte per pixel. Grey: the byte; BGR: the byte three times.
 *   BGR8                   3 interleaved bytes, row_stride >= 3 * width. Grey: gray_of(b, g, r), the bytes of arucohip_bgr_to_gray.
 *   RGB8, BGRA8, RGBA8     3 / 4 interleaved bytes, row_stride >= 3 / 4 * width. Grey: gray_of(b, g, r). BGR: reordered, alpha ignored.
 *   GRAY16, bits = 8..16   little-endian uint16, row_stride >= 2 * width; neither rows nor the base need 2-byte alignment.
 *                          Grey: min(v >> (bits - 8), 255); BGR: that value three times. An MSB-aligned decoder plane (P010 / P016
 *                          luma) is bits = 16.
 *   YUYV (Y0 U Y1 V), UYVY (U Y0 V Y1)   2 bytes per pixel, width even, row_stride >= 2 * width. Grey: the Y byte. BGR: the formula
 *                          below, U and V shared by the pixel pair.
 *   NV12                   Y plane of `height` rows, then an interleaved U,V plane of height / 2 rows with the same row_stride that
 *                          starts chroma_offset bytes after the frame's start (0: row_stride * height). width and height even,
 *                          row_stride >= width, chroma_offset >= row_stride * height when given, frame_stride covers both planes.
 *                          Grey: the Y plane. BGR: the formula below with U, V of chroma sample (x / 2, y / 2).
 *   BAYER_RGGB, _BGGR, _GRBG, _GBRG      1 byte per pixel; the name is the top-left 2 x 2 block row by row. width, height >= 2, odd sizes
 *                          allowed. BGR: the bilinear demosaic below. Grey: gray_of of the demosaiced pixel.
 * YUV -> BGR, BT.601 video range in 20-bit fixed point (round of 1.164, 1.596, 0.813, 0.391, 2.018 times 2^20):
 *     y = max(0, Y - 16) * 1220542
 *     R = sat((y + 1673527 * (V - 128) + 524288) >> 20)
 *     G = sat((y - 852492 * (V - 128) - 409993 * (U - 128) + 524288) >> 20)
 *     B = sat((y + 2116026 * (U - 128) + 524288) >> 20)
 * Bayer -> BGR: neighbours outside the image by reflect-101 (-1 -> 1, N -> N - 2; it keeps the mosaic's colour parity). At a site of
 * colour C the channel C is the sample. At a red or blue site green = (N + S + E + W + 2) >> 2 and the opposite colour =
 * (NW + NE + SW + SE + 2) >> 2. At a green site the colour of its row's other sites = (W + E + 1) >> 1 and the colour of its column's
 * other sites = (N + S + 1) >> 1.
 * Out of scope: full-range (JPEG) YUV and BT.709, planar I420 / YV12, packed 10 / 12-bit (MIPI) rows, 16-bit Bayer, big-endian 16-bit
 * data, and the multi-GPU entry points (arucohip_mgpu_*: convert first, then shard the grey frames). */
typedef enum {
    ARUCOHIP_PIX_GRAY8 = 0, ARUCOHIP_PIX_BGR8, ARUCOHIP_PIX_RGB8, ARUCOHIP_PIX_BGRA8, ARUCOHIP_PIX_RGBA8,
    ARUCOHIP_PIX_GRAY16, ARUCOHIP_PIX_YUYV, ARUCOHIP_PIX_UYVY, ARUCOHIP_PIX_NV12,
    ARUCOHIP_PIX_BAYER_RGGB, ARUCOHIP_PIX_BAYER_BGGR, ARUCOHIP_PIX_BAYER_GRBG, ARUCOHIP_PIX_BAYER_GBRG
} arucohip_pixel_format;
typedef struct {
    int32_t format;          /* arucohip_pixel_format */
    int32_t bits;            /* GRAY16 only, else 0 */
    uint64_t chroma_offset;  /* NV12 only */
} arucohip_frame_format_t;
/* Host arithmetic. The bytes of a row the library reads (0: the format, its bits or the width are invalid), and the bytes of one frame
 * from its first to its last byte read, which frame_stride must cover when a call has more than one frame (0: invalid format, size,
 * row_stride or chroma_offset): row_stride * (height - 1) + the row's bytes; NV12: chroma_offset + row_stride * (height / 2 - 1) + width. */
size_t arucohip_frame_min_row_stride(const arucohip_frame_format_t* fmt, int width);
size_t arucohip_frame_min_stride(const arucohip_frame_format_t* fmt, int width, int height, size_t row_stride);
/* The conversion as a stage of its own, like arucohip_undistort / arucohip_pyr_down: dst_channels = 1 (grey) or 3 (B,G,R); dst rows are
 * dst_row_stride apart (>= width * dst_channels), frames dst_frame_stride apart (they cover dst_row_stride * (height - 1) + width * dst_channels bytes);
 * the bytes between are never written. src and dst in host or device memory; nframes and the size within the handle's limits. With
 * dst_on_device the call is asynchronous on the handle's stream, so arucohip_detect_batch(frames_on_device = 1) on the grey result, or a
 * colour consumer on the B,G,R result, can follow without a round trip; host src frames (pinned memory in particular, whose copies are
 * only queued when the call returns) must then stay untouched until the stream has passed the call (arucohip_synchronize, or whatever
 * completes the work queued behind it). Host frames are copied raw (arucohip_frame_min_row_stride bytes
 * per row; of NV12 with dst_channels = 1 the Y plane only) and converted on the device: a Bayer or NV12 frame crosses the link with a
 * third of the bytes of its BGR form. Everything is checked before anything runs: ARUCOHIP_E_INVALID for an unknown format, bits
 * outside 8..16, an odd width (YUYV / UYVY / NV12) or height (NV12), a Bayer frame below 2 x 2, strides below the minimum,
 * dst_channels other than 1 or 3 and a dst that overlaps src; the last batch's results stay as they were.
 * The detection calls carry no format: convert to grey (dst_channels = 1, dst_on_device = 1) and hand the result to
 * arucohip_detect_batch / arucohip_detect_batch_submit / arucohip_detect_batch_retry_overflowed with frames_on_device = 1. The Y plane
 * of an NV12 device frame needs no conversion: it is a grey frame with the same row_stride and frame_stride.
 * A host Bayer batch therefore takes a device buffer the caller owns and two calls:
 *     arucohip_frame_format_t f = {ARUCOHIP_PIX_BAYER_RGGB, 0, 0};              // d_grey: n * w * h bytes of device memory
 *     arucohip_convert_batch(h, bayer, &f, n, w, h, w, (size_t)w * h, 0, 1, d_grey, w, (size_t)w * h, 1);
 *     arucohip_detect_batch(h, d_grey, n, w, h, w, (size_t)w * h, 1, K, dist, ndist, size, 0, out, cap, n_out, 0);   // waits, fills out */
int arucohip_convert_batch(arucohip_handle* h, const void* src, const arucohip_frame_format_t* fmt, int nframes, int width, int height,
                           size_t row_stride, size_t frame_stride, int src_on_device, int dst_channels, uint8_t* dst,
                           size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device);

/* Frames out (k_egress.hip, capi_egress.hip) - the mirror of camera-native input: the 8-bit grey or interleaved B,G,R frames the library
 * paints, rectifies and composites, converted on the device to what the next stage takes: NV12 for a hardware video encoder, YUYV / UYVY
 * for a capture or loop-back sink, BGRA / RGBA for a display or a texture. src is src_channels = 1 (grey) or 3 (B,G,R) with rows
 * src_row_stride apart (>= width * src_channels) and frames src_frame_stride apart (they cover src_row_stride * (height - 1) +
 * width * src_channels bytes). fmt describes the destination with the record of the input side; its rows are dst_row_stride apart
 * (>= arucohip_frame_min_row_stride) and its frames dst_frame_stride apart (>= arucohip_frame_min_stride); NV12 puts its U,V plane
 * chroma_offset bytes after the frame's start (0: dst_row_stride * height). Destinations: GRAY8, BGR8, RGB8, BGRA8, RGBA8, YUYV, UYVY,
 * NV12. GRAY16 and the Bayer mosaics are input formats only and are refused.
 * All arithmetic is integer; >> is the floor shift; every sum below is non-negative and fits int32; gray_of is the one above. These
 * definitions are this library's own and have no reference counterpart. The colour transform is BT.601 video range in 20-bit fixed
 * point, the constants round(c * 2^20 / 255) of the standard matrix (65.481, 128.553, 24.966 / -37.797, -74.203, 112 /
 * 112, -93.786, -18.214); both chroma rows sum to exactly 0, the luma row to 900542:
 *     Y = (269262 R + 528618 G + 102662 B + (16 << 20) + (1 << 19)) >> 20
 *     U = (-155424 Sr - 305127 Sg + 460551 Sb + (128 << (20 + k)) + (1 << (19 + k))) >> (20 + k)
 *     V = ( 460551 Sr - 385654 Sg -  74897 Sb + (128 << (20 + k)) + (1 << (19 + k))) >> (20 + k)
 * Sr, Sg, Sb are the channel sums over the pixels that share the chroma sample: the two pixels of a YUYV / UYVY pair (k = 1), the
 * 2 x 2 block of NV12 (k = 2). This box filter matches the way the input side replicates chroma at (x / 2, y / 2). No clamp is
 * needed: Y stays in 16..235, U and V in 16..240.
 *   grey  -> Y of YUYV / UYVY / NV12     (900542 g + (16 << 20) + (1 << 19)) >> 20, the Y of (g, g, g); U = V = 128.
 *            with ARUCOHIP_EXPORT_GREY_IS_LUMA: Y = g, untouched, for a grey frame that was the Y plane of an NV12 or YUYV frame
 *            which the input side hands over as it lies; U = V = 128.
 *   grey  -> GRAY8                       a strided copy
 *   grey  -> BGR8, RGB8, BGRA8, RGBA8    the byte three times, alpha 255
 *   B,G,R -> GRAY8                       gray_of(b, g, r)
 *   B,G,R -> RGB8, BGRA8, RGBA8          reordered, alpha 255
 *   B,G,R -> BGR8                        a strided copy
 *   B,G,R -> YUYV / UYVY / NV12          the formulas above
 * The flag is ignored for a B,G,R source and for destinations other than the three YUV formats.
 * src and dst are each in host or device memory. With dst_on_device the call is asynchronous on the handle's stream, so it can follow
 * arucohip_draw_*_batch or arucohip_board_composite_batch on device frames with no synchronisation between:
 *     arucohip_board_composite_batch(h, d_bgr, ...);                              // frames in device memory, painted in place
 *     arucohip_frame_format_t f = {ARUCOHIP_PIX_NV12, 0, 0};                      // d_nv12: n * w * h * 3 / 2 bytes of device memory
 *     arucohip_export_batch(h, d_bgr, 3, n, w, h, 3 * w, (size_t)3 * w * h, 1, &f, 0, d_nv12, w, (size_t)w * h * 3 / 2, 1);
 *     arucohip_synchronize(h);                                                    // or an event: d_nv12 goes to the encoder
 * Host sources go up raw (width * src_channels bytes per row) and host destinations come down by rows; of NV12 only the bytes of both
 * planes move, not the gap before chroma_offset. The bytes between rows, between the planes and between frames are never written.
 * Everything is checked before anything runs: ARUCOHIP_E_INVALID for NULL pointers, an unknown or refused format, src_channels other
 * than 1 or 3, an odd width (YUYV / UYVY / NV12) or height (NV12), strides below the minimum, a frame_stride that does not cover a
 * frame, chroma_offset inside the Y plane, nframes or the size beyond the handle's limits, a dst that overlaps src and flag bits other
 * than the one defined; the last batch's results stay as they were.
 * Out of scope: planar I420 / YV12 and P010, full-range and BT.709 matrices, any resize, and the multi-GPU entry points. */
#define ARUCOHIP_EXPORT_GREY_IS_LUMA 1
int arucohip_export_batch(arucohip_handle* h, const uint8_t* src, int src_channels, int nframes, int width, int height,
                          size_t src_row_stride, size_t src_frame_stride, int src_on_device,
                          const arucohip_frame_format_t* fmt, int flags,
                          void* dst, size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device);
/* SURVEY §8 row f3 — lens undistortion of the frames on the device: cv::undistort(src, dst, CameraMatrix, Distorsion), which
 * the reference's GL apps run on every frame before detect() (utils/aruco_test_gl.cpp:237-240, utils/aruco_test_board_gl.cpp:
 * 265-268; detect is then called with an empty distortion vector). 8-bit frames with `channels` = 1 or 3 interleaved channels;
 * dst is tightly packed (nframes x height x width x channels), in host or device memory; with dst_on_device the call is
 * asynchronous on the handle's stream, so arucohip_detect_batch(frames_on_device = 1) can follow without a round trip. The
 * fixed-point map (OpenCV's CV_16SC2 form: bilinear, 5 fractional bits, constant 0 outside) is computed once per (size, K, dist)
 * and kept in the handle. */
int arucohip_undistort(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, size_t row_stride, size_t frame_stride,
                       int channels, int src_on_device, const float* K, const float* dist, int ndist, uint8_t* dst, int dst_on_device);
/* MarkerDetector::pyrDown(level) of ArUco 1.2 (this snapshot of the reference dropped it as a no-op, PortingManual.md): detect on a
 * reduced image. With level > 0 every detection call of the handle reduces the gray frame `level` times (cv::pyrDown: 5x5 Gaussian,
 * BORDER_REFLECT_101, half the size rounded up; BGR input reduces the converted gray image) and runs threshold, erosion, contours and
 * quads on the reduced image; min / max contour length are measured on the reduced size. Corners and contour points are then multiplied
 * by 2^level, and decoding (warp + Otsu), HARRIS / SUBPIX refinement, the border filter and the poses work on the full-resolution frame;
 * LINES fits its lines to the scaled contour. From then on every getter (arucohip_get_candidates, arucohip_debug_contour,
 * arucohip_debug_candidates) reports full-frame coordinates, while arucohip_get_thresholded returns the reduced image (the size of the
 * last level, tightly packed). 0 <= level <= 3 (ARUCOHIP_E_INVALID otherwise, the level stays as it was); nothing may be in flight
 * (arucohip_detect_batch_submit). Level 0, the default, is the path without the option, launch for launch. With a level above 0 a
 * one-frame call takes the eager path: the reduced path is not captured in the frame graph. The level is a property of the handle beside
 * arucohip_params_t (arucohip_get_params does not report it); a multi-GPU detector sets it per slot through arucohip_mgpu_handle. */
int arucohip_set_pyr_down(arucohip_handle* h, int level);
int arucohip_get_pyr_down(const arucohip_handle* h);
/* The reduction as a stage of its own: nframes 8-bit gray frames, in host or device memory, reduced `levels` (1..3) times; dst is tightly
 * packed (nframes x Ho x Wo of the last level, Wo = (W + 1) / 2 per level), in host or device memory; with dst_on_device the call is
 * asynchronous on the handle's stream, like arucohip_undistort. */
int arucohip_pyr_down(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, size_t row_stride, size_t frame_stride,
                      int src_on_device, int levels, uint8_t* dst, int dst_on_device);
/* After an asynchronous batch: synchronise and report device-side overflow / capacity conditions. */
int arucohip_batch_status(arucohip_handle* h);
/* Capacities of the device lists, from arucohip_limits_t (F = frames per worker: max_batch, or ceil(max_batch / ARUCOHIP_STREAMS)). triggers_per_frame,
 * contours_per_frame, points_per_frame, candidates_per_frame and markers_per_frame must be at least 1 (ARUCOHIP_E_INVALID otherwise),
 * candidates_per_frame at most 512, markers_per_frame at most 256. The bits are those of the batch status word. Per threshold plane:
 *   start candidates      max(triggers_per_frame, 8192) / 2 of each kind (outer, hole)                      bit 1  (triggers)
 *   waypoint records      triggers_per_frame, no minimum (segment pipeline: one small frame per call)        bit 1; a graph cut short may add bit 64
 *   long-walk rings       min(max(long_walks_per_plane, 64), 65536) of each kind; the walks of one generation share lists of that many
 *                         entries times the planes rounded up to 8, in up to 8 sublists by plane              bit 1
 *   border descriptors    contours_per_frame: borders of at most 960 points from slot 0 upwards, longer ones (the late list) from the last slot
 *                         downwards, in the room the first kind left                                          bit 2  (contours)
 *   points pool           points_per_frame words (fewer when planes * points_per_frame would pass 2^32 - 16): a border of n points takes n words,
 *                         on the walker pipeline ceil(n / 16) checkpoint words in front of them as well          bit 4  (points)
 * Per frame, all its planes together:
 *   quads                 min(2 * candidates_per_frame, 512): with several threshold planes a frame of more than 512 quads cannot be held by
 *                         any handle and is always reported                                                   bit 8  (quads)
 *   candidates            candidates_per_frame (after the near-duplicate removal)                            bit 16 (candidates)
 *   markers               markers_per_frame                                                                  bit 32 (markers)
 * Per batch:
 *   flat decode list      max(F * min(candidates_per_frame, 96), candidates_per_frame): 96 candidates per frame on the batch's average, and one
 *                         frame alone may always fill its own candidate list; the frames that do not fit are given up whole    bit 16
 * Device lists are finite (arucohip_limits_t), the reference's vectors are not (src/markerdetector.cpp:496-635). When a list overflows
 * the call returns ARUCOHIP_E_OVERFLOW, but only the frames it happened to are given up: their n_out is -1, every other frame of the batch
 * holds its complete result. arucohip_detect_batch_retry_overflowed takes the arguments of the batch call that returned the code (after it
 * has completed: arucohip_batch_status / _wait for device outputs) and runs the frames with n_out = -1 again, one at a time, on an internal
 * one-frame handle whose per-frame lists are 4x (16x, 64x) larger, patching out / n_out in place; *n_retried = frames redone. */
int arucohip_detect_batch_retry_overflowed(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                                           size_t frame_stride, int frames_on_device, const float* K, const float* dist, int ndist,
                                           float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out,
                                           int out_on_device, int* n_retried);
/* With the environment variable ARUCOHIP_STREAMS = 2..8 a large batch is processed as that many chunks of consecutive
 * frames on separate HIP streams (default 1) that fork from and join the handle's stream, so the caller sees one
 * stream-ordered call; host frames of chunk i+1 are copied while chunk i computes. Returns the number of chunks of the
 * last batch and, if not NULL, the frames per chunk — every kernel launch covers one chunk. No reference counterpart. */
int arucohip_batch_chunks(arucohip_handle* h, int* frames_per_chunk);

/* Batches in flight (no reference counterpart: MarkerDetector::detect is synchronous). The tail of a batch — border
 * following of the longest contours, decoding — is latency bound and leaves most of the chip idle, the head of the next
 * batch is a streaming kernel: with depth >= 2 a stream of batches overlaps them. arucohip_set_pipeline_depth creates
 * `depth` complete workers (own buffers, own stream; 0 removes them); arucohip_detect_batch_submit takes the arguments
 * of arucohip_detect_batch, enqueues the batch on worker ticket mod depth behind everything queued on the handle's stream so
 * far and returns at once; arucohip_detect_batch_wait(ticket) returns when that batch is complete (its status code: overflow /
 * capacity conditions as arucohip_detect_batch / arucohip_batch_status would report them), host outputs are filled then.
 * At most `depth` tickets can be outstanding (ARUCOHIP_E_CAPACITY otherwise); getters and arucohip_board_detect_batch
 * address the batch that finished last, a synchronous call's or the last ticket waited for. Input frames and output
 * arrays of a ticket must stay untouched until its wait returns. */
int arucohip_set_pipeline_depth(arucohip_handle* h, int depth);
int arucohip_detect_batch_submit(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                                 size_t frame_stride, int frames_on_device, const float* K, const float* dist, int ndist,
                                 float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out,
                                 int out_on_device, int* ticket);
int arucohip_detect_batch_wait(arucohip_handle* h, int ticket);

/* MarkerDetector::getThresholdedImage (markerdetector.h:183): thresholded image of frame `frame` of the last call
 * (the middle one when thres_param1_range > 0), copied to host `dst` (width*height bytes, tightly packed). The hot path keeps the image
 * as bit tiles plus its four border lines (what cv::findContours works on); this call expands the requested plane to the reference's
 * 0 / 255 bytes. ARUCOHIP_THRES_BYTES=1 (environment, read at handle creation) writes the bytes during detection instead. */
int arucohip_get_thresholded(arucohip_handle* h, int frame, uint8_t* dst);
/* MarkerDetector::getCandidates (markerdetector.h:266): quads that were rectangles but not markers. quads: cap*8 floats. */
int arucohip_get_candidates(arucohip_handle* h, int frame, float* quads, int cap, int* n);

/* Stage entry points the reference keeps public (markerdetector.h:255-280), on host buffers. */
int arucohip_threshold(arucohip_handle* h, int method, const uint8_t* gray, int width, int height, size_t row_stride,
                       double param1, double param2, uint8_t* dst);
int arucohip_detect_rectangles(arucohip_handle* h, const uint8_t* thres, int width, int height, size_t row_stride,
                               float* quads, int cap, int* n);
int arucohip_warp(arucohip_handle* h, const uint8_t* gray, int width, int height, size_t row_stride, const float quad[8],
                  int size, uint8_t* dst);

/* MarkerDetector::refineCandidateLines(MarkerCandidate&, camMatrix, distCoeff) (markerdetector.h:280, .cpp:931-997), the LINES
 * corner refinement as a stage of its own: contour_xy = the candidate's contour (MarkerCandidate::contour, markerdetector.h:60: npoints
 * cv::Point = int32 pairs x0,y0,x1,y1,... in the order cv::findContours produced them, reversed if detectRectangles swapped the corners),
 * corners = the candidate's four corners on input (they must be contour points: every corner is looked up in the contour after rounding
 * to int like Point(candidate[k]), the last match wins) and the four intersections of the sides' least-squares lines on output. With K
 * (9 floats) and dist (ndist > 0) the contour is undistorted before the fit and the corners are distorted again, as the reference does
 * when both matrices are non-empty. Coordinates are image pixels, 0 <= x, y <= 32767; npoints at most the handle's
 * points_per_frame. Uses the handle's candidate and point lists: results of the last batch are gone afterwards (like the other stage calls). */
int arucohip_refine_candidate_lines(arucohip_handle* h, const int32_t* contour_xy, int npoints, float corners[8], const float* K,
                                    const float* dist, int ndist);

/* Stage inspection for parity tests (results of the last detect/detect_batch/detect_rectangles call).
 * Contours that passed the size filter, in the reference's cv::findContours(RETR_LIST) relative order. */
int arucohip_debug_num_contours(arucohip_handle* h, int frame, int* n);
int arucohip_debug_contour(arucohip_handle* h, int frame, int index, int* is_hole, int* start_x, int* start_y, int16_t* xy,
                           int cap_points, int* n_points);
/* Border-start candidates of a frame after the run rule (walker mode only: a handle whose borders go through the waypoint segments returns
 * ARUCOHIP_E_INVALID): the transition pixels y << 16 | x of the outer (kind 0: the first pixel of a run of set pixels) or hole (kind 1: the clear
 * pixel right of a set one) list, the frame's threshold planes one after the other, in the order the device appended them (any). *n is the list's
 * length; ARUCOHIP_E_CAPACITY when it exceeds cap. */
int arucohip_debug_start_candidates(arucohip_handle* h, int frame, int kind, uint32_t* yx, int cap, int* n);
/* Candidates after detectRectangles in reference order: integer quad, decoded id (-1 none), nRotations. */
int arucohip_debug_candidates(arucohip_handle* h, int frame, float* quads0, int32_t* ids, int32_t* nrot, int cap, int* n);
/* Otsu threshold (cv::threshold THRESH_OTSU inside the decoders, arucofidmarkers.cpp:169 / highlyreliablemarkers.cpp:346) of every candidate's patch,
 * same order; -1 where the decode stage did not run for the candidate. */
int arucohip_debug_otsu(arucohip_handle* h, int frame, int32_t* thr, int cap, int* n);
/* Cell medians of every candidate's patch, same order: cells49[49 * i + 7 * cy + cx] = the 33rd-largest of the 64 pixels of cell (cy, cx) of candidate
 * i's 56x56 patch. The last batch must have decoded from them (built-in 5x5 decoder, warp size 56, three frames or more); ARUCOHIP_E_INVALID otherwise. */
int arucohip_debug_cells(arucohip_handle* h, int frame, uint8_t* cells49, int cap, int* n);

/* Test hooks of the threshold stage.
 * arucohip_debug_threshold_batch runs the threshold stage of a batch and nothing behind it: the geometry and argument checks of
 * arucohip_detect_batch, the handle's current parameters (method, block sizes, C, range), the same kernel choice as a batch of nframes
 * frames with this geometry and base address. want_bytes != 0 asks for the byte image at once, as the stage entry points and
 * ARUCOHIP_THRES_BYTES=1 do; 0 leaves the choice to the handle. The frames are thresholded as given, whatever pyramid level the handle has
 * (arucohip_set_pyr_down). The batch becomes the last one for the getters below and for arucohip_get_thresholded; the contour, candidate and
 * marker lists and the cell medians of an earlier batch no longer belong to it (arucohip_debug_cells answers ARUCOHIP_E_INVALID).
 * arucohip_debug_threshold_plan reports which kernels the last threshold launch ran (of a batch in chunks: the first chunk's), as
 * its launcher executed them: per plane five words - family (0 strip, 1 wide, 2 eo kernel), block radius R (0 with the FIXED method),
 * the strip kernel's P16 and FAST, the wide / eo kernel's rows per wave (16, 32, 128; 0 for a strip plane) - then the strips per row,
 * whether the byte image was left out, and whether the separate bitmap pass ran. cap counts int32 words: 5 * planes + 3 are needed
 * (ARUCOHIP_E_CAPACITY below that; *nplanes is set either way). ARUCOHIP_E_INVALID before any threshold launch and after CANNY.
 * arucohip_debug_threshold_plane reads plane t (0 .. 2 * thres_param1_range) of frame `frame` of the last batch; every output may be
 * null. bytes: width * height, as arucohip_get_thresholded returns the middle plane (expanded from tiles and border lines when the
 * batch left the byte image out). tiles: the contour image as the device keeps it, [tiles_y][tiles_x] words of 8 x 8 pixels, bit
 * (y & 7) * 8 + (x & 7), tiles_x = max(4, ceil(width / 8) + 1) and likewise tiles_y. tile_bits: the non-empty-tile bitmap,
 * [tiles_y][2 * ceil(width / 1024)] words: per 128-tile strip the even tiles' word, then the odd tiles'. */
int arucohip_debug_threshold_batch(arucohip_handle* h, const uint8_t* gray, int nframes, int width, int height, size_t row_stride,
                                   size_t frame_stride, int frames_on_device, int want_bytes);
int arucohip_debug_threshold_plan(arucohip_handle* h, int32_t* out, int cap, int* nplanes);
int arucohip_debug_threshold_plane(arucohip_handle* h, int frame, int t, uint8_t* bytes, uint64_t* tiles, uint64_t* tile_bits);

/* Device list fill levels of the last batch: [0] border-start candidates, [1] borders kept, [2] contour points,
 * [3] overflow bits, [4] long walks (waypoint records in segment mode), [5] 1 when the batch ran on the waypoint-segment pipeline, so that [4]
 * counts waypoint records, else 0. For sizing arucohip_limits_t. For tests: [6] the long walks that
 * reached the late generations (borders of more than 960 points), [7] how many of the workers that hold the batch own a side stream for
 * those generations (a pipeline lane, arucohip_set_pipeline_depth, owns none: its batch runs on one stream). */
int arucohip_debug_counters(arucohip_handle* h, uint32_t* out8);
/* Test hook: the counters of ONE threshold plane of the last batch (plane = frame * planes per frame + t), read as the kernels left them; nothing
 * is launched. The counters keep counting past the capacities, so a generous handle's values are the plane's demand on each list. out, at least 36
 * words: [0] outer and [1] hole start candidates, [2] borders kept, [3] pool words (points and the checkpoints in front of them), [5] the plane's own
 * overflow bits (the bits of the batch status word; a frame with a bit on any of its planes is given up), [6] borders of the late list, [32] outer and
 * [33] hole long walks (checkpoint rings asked for), [34] waypoint records (segment pipeline), [35] 1 when the handle follows borders by waypoint
 * segments. cap below 36: ARUCOHIP_E_CAPACITY; a plane outside the last batch: ARUCOHIP_E_INVALID. */
int arucohip_debug_plane_counters(arucohip_handle* h, int plane, uint32_t* out, int cap);

/* Test hook: the pixel-domain corner kernels on corners of the caller's. gray: one host frame with its row stride (kept on the device,
 * at most four times the handle's width); corners_xy: ncorners x,y pairs, refined in place. locked_wsize > 0 runs findCornerMaxima with that
 * window (at most 31) first; method ARUCOHIP_CORNER_SUBPIX (win 1..15) or _HARRIS (win unused) runs the refinement; _NONE with locked_wsize > 0
 * runs the pre-pass alone. ncorners is 1..4 * candidates_per_frame; every coordinate finite and within +-65534. Everything is checked before
 * anything runs (ARUCOHIP_E_INVALID / _E_UNSUPPORTED / _E_CAPACITY). Uses the handle's candidate list: results of the last batch are gone afterwards. */
int arucohip_debug_refine_pixels(arucohip_handle* h, const uint8_t* gray, int width, int height, size_t row_stride, float* corners_xy,
                                 int ncorners, int method, int win, int locked_wsize);

/* Test hook: the decode stage (inverse homography, warp + histogram, Otsu threshold, cell votes, id and rotation) on quads of the caller's.
 * gray: nframes host frames [nframes][height][row_stride] (the stride is kept on the device, at most four times the handle's width; nframes at most
 * the handle's max_batch); quads_xy: n quads of four integer corners x0,y0 .. x3,y3, as detectRectangles leaves them (any values an int16 holds,
 * outside the frame included); frame_of: the frame each quad is warped from. The handle's current parameters (warp_size, decoder_kind, dictionary)
 * and nframes choose the kernels exactly as a batch of nframes frames would: one or two frames store the patch, three or more with the built-in 5x5
 * decoder and warp_size 56 keep the cell medians instead. Outputs, each optional, in the order of the quads: iM [n][9] inverse homographies,
 * hist [n][256], thr [n] Otsu thresholds, cells49 [n][49] (written when *paths & 1: the cell medians were kept), patches [n][warp_size^2] (written
 * when *paths & 2: the patches were stored), ids / nrot [n] (id -1: not a marker). n is 1..the capacity of the flat decode list (the formula above
 * arucohip_detect_batch_retry_overflowed) and at most candidates_per_frame quads per frame: ARUCOHIP_E_CAPACITY beyond; a frame index outside the call: ARUCOHIP_E_INVALID; the
 * caller's decoder (ARUCOHIP_DECODER_USER): ARUCOHIP_E_UNSUPPORTED. Everything is checked before anything runs. Uses the handle's candidate
 * lists: results of the last batch are gone afterwards. */
int arucohip_debug_decode_quads(arucohip_handle* h, const uint8_t* gray, int nframes, int width, int height, size_t row_stride,
                                const int16_t* quads_xy, const int32_t* frame_of, int n, double* iM, uint16_t* hist, int32_t* thr, uint8_t* cells49,
                                uint8_t* patches, int32_t* ids, int32_t* nrot, int32_t* paths);

/* Test hook: the marker-list tail of a batch (sort by id, same-id dedupe by perimeter, border filter, capacities and statuses, then the per-marker
 * poses when K is given and marker_size > 0) on decoded candidates of the caller's. nframes frames of width x height (no pixels are read; nframes at
 * most the handle's max_batch); n >= 0 candidates: ids [n] (-1: not a marker), corners [n][8] (every coordinate finite and within +-65534),
 * frame_of [n] the frame of each; they become their frames' candidates in the order given, at most candidates_per_frame in a frame
 * (ARUCOHIP_E_CAPACITY beyond). plane_status (optional): [nframes][planes] status words stored as the threshold planes' own, planes =
 * 2 * thres_param1_range + 1 of the handle's parameters; a frame with a non-zero word is given up (count -1), and the batch's status bits hold every word's bits, as when a kernel reports an overflow. The handle's border_dist gives the border
 * rectangle as in a detection. out_dev [nframes][out_cap] / n_out_dev [nframes] (optional, both or neither): DEVICE arrays the list kernel writes
 * through to, as it does for a batch whose results stay on the device. Outputs, each optional, on the host: rows [nframes][markers_per_frame] the raw
 * marker rows, filled with the byte 0xA5 before the kernels ran; nmarkers [nframes] the true counts (-1: given up); *status the batch's status
 * bits (32: a frame kept more than markers_per_frame markers); *nmark the length of the flat marker list and marker_list [nframes * markers_per_frame]
 * its entries frame << 16 | slot (0xA5 bytes beyond *nmark); hdr [2] the two words behind the rows, which a one-frame call sets to the count and the
 * status bits. Everything is checked before anything runs. Unlike the other hooks it leaves the frames as the handle's last batch: the batch
 * consumers (arucohip_gl_modelview_batch, arucohip_board_detect_batch, arucohip_planar_poses_batch, ...) then work on these lists. */
int arucohip_debug_marker_tail(arucohip_handle* h, int nframes, int width, int height, const int32_t* ids, const float* corners,
                               const int32_t* frame_of, int n, const uint32_t* plane_status, const float* K, const float* dist, int ndist,
                               float marker_size, int y_perp, arucohip_marker_t* out_dev, int out_cap, int32_t* n_out_dev, arucohip_marker_t* rows,
                               int32_t* nmarkers, uint32_t* status, uint32_t* nmark, uint32_t* marker_list, int32_t* hdr);

/* glibc's rand() outputs [offset, offset + count) after srand(seed), as the device makes them for arucohip_hrm_create_dictionary
 * (jump-ahead of the stream's state). count <= 2^24, offset + count < 2^48. */
int arucohip_debug_hrm_stream(arucohip_handle* h, uint32_t seed, uint64_t offset, int count, uint32_t* out);
/* The last arucohip_hrm_create_dictionary: [0] windows, [1] host synchronisations, [2] acceptances, [3] tau decrements. */
int arucohip_debug_hrm_counters(arucohip_handle* h, int32_t out[4]);

/* BoardDetector::detect (boarddetector.h:103-108). markers: output of arucohip_detect; ids/obj: BoardConfiguration
 * (board.h:56-69) as nboard ids and nboard*4*3 floats; returns likelihood in *prob (found / total).
 * out_markers (cap n) receives the board's member markers (Board : vector<Marker>). Up to 1168 correspondences (292 member
 * markers) are solved; more give ARUCOHIP_E_CAPACITY.
 * The object points may be any rigid set (a marker cube, markers on two walls, a planar board written in world coordinates): the pose
 * starts as cv::solvePnP(ITERATIVE) starts it. With n points M (scaled to metres) and Mc their mean:
 *   - every z == 0: the planar start (homography), as before;
 *   - else the eigenvalues w0 >= w1 >= w2 of sum (M - Mc)(M - Mc)^T decide. w2 / w1 < 1e-3: planar in the frame of the eigenvectors;
 *     the homography is taken there and its pose composed with that frame. Otherwise the direct linear transform of the undistorted
 *     points (n >= 6; fewer give has_pose = 0): the eigenvector of the smallest eigenvalue of the 12 x 12 normal matrix as [RR | tt],
 *     R the nearest rotation to RR, t = tt sqrt(3) / |RR|_F;
 *   - Levenberg-Marquardt on the original points from that start. A start that is not finite gives has_pose = 0, without an error.
 * The same holds for arucohip_board_detect_batch, arucohip_board_recover_batch and the shim's BoardDetector::detect. No reasoning about
 * self-occlusion: a face turned away from the camera is simply not detected. Still planar-only: the per-marker pose, arucohip_planar_poses,
 * calibration (views out of a plane give ARUCOHIP_E_UNSUPPORTED), the ChromaticMask board rectangle and ChArUco boards. */
int arucohip_board_detect(arucohip_handle* h, const arucohip_marker_t* markers, int n, const int32_t* ids, const float* obj,
                          int nboard, int info_type, const float* K, const float* dist, int ndist, float marker_size,
                          float repj_err_thres, int y_perpendicular, arucohip_marker_t* out_markers, arucohip_board_t* out,
                          float* prob);

/* BoardDetector::detect for every frame of the LAST arucohip_detect_batch call, on its device-resident markers (one
 * wavefront per frame, wave-parallel solvePnP over all board corners). out / prob: host arrays of nframes entries. The
 * board's member markers are the detected markers whose id is in `ids`, in the same order. */
int arucohip_board_detect_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                const float* K, const float* dist, int ndist, float marker_size, float repj_err_thres,
                                int y_perpendicular, arucohip_board_t* out, float* prob);

/* Board marker recovery. A marker of a board is lost when one of its cells reads wrong (a highlight, a fingertip, motion blur): the
 * decoder accepts only Hamming distance 0 with a clean border. Its quad is still among the frame's rejected candidates, and the board's
 * other markers say where it must be and what it must show. No counterpart in the reference (OpenCV's aruco module has
 * refineDetectedMarkers). */
typedef struct arucohip_recover {
    float   max_corner_dist;  /* pixels: largest distance between a candidate corner and the projected corner it is matched to.
                                 Default 10 (OpenCV's minRepDistance; taken over, not measured here) */
    int32_t max_cell_errors;  /* 0..49: cells of the 7 x 7 grid (24 border + 25 code) that may differ from the expected marker. Default 3 */
    int32_t min_markers;      /* board members a frame must already hold (>= 1). Default 2 */
    int32_t pose_markers;     /* != 0: recovered markers get ssize and their own pose from this call's camera, as
                                 arucohip_calculate_extrinsics would give; 0: has_pose = 0, ssize = -1 */
} arucohip_recover_t;
void arucohip_default_recover(arucohip_recover_t* o);

/* Works on the first nframes frames of the LAST batch (a synchronous call, a waited ticket or a one-frame arucohip_detect; every chunk
 * worker), entirely on the device, frame by frame:
 *  1. the board pose from the frame's markers whose id is in `ids`, as arucohip_board_detect_batch solves it, before rotateXAxis. A frame
 *     without a pose, with fewer than min_markers members or given up by the batch (n = -1) is left untouched;
 *  2. for every board entry the frame lacks, in board order: its four corners are projected, and over the rejected candidates no earlier
 *     entry took and their four cyclic rotations the smallest "largest corner distance" to the integer quad is found (ties: lower
 *     candidate, then lower rotation). The entry stays missing unless that is < max_corner_dist;
 *  3. the candidate's 49 cell votes (the decoder's) are compared with the expected marker in the candidate's orientation; more than
 *     max_cell_errors differing cells leave the entry missing and the candidate free;
 *  4. the candidate gets id and rotation, its corners are refined as detection refines them with this call's camera (LINES or NONE) and
 *     turned to canonical order; a marker with a corner outside the border rectangle (border_dist) is not adopted;
 *  5. the adopted markers enter the frame's marker list at their place in id order (pose_markers: with their own pose). A full list
 *     (markers_per_frame) stops the frame's recovery: the call completes and returns ARUCOHIP_E_CAPACITY;
 *  6. the board is solved again over all members: boards[f] / prob[f] (host, may be NULL), rotated with y_perpendicular. The poses stay
 *     on the device as after arucohip_board_detect_batch (arucohip_chromatic_classify_batch may follow).
 * Every later reader of the last batch sees the recovered markers; a second call recovers nothing. out / n_out (both NULL, or both
 * given) receive each frame's whole marker list as arucohip_detect_batch lays it out (cap per frame; n_out[f] = -1 stays -1; a frame
 * with more than cap markers gives its count and ARUCOHIP_E_CAPACITY): host arrays, or device arrays with out_on_device. With
 * out_on_device and recovered, boards and prob all NULL the call is asynchronous on the handle's stream and reports no capacity
 * condition. recovered (host, nframes, may be NULL): markers recovered per frame.
 * Supported: the built-in 5 x 5 decoder, corner methods LINES and NONE, any threshold range, any pyrDown level.
 * ARUCOHIP_E_UNSUPPORTED: HARRIS / SUBPIX (the handle does not hold the frames), locked corners, the HRM and USER decoders.
 * ARUCOHIP_E_INVALID: no K, marker_size <= 0 on a PIX board, max_corner_dist <= 0, max_cell_errors outside 0..49, min_markers < 1,
 * nframes beyond the last batch. ARUCOHIP_E_BOARD_CONFIG: an empty board. ARUCOHIP_E_CAPACITY: a board of more than 682 markers. */
int arucohip_board_recover_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                 const float* K, const float* dist, int ndist, float marker_size, float repj_err_thres,
                                 int y_perpendicular, const arucohip_recover_t* opt, arucohip_marker_t* out, int cap, int32_t* n_out,
                                 int out_on_device, int32_t* recovered, arucohip_board_t* boards, float* prob);

/* cv::calibrateCamera for planar targets (pinhole model, dist = k1 k2 p1 p2 k3), solved on the device in double precision: start
 * values as OpenCV's (homography per view, focal lengths from the vanishing points, principal point at the image centre, distortion
 * 0, planar solvePnP per view), then Levenberg-Marquardt over the intrinsics and every view's pose with the poses eliminated
 * per view (Schur complement); 30 iterations or a relative step below DBL_EPSILON. Views are reduced in view order: the result
 * is bit-reproducible. flags: the values of cv::CALIB_*. */
#define ARUCOHIP_CALIB_USE_INTRINSIC_GUESS 1   /* start from K and dist (else K only gives the FIX_ASPECT_RATIO ratio) */
#define ARUCOHIP_CALIB_FIX_ASPECT_RATIO 2      /* fx / fy stays at the ratio of the given K (1 when K holds no focal lengths) */
#define ARUCOHIP_CALIB_FIX_PRINCIPAL_POINT 4
#define ARUCOHIP_CALIB_ZERO_TANGENT_DIST 8     /* p1 = p2 = 0 */
#define ARUCOHIP_CALIB_FIX_FOCAL_LENGTH 16
#define ARUCOHIP_CALIB_FIX_K1 32
#define ARUCOHIP_CALIB_FIX_K2 64
#define ARUCOHIP_CALIB_FIX_K3 128
#define ARUCOHIP_CALIB_MAX_VIEW_POINTS 512     /* points of one view */
/* obj: 3 floats per point, img: 2 floats per point, view after view (npoints[v] points each); on_device: obj, img and npoints are
 * device pointers. Every view's obj must have one constant z (ARUCOHIP_E_UNSUPPORTED otherwise). K (row-major 3x3) and dist are
 * in/out; rvecs / tvecs (3 doubles per view), per_view_rms (1 per view) may be NULL; *rms = sqrt(sum |r|^2 / sum npoints). */
int arucohip_calibrate_camera(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device,
                              int width, int height, int flags, double K[9], double dist[5], double* rvecs, double* tvecs,
                              double* per_view_rms, double* rms);
/* The same on the board detections of the LAST arucohip_detect_batch call, where they are (device-resident, every chunk): a frame
 * is a view when it holds >= min_markers markers of the board (ids / obj / info_type / marker_size as arucohip_board_detect_batch;
 * PIX boards are scaled to metres when marker_size > 0). used[f] (nframes entries, may be NULL) = 1 for the frames taken; rvecs /
 * tvecs (may be NULL) hold 3 doubles per used frame, in frame order. ARUCOHIP_E_INVALID when no frame qualifies. */
int arucohip_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard, int info_type,
                                   float marker_size, int min_markers, int width, int height, int flags, double K[9], double dist[5],
                                   int32_t* used, double* rvecs, double* tvecs, double* rms);
/* Test hook: the start values of a calibration and nothing after them. Views, size and flags as arucohip_calibrate_camera (model 0) or as
 * arucohip_fisheye_calibrate (model 1: K and the four coefficients dist[0..3] are its model, flags its ARUCOHIP_FISHEYE_*); K and dist are
 * read only. The views are staged and the start kernels run as in those calls, then: intr[9] the start intrinsics (fx fy cx cy and the
 * model's coefficients, a fisheye's ninth entry 0), poses[6 per view] the start rvec, tvec, *cost the sum of squared residuals at that
 * start, *err the start kernels' condition bits (0: fine, 1: degenerate views, 2: a view is not planar). The condition is reported, not
 * turned into an error: the call answers ARUCOHIP_OK, and with *err != 0 the other outputs are not meaningful. */
int arucohip_debug_calib_start(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device,
                               int width, int height, int flags, int model, const double K[9], const double* dist, double intr[9],
                               double* poses, double* cost, int32_t* err);

/* Marker mapping: the 3-D layout of a rigid marker set from frames that show several of its markers. This is what produces the
 * object points of a board that is not planar (a marker cube, markers taped around a room) for arucohip_board_detect* above, whose
 * comment lists what stays planar-only. No counterpart in this snapshot of the reference (its later versions ship a marker mapper).
 * Given a camera (K, dist), the marker side in metres and nboard ids, the call finds the rigid placement of every listed marker in
 * the frame of the FIRST listed one (the reference marker: identity, not a variable) and the board pose of every used frame, minimising
 * the squared pixel residuals of all four corners of all observations through the full camera model: corner k of marker m in frame
 * f projects R_f (R_m c_k + t_m) + t_f, c_k = Marker::getObjectPoints of marker_size. Intrinsics are fixed; FP64 on the device.
 * Start values: both planar solutions of every observation without refinement (arucohip_planar_poses), solution 0 with confidence
 * q = rms[1] / rms[0]; per marker pair the relative transform from the frame with the largest min(q_a, q_b) (ties: the lower frame); a
 * spanning tree from the reference marker that always adds the marker whose best edge into the mapped set scores highest (ties: the
 * lower board index); every frame's pose from its highest-q mapped marker. Then Levenberg-Marquardt with the frames' poses
 * eliminated per frame (Schur complement), CvLevMarq's rule as arucohip_calibrate_camera: at most 30 accepted steps or a relative
 * step below DBL_EPSILON. Frames are reduced in frame order: the result is bit-reproducible.
 * Which observations count: an id that is not listed is ignored; a repeated id within a frame keeps the first; a frame that shows
 * more than ARUCOHIP_MAP_MAX_FRAME_MARKERS listed markers keeps those with the largest quad perimeter, in detection order; an
 * observation without planar solutions (a degenerate quad) is dropped; a frame with fewer than max(min_markers, 2) listed markers is
 * not used. A listed marker that is not connected to the reference marker through used frames gets mapped = 0 and zeros in its
 * outputs (not an error), and a frame that shows only such markers is not used.
 * Outputs: obj (nboard * 4 * 3 floats, metres: the `obj` of arucohip_board_detect* with ARUCOHIP_BOARD_METERS), marker_rvec /
 * marker_tvec (3 doubles per marker), mapped (nboard); optional (may be NULL): used (nframes), frame_rvec / frame_tvec (3 doubles per
 * frame, zeros for a frame that is not used), marker_rms (nboard, pixels, root mean square over a marker's corners), rms
 * (sqrt(sum |r|^2 / corners)), iterations (accepted steps).
 * ARUCOHIP_E_INVALID: no K, ndist not 0, 4 or 5, marker_size <= 0, nboard < 2, nframes < 1 (or beyond the last batch), a NULL
 * required output, the reference marker in no used frame, fewer than two markers mapped. ARUCOHIP_E_CAPACITY: nboard >
 * ARUCOHIP_MAP_MAX_MARKERS. The call returns when the results are complete; it leaves the single-frame graph and the last batch's
 * results as they are. */
#define ARUCOHIP_MAP_MAX_MARKERS 64         /* listed markers: the reduced system is at most 378 x 378 */
#define ARUCOHIP_MAP_MAX_FRAME_MARKERS 16   /* listed markers used per frame */
/* Observations as three parallel arrays of nobs entries (frame index in [0, nframes), id, 8 floats x0 y0 .. x3 y3), in any order of
 * frames; the order within a frame is the detection order. on_device: the three arrays are device pointers. min_markers is 2. */
int arucohip_board_map(arucohip_handle* h, const int32_t* obs_frame, const int32_t* obs_id, const float* obs_corners, int nobs,
                       int on_device, int nframes, const int32_t* ids, int nboard, const float* K, const float* dist, int ndist,
                       float marker_size, float* obj, double* marker_rvec, double* marker_tvec, int32_t* mapped, int32_t* used,
                       double* frame_rvec, double* frame_tvec, double* marker_rms, double* rms, int32_t* iterations);
/* The same on the markers of the first nframes frames of the LAST arucohip_detect_batch call, where they are (device-resident, every
 * chunk and worker); no frame or marker leaves the device before the solve. */
int arucohip_board_map_batch(arucohip_handle* h, int nframes, const int32_t* ids, int nboard, const float* K, const float* dist,
                             int ndist, float marker_size, int min_markers, float* obj, double* marker_rvec, double* marker_tvec,
                             int32_t* mapped, int32_t* used, double* frame_rvec, double* frame_tvec, double* marker_rms, double* rms,
                             int32_t* iterations);

/* Camera rigs: several cameras on one frame, exposed together. Two questions that no single-camera call answers: where the cameras stand
 * relative to each other (arucohip_rig_calibrate*, what cv::stereoCalibrate answers for two cameras with fixed intrinsics), and where a
 * board is, using every camera that sees part of it at this instant (arucohip_rig_pose*). No counterpart in this snapshot of the
 * reference.
 * A rig is ncams cameras, 2 .. ARUCOHIP_RIG_MAX_CAMERAS. Camera c has fixed intrinsics (K, dist with ndist 0, 4 or 5) and a rigid
 * transform rig -> camera, X_c = R_c X_rig + t_c. Camera 0 is the rig frame: its transform is the identity and never a variable. An
 * instant t is one simultaneous exposure of all cameras, a view the pair (t, c) with index v = t * ncams + c: the camera varies
 * fastest, so an interleaved multi-camera stream is a batch as it stands. The board is ids / obj / nboard / info_type / marker_size
 * as arucohip_board_detect_batch takes it (planar or not, PIX boards scaled to metres by marker_size), at most 128 markers: a view
 * holds at most 512 points. The cost, everywhere: over every counted view and every corner k of every member marker m in it, the
 * squared pixel residual of project(K_c, dist_c, R_c (R_t X_mk + t_t) + t_c) - x, with (R_t, t_t) the board's pose in the rig frame at
 * instant t. FP64 on the device.
 * Which observations count:
 *  - an id that is not on the board is ignored; a repeated id within a view keeps the first, in detection order;
 *  - a view counts when it holds >= min_markers (>= 1) member markers and its single-camera start pose exists: the pose of
 *    arucohip_board_detect_batch without the reprojection filter;
 *  - calibration: an instant is eligible when at least 2 of its views count. The score of a camera pair (a, b) is the largest
 *    min(n_a, n_b) of member-marker counts over the eligible instants where both views count (ties: the lower instant). A spanning tree
 *    grows from camera 0 and always adds the camera whose best edge into the reached set scores highest (ties: the lower camera; among a
 *    camera's equal edges the lower reached camera). A camera b reached through edge (a, b) at instant t starts at T_b = V_tb V_ta^-1 T_a,
 *    V the view's single-camera pose. A camera the tree does not reach gets calibrated = 0 and zeros (not an error); its views are not
 *    used. An instant is used when at least 2 of its counted views belong to calibrated cameras; it starts at T_c^-1 V_tc from the
 *    counted, calibrated view with the most member markers (ties: the lower camera);
 *  - rig pose: the same view rule; only cameras passed with calibrated != 0 take part (camera 0's transform is the identity whatever
 *    its rvec / tvec hold); an instant has a pose when at least one such view counts, with the same start;
 *  - views and instants that do not count or are not used change no output bit.
 * Calibration is Levenberg-Marquardt over the cameras' transforms with every used instant's pose eliminated per instant (Schur
 * complement; the reduced system is 6 (ncams - 1) square), CvLevMarq's rule as arucohip_calibrate_camera and arucohip_board_map: at most
 * 30 accepted steps or a relative step below DBL_EPSILON. All sums run in a fixed order (points within a view, views in camera order,
 * instants in instant order, no floating-point atomics): two calls, or host and device input, give the same bits. The rig pose runs
 * the same rule on the 6 pose unknowns of every instant, all instants in one launch.
 * ARUCOHIP_E_INVALID: ncams < 2, ninstants < 1 (or beyond the last batch), ndist not 0, 4 or 5, a NULL required pointer (cams, ids,
 * obj; out of the pose calls), a PIX board without marker_size, min_markers < 1, nframes no multiple of ncams; calibrate: no eligible
 * instant shows camera 0, or no camera besides camera 0 is reached; pose: no camera has calibrated != 0. ARUCOHIP_E_CAPACITY: ncams >
 * ARUCOHIP_RIG_MAX_CAMERAS, nboard > 128. A call that fails writes none of its outputs. The calls return when their outputs are
 * complete and leave the single-frame graph and the last batch's results as they are. rotateXAxis is not offered here. */
#define ARUCOHIP_RIG_MAX_CAMERAS 16
typedef struct arucohip_rig_camera {
    float K[9];           /* in: fixed intrinsics, row-major 3x3 */
    float dist[5];        /* in: k1 k2 p1 p2 k3, the first ndist are read */
    int32_t ndist;        /* in: 0, 4 or 5 */
    int32_t calibrated;   /* out of calibrate, in of pose */
    double rvec[3], tvec[3];   /* rig -> camera, out of calibrate, in of pose; camera 0: zeros */
} arucohip_rig_camera_t;
/* Observations as three parallel arrays of nobs entries (view index in [0, ninstants * ncams), id, 8 floats x0 y0 .. x3 y3), in any order
 * of views; the order within a view is the detection order. on_device: the three arrays are device pointers. cams: ncams entries,
 * in-out. Optional outputs (may be NULL): used (ninstants), board_rvec / board_tvec (3 doubles per instant: the board in the rig frame,
 * zeros for an instant that is not used), camera_rms (ncams, pixels, root mean square over the points of a camera's views), rms
 * (sqrt(sum |r|^2 / points)), iterations (accepted steps). */
int arucohip_rig_calibrate(arucohip_handle* h, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs,
                           int on_device, int ninstants, arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj,
                           int nboard, int info_type, float marker_size, int min_markers, int32_t* used, double* board_rvec,
                           double* board_tvec, double* camera_rms, double* rms, int32_t* iterations);
/* The same on the markers of the first nframes frames of the LAST arucohip_detect_batch call, where they are (device-resident, every
 * chunk and worker): frame f is view f, nframes / ncams instants. */
int arucohip_rig_calibrate_batch(arucohip_handle* h, int nframes, arucohip_rig_camera_t* cams, int ncams, const int32_t* ids,
                                 const float* obj, int nboard, int info_type, float marker_size, int min_markers, int32_t* used,
                                 double* board_rvec, double* board_tvec, double* camera_rms, double* rms, int32_t* iterations);
/* The board's pose in the rig frame at every instant: out[t] (ninstants entries; has_pose = 0 and zeros for an instant no calibrated
 * camera's view counts in; n_markers = the member markers summed over the views used), views_used[t] (may be NULL). */
int arucohip_rig_pose(arucohip_handle* h, const int32_t* obs_view, const int32_t* obs_id, const float* obs_corners, int nobs,
                      int on_device, int ninstants, const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids, const float* obj,
                      int nboard, int info_type, float marker_size, int min_markers, arucohip_board_t* out, int32_t* views_used);
int arucohip_rig_pose_batch(arucohip_handle* h, int nframes, const arucohip_rig_camera_t* cams, int ncams, const int32_t* ids,
                            const float* obj, int nboard, int info_type, float marker_size, int min_markers, arucohip_board_t* out,
                            int32_t* views_used);

/* Fisheye lenses: the equidistant model as cv::fisheye writes it, FP64 on the device. No counterpart in the reference. For a
 * camera-frame point (X, Y, Z): r = hypot(X, Y), theta = atan2(r, Z), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 +
 * k4 theta^8), pixel = (fx X theta_d / r + cx, fy Y theta_d / r + cy), the principal point when r = 0. Skew (K[1]) must be 0.
 * Pixel to ray: x = (u - cx) / fx, y = (v - cy) / fy, theta_d = hypot(x, y); 10 Newton steps on theta P(theta) - theta_d from
 * theta = theta_d; the ideal normalised point is (x, y) tan(theta) / theta_d, and (x, y) itself when theta_d = 0. A pixel is VALID
 * when the residual after the last step is at most 1e-12 max(theta_d, 1), the derivative stayed positive during the iteration and
 * theta <= max_angle. max_angle is in radians, 0 < max_angle < pi / 2 (ARUCOHIP_E_INVALID at or above pi / 2); a value <= 0 selects
 * 1.4. The residual bound is loose on purpose: it only catches coefficients for which theta_d(theta) is not monotone up to the pixel.
 * The pinhole entry points know nothing of this model. Instead the detected corners, or the frames, are mapped once to the pixels of
 * an ideal pinhole camera Knew (row-major 3 x 3 floats, NULL: the model's K), and every solver of this header (marker and planar
 * poses, board poses planar or 3-D, mapping, rig calibration and rig pose) then runs unchanged with K = Knew and ndist = 0.
 * Not provided: skew, a fisheye model inside arucohip_rig_camera_t. */
typedef struct arucohip_fisheye {
    double K[9]; /* row-major */
    double D[4]; /* k1..k4 */
} arucohip_fisheye_t;
/* n pixel pairs (src, dst: 2 floats per point; host memory, or device memory with on_device: then the call is asynchronous on the
 * handle's stream) between fisheye pixels and ideal pixels under Knew. One lane per point; the result is rounded once from double to
 * float. undistort: valid[i] = 1 or 0 (n bytes, where src and dst are), and an invalid point is written as (0, 0). distort: the
 * forward model on the ray Knew^-1 (u, v, 1), every point. */
int arucohip_fisheye_undistort_points(arucohip_handle* h, const arucohip_fisheye_t* model, const float* Knew, float max_angle,
                                      const float* src, int n, int on_device, float* dst, uint8_t* valid);
int arucohip_fisheye_distort_points(arucohip_handle* h, const arucohip_fisheye_t* model, const float* Knew, const float* src, int n,
                                    int on_device, float* dst);
/* Frames, for the paths that read pixels around the markers (arucohip_charuco_corners_batch, arucohip_board_recover_batch, overlays):
 * detect on the result with K = Knew and no distortion. Arguments as arucohip_undistort (1 or 3 channels, dst tightly packed in host
 * or device memory, asynchronous with a device dst). Destination pixel (x, y) reads the source at the forward model of the ray
 * Knew^-1 (x, y, 1), bilinear with 5 fractional bits (round half to even) and constant 0 outside the frame and where theta >
 * max_angle. The map is kept per (size, model, Knew, max_angle) in a slot of its own: it never evicts arucohip_undistort's map. */
int arucohip_fisheye_undistort(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, size_t row_stride,
                               size_t frame_stride, int channels, int src_on_device, const arucohip_fisheye_t* model, const float* Knew,
                               float max_angle, uint8_t* dst, int dst_on_device);
/* The device-resident markers of the first nframes frames of the LAST batch (a synchronous call, a waited ticket or a one-frame
 * arucohip_detect; every chunk worker), in place: frame f uses models[f % nmodels] (an interleaved rig stream with one lens per camera
 * is one call) and Knew + 9 (f % nmodels) (Knew: NULL or nmodels x 9 floats). Each marker's four corners become their ideal pixels;
 * has_pose is set to 0 and ssize to -1, since a pose the batch computed came from the wrong model. A marker with an invalid corner
 * leaves the list, which closes up in order; dropped[f] (host, nframes, may be NULL) counts them. Frames with n = -1 stay -1.
 * out / n_out: both NULL or both given, with the layout, capacity rule and asynchrony rule of arucohip_board_recover_batch (the call
 * is asynchronous when out is on the device or NULL and dropped is NULL).
 * Every later reader of the last batch sees the ideal corners (arucohip_board_detect_batch, arucohip_planar_poses_batch,
 * arucohip_board_map_batch, arucohip_rig_*_batch, ...: pass K = Knew, ndist = 0). Until the next detection a second call returns
 * ARUCOHIP_E_INVALID, and arucohip_board_recover_batch and arucohip_charuco_corners_batch return ARUCOHIP_E_UNSUPPORTED: they match
 * corners against the pixels of the distorted frame. For those, undistort the frames with arucohip_fisheye_undistort and detect on
 * the result. */
int arucohip_fisheye_undistort_markers_batch(arucohip_handle* h, int nframes, const arucohip_fisheye_t* models, int nmodels,
                                             const float* Knew, float max_angle, arucohip_marker_t* out, int cap, int32_t* n_out,
                                             int out_on_device, int32_t* dropped);
/* Fisheye calibration from planar views, so that K and D need no other library. Arguments as arucohip_calibrate_camera and
 * arucohip_calibrate_board_batch, with the model in/out instead of K / dist; rvecs, tvecs, per_view_rms, rms and used may be NULL.
 * Views are planar (ARUCOHIP_E_UNSUPPORTED otherwise), at most ARUCOHIP_CALIB_MAX_VIEW_POINTS points each. The algorithm is this
 * library's own:
 *  - start values: cx = (width - 1) / 2, cy = (height - 1) / 2, fx = fy = max(width, height) / pi, D = 0; with
 *    ARUCOHIP_FISHEYE_USE_INTRINSIC_GUESS the given model;
 *  - every view's start pose: its points undistorted with the start model (each angle clamped to 1.5 rad, for this start only), then
 *    the planar homography start of arucohip_calibrate_camera on the normalised points;
 *  - Levenberg-Marquardt over the 8 intrinsics and every view's pose, the poses eliminated per view (Schur complement; per point 8
 *    intrinsic, 6 pose and 1 residual column from the analytic Jacobian), the views' Gram matrices added in view order. It is
 *    arucohip_calibrate_camera's solver with this projection: CvLevMarq's rule, at most 30 accepted steps or a relative step below
 *    DBL_EPSILON. No floating-point atomics: two calls, or host and device input, give the same bits.
 * The batch form reads the distorted corners of the last batch: after arucohip_fisheye_undistort_markers_batch it returns
 * ARUCOHIP_E_INVALID. */
#define ARUCOHIP_FISHEYE_USE_INTRINSIC_GUESS 1 /* start from the given model (else its K only gives the FIX_ASPECT_RATIO ratio) */
#define ARUCOHIP_FISHEYE_FIX_ASPECT_RATIO 2    /* fx / fy stays at the ratio of the given K (1 when K holds no focal lengths) */
#define ARUCOHIP_FISHEYE_FIX_PRINCIPAL_POINT 4
#define ARUCOHIP_FISHEYE_FIX_K1 8
#define ARUCOHIP_FISHEYE_FIX_K2 16
#define ARUCOHIP_FISHEYE_FIX_K3 32
#define ARUCOHIP_FISHEYE_FIX_K4 64
int arucohip_fisheye_calibrate(arucohip_handle* h, const float* obj, const float* img, const int32_t* npoints, int nviews, int on_device,
                               int width, int height, int flags, arucohip_fisheye_t* model, double* rvecs, double* tvecs,
                               double* per_view_rms, double* rms);
int arucohip_fisheye_calibrate_board_batch(arucohip_handle* h, int nframes, const int32_t* ids, const float* obj, int nboard,
                                           int info_type, float marker_size, int min_markers, int width, int height, int flags,
                                           arucohip_fisheye_t* model, int32_t* used, double* rvecs, double* tvecs, double* rms);

/* Board occlusion mask: ChromaticMask / EMClassifier of the reference (src/chromaticmask.cpp). Each of the mc x nc cells of the board
 * holds a 2-component Gaussian mixture over the 256 grey levels of one 8-bit plane; a pixel on the board is 1 when its level is
 * "board colour" under the model, 0 where something in front of the board hides it. The reference's quirks are kept;
 * the EM fit is this library's definition (cv::ml::EM cannot be checked here). A chromatic object uses its handle's device and
 * stream but owns its own buffers: its calls never invalidate the handle's single-frame graph. Not thread-safe with its handle. */
typedef struct arucohip_chromatic arucohip_chromatic;
/* setParams(mc, nc, threshProb, CP, BC, markersize) (:122-165): the 4 board corners (x y z each) from the board's nboard markers
 * (obj: 12 floats per marker, as arucohip_board_detect). A METERS board takes the length of its first edge as marker_size.
 * ARUCOHIP_E_INVALID for an empty board, or marker_size == -1 on a board that is not METERS. */
int arucohip_chromatic_board_corners(const float* obj, int nboard, int info_type, float marker_size, float corners[12]);
/* setParams(mc, nc, threshProb, CP, BC, corners) (:167-216) for width x height frames with camera K (row-major 3x3) and dist (ndist
 * 0..8). ARUCOHIP_E_UNSUPPORTED for mc or nc of 0, nc > mc or mc * nc > 255 (undefined in the reference). */
int arucohip_chromatic_create(arucohip_handle* h, int mc, int nc, double thresh_prob, const float* K, const float* dist, int ndist, int width,
                              int height, const float corners[12], arucohip_chromatic** out);
void arucohip_chromatic_destroy(arucohip_chromatic* m);
/* One frame: a width x height plane (host, or device with on_device), its row stride and the board pose rvec / tvec (same units as
 * the corners). train (:271-313); classify with method 1 = classify (:317-354), 2 = classify2 (:372-438); update (:440-460) retrains
 * the cells with more than 50 samples under the last mask and the cell map of the last train / method-1 classify. */
int arucohip_chromatic_train(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride, const double rvec[3],
                             const double tvec[3]);
int arucohip_chromatic_classify(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride, const double rvec[3],
                                const double tvec[3], int method);
int arucohip_chromatic_update(arucohip_chromatic* m, const uint8_t* plane, int on_device, size_t row_stride);
/* calculateGridImage (:222-268) alone: the cell map of the pose; resetMask: the mask to 0 */
int arucohip_chromatic_grid(arucohip_chromatic* m, const double rvec[3], const double tvec[3]);
int arucohip_chromatic_reset_mask(arucohip_chromatic* m);
/* getMask / getCellMap: width x height bytes (mask 0 / 1, cell map 1 + cell or 0) into dst (host, or device with on_device) */
int arucohip_chromatic_get_mask(arucohip_chromatic* m, uint8_t* dst, int on_device);
int arucohip_chromatic_get_cell_map(arucohip_chromatic* m, uint8_t* dst, int on_device);
/* isValid(): 1 after a train */
int arucohip_chromatic_is_valid(arucohip_chromatic* m);
/* The model: prob[cell][256] doubles (cell = j * mc + i) and trained[cell] (1 once a fit has run). Cells never fitted hold 0.5.
 * set_model recomputes inside[cell][v] = prob > thresh_prob. */
int arucohip_chromatic_get_model(arucohip_chromatic* m, double* prob, int32_t* trained);
int arucohip_chromatic_set_model(arucohip_chromatic* m, const double* prob, const int32_t* trained);
/* EMClassifier::train on one cell's raw samples (samples_hist[v] = samples of grey level v), by the device code of the object's fit.
 * *trained = 0 when the discretised histogram holds fewer than 10 samples: prob / inside are left as they were. */
int arucohip_em_fit(arucohip_handle* h, const uint32_t samples_hist[256], double thresh_prob, double prob[256], uint8_t inside[256], int* trained);
/* Geometry of the last single-frame call (frame < 0) or of frame `frame` of the last batch: projected corners, calculateGridImage's
 * and classify2's homographies (row-major, double). Any output may be NULL. */
int arucohip_chromatic_debug_geometry(arucohip_chromatic* m, int frame, float corners2d[8], double H_train[9], double H_classify[9]);
/* The raw-sample histograms and the discretised histograms (histCount) of the last train / update, ncell x 256 each (may be NULL),
 * and per cell: 1 fitted, 0 fewer than 10 samples (model kept), -1 not retrained (update: 50 samples or fewer). */
int arucohip_chromatic_debug_hist(arucohip_chromatic* m, uint32_t* raw, uint32_t* hist_count, int32_t* fitted);
/* classify (method 1) or classify2 (method 2) of every frame of the last arucohip_detect_batch on handle h, at the board poses the last
 * arucohip_board_detect_batch left on the device (every chunk), against the current model, frozen for the batch. The model is NOT
 * updated between frames: the reference's update() makes frame f+1 depend on frame f, which a batch cannot honour. A frame without a
 * pose or with prob <= min_prob gets an all-zero mask. frames: nframes planes (host or device), masks: nframes x width x height
 * (host or device), npix[f] (may be NULL): the 1 pixels of frame f. The object's single-frame mask and cell map are not touched.
 * ARUCOHIP_E_INVALID without a board batch of nframes frames on h. */
int arucohip_chromatic_classify_batch(arucohip_chromatic* m, arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height,
                                      size_t row_stride, size_t frame_stride, int frames_on_device, int method, float min_prob, uint8_t* masks,
                                      int masks_on_device, int32_t* npix);

/* Marker::calculateExtrinsics (marker.h:98-104 / marker.cpp:112-124) for n markers at once (batched solvePnP). */
int arucohip_calculate_extrinsics(arucohip_handle* h, arucohip_marker_t* markers, int n, const float* K, const float* dist,
                                  int ndist, float marker_size, int y_perpendicular);

/* Both pose solutions of a planar marker. A square seen under weak perspective has two poses that explain its four corners almost
 * equally well; arucohip_calculate_extrinsics and the detect calls report the one solvePnP(ITERATIVE) converges to and are unchanged.
 * Here both come out of the homography in closed form (infinitesimal plane-based pose estimation, Collins and Bartoli 2014), in double
 * precision on the device; with refine != 0 each is then refined by the library's Levenberg-Marquardt (<= 20 iterations, eps
 * FLT_EPSILON) started from it. rms[j] is the root-mean-square distance in pixels between the four given corners and the projection
 * of solution j through K and dist; the solutions are ordered by it. Degenerate corners (coincident, on one line, a homography that
 * cannot be fitted, a solution behind the camera) give n_solutions = 0 and all doubles 0.
 * Only `corners` of each marker is read; on_device: markers and out are both device pointers. K is required, ndist is 0, 4, 5 or 8,
 * marker_size > 0 (ARUCOHIP_E_INVALID otherwise); y_perpendicular applies rotateXAxis to both rotations. The call returns when the
 * results are complete, and never touches the single-frame graph or the last batch. */
int arucohip_planar_poses(arucohip_handle* h, const arucohip_marker_t* markers, int n, int on_device, const float* K, const float* dist,
                          int ndist, float marker_size, int refine, int y_perpendicular, arucohip_planar_poses_t* out);
/* The same for the device-resident markers of the first nframes frames of the LAST arucohip_detect_batch call (every chunk; the batch
 * need not have been run with a pose): out[f * cap + i] belongs to marker i of frame f as that batch returned it, entries beyond a
 * frame's count are left untouched. out: host, or device with out_on_device. ARUCOHIP_E_CAPACITY when a frame holds more than cap
 * markers (nothing is written), ARUCOHIP_E_INVALID without a batch of nframes frames. */
int arucohip_planar_poses_batch(arucohip_handle* h, int nframes, const float* K, const float* dist, int ndist, float marker_size,
                                int refine, int y_perpendicular, arucohip_planar_poses_t* out, int cap, int out_on_device);

/* ---- Chessboard-corner (ChArUco) boards (DESIGN.md "ChArUco"): a chessboard whose white squares carry the markers. The calibration
 * points are the chessboard's inner corners (saddle points); the markers only say which corner is which. No counterpart in the
 * reference (OpenCV's aruco module has CharucoBoard / interpolateCornersCharuco); the algorithm is this library's, stated here.
 *
 * The board is squares_x * square_px by squares_y * square_px pixels. Square (sx, sy) is black when sx + sy is even. Every white square
 * holds one marker of side marker_px whose top-left is at (sx * square_px + m, sy * square_px + m), m = (square_px - marker_px) / 2.
 * Markers are numbered in row-major order of the white squares; marker k shows ids[k]. Inner corner c = iy * (squares_x - 1) + ix lies
 * at board pixel ((ix + 1) * square_px, (iy + 1) * square_px); its two neighbour markers are those of the two white squares among the
 * four around it. Limits (ARUCOHIP_E_INVALID otherwise): squares 2..64 each, marker_px >= 7, square_px - marker_px >= 2, at most
 * ARUCOHIP_CALIB_MAX_VIEW_POINTS inner corners, at most 1024 markers, image at most 16383 a side. */
typedef struct arucohip_charuco {
    int32_t squares_x, squares_y, square_px, marker_px;
} arucohip_charuco_t;
/* One inner corner of one frame. 32 bytes. */
typedef struct arucohip_charuco_corner {
    float x, y;              /* the refined corner (found != 0) */
    float start_x, start_y;  /* where the neighbour markers' homographies put it */
    int32_t found;
    int32_t win;             /* the refinement's half window */
    int32_t markers;         /* neighbour markers used: 0..2 */
    int32_t pad_;
} arucohip_charuco_corner_t;
typedef struct arucohip_charuco_opt {
    int32_t min_markers;     /* 1 or 2 neighbour markers a corner needs. Default 2 (OpenCV's; taken over, not measured here) */
    int32_t max_win;         /* 2..15: the largest half window of the refinement. Default 5 */
} arucohip_charuco_opt_t;
void arucohip_default_charuco(arucohip_charuco_opt_t* o);
/* The image's size, the markers and the inner corners of a layout. Any output may be NULL. Host arithmetic. */
int arucohip_charuco_board_size(const arucohip_charuco_t* layout, int* width, int* height, int* markers, int* corners);
/* The board image, painted by one launch on scratch of its own: white, the black squares, createMarkerImage(ids[k], marker_px) in every
 * white square. image: height rows of row_stride bytes (>= width, no alignment needed), host or device. obj (may be NULL): markers * 4 * 3
 * floats in pixels (PIX), y down, corner order as arucohip_fiducial_board_image: with ids it is a board for every board call.
 * corner_obj (may be NULL): corners * 3 floats. Both are shifted by (width / 2, height / 2) (integer halves) when `centered`. nids must be
 * the layout's marker count, ids 0..1023. */
int arucohip_charuco_board_image(arucohip_handle* h, const arucohip_charuco_t* layout, int centered, const int32_t* ids, int nids,
                                 uint8_t* image, size_t row_stride, int image_on_device, float* obj, float* corner_obj);
/* The inner corners of the first nframes frames of the LAST batch (a synchronous call, a waited ticket or a one-frame arucohip_detect;
 * every chunk worker), from the batch's device-resident markers. frames: the gray planes that batch saw (host or device; the handle does
 * not keep them). out[f * corners + c] (host, or device with out_on_device) and n_found[f] (host, may be NULL): the found corners of
 * frame f. A frame the batch gave up (n = -1) or without markers has found = 0 everywhere. Per corner, one wavefront:
 *  1. its two neighbour markers are looked up by id in the frame's marker list (the first entry of that id). For each one present, the
 *     homography that maps its four board-pixel corners to its four image corners is solved exactly (8 x 8, double, from the float
 *     corners as stored). A singular system or a non-positive w at the corner makes the neighbour absent. `markers` counts the
 *     neighbours used; fewer than min_markers: not found;
 *  2. the start is the mean, in double, of the neighbours' projections of the corner, rounded once to float: start_x, start_y;
 *  3. d = the smallest distance (double) from the unrounded start to an image corner of a used neighbour;
 *     win = min(max_win, (int)floor(d * 0.70710678118654752) - 1), which keeps the window off the markers' own borders. win < 2: not found;
 *  4. not found when start - (win + 1) < 0 or start + (win + 1) > size - 1 in x or y (the refinement's patch would leave the frame);
 *  5. x, y = the SUBPIX refinement (cv::cornerSubPix as the detector's SUBPIX corner method runs it: 8 iterations, step 0.005) of the
 *     float start with half window win. A refinement that leaves the window returns the start and stays found.
 * Only final marker corners and ids are read: every corner method, threshold range, pyrDown level and decoder is supported. The result
 * and the layout also stay on the device, in memory no captured launch reads, until the next call: arucohip_charuco_calibrate_batch and
 * arucohip_charuco_pose_batch work on them. ARUCOHIP_E_INVALID: a layout outside the limits, nids other than the layout's marker count,
 * nframes beyond the last batch, width / height other than that batch's frames, strides too small, min_markers outside 1..2, max_win
 * outside 2..15. opt may be NULL (defaults). */
int arucohip_charuco_corners_batch(arucohip_handle* h, const arucohip_charuco_t* layout, const int32_t* ids, int nids, const uint8_t* frames,
                                   int nframes, int width, int height, size_t row_stride, size_t frame_stride, int frames_on_device,
                                   const arucohip_charuco_opt_t* opt, arucohip_charuco_corner_t* out, int32_t* n_found, int out_on_device);
/* arucohip_calibrate_camera on the resident corners: a frame is a view when it has >= min_corners (>= 4) found corners; a corner's object
 * point is its corner_obj (not centred), times square_size / square_px when square_size > 0. The views are laid out on the device, found
 * corners in corner order, and the device solver runs unchanged. Outputs and errors as arucohip_calibrate_board_batch. */
int arucohip_charuco_calibrate_batch(arucohip_handle* h, float square_size, int min_corners, int width, int height, int flags, double K[9],
                                     double dist[5], int32_t* used, double* rvecs, double* tvecs, double* rms);
/* The board pose of the first nframes frames of the resident corners (one wavefront per frame, planar solvePnP over the found corners,
 * object points as above): out[f] (host) with n_markers = the corners used; has_pose = 0 below min_corners (>= 4), without K or when the
 * solve fails. y_perpendicular applies rotateXAxis. */
int arucohip_charuco_pose_batch(arucohip_handle* h, int nframes, const float* K, const float* dist, int ndist, float square_size,
                                int min_corners, int y_perpendicular, arucohip_board_t* out);

/* ---- Overlays: Marker::draw (marker.cpp:54-81), Board::draw and CvDrawingUtils::draw3dAxis / draw3dCube (cvdrawingutils.cpp:41-255) painted
 * into 8-bit frames where they lie (DESIGN.md "Overlay"). Primitives, order, colours (B G R) and geometry are the reference's; the pixel
 * coverage is this library's: lines are not antialiased, text uses a 5 x 7 bitmap font. Within a frame the result is that
 * of painting the primitives one after another, markers in array order; identical on every run. */
enum {
    ARUCOHIP_DRAW_OUTLINE = 1,          /* the four edges in `color`, then small squares at corners 0, 1, 2 in red, green, blue */
    ARUCOHIP_DRAW_IDS = 2,              /* "id=<id>" in 255 - color at the integer centroid */
    ARUCOHIP_DRAW_AXIS = 4,             /* markers with a pose: draw3dAxis, length 3 * ssize */
    ARUCOHIP_DRAW_CUBE = 8,             /* markers with a pose: draw3dCube */
    ARUCOHIP_DRAW_Y_PERPENDICULAR = 16  /* the cube's setYperpendicular form */
};
typedef struct arucohip_overlay {
    int32_t flags;      /* ARUCOHIP_DRAW_* */
    int32_t line_width; /* 1..7, of the outline */
    uint8_t color[4];   /* B, G, R of the outline; [3] is ignored */
} arucohip_overlay_t;
/* frames: nframes frames of height rows of width pixels with `channels` (1 or 3, B G R) interleaved bytes, rows row_stride and frames
 * frame_stride bytes apart; on a one-channel frame only component 0 of a colour is written. Bytes between width * channels and
 * row_stride are never written, and a 64 x 16 tile that nothing touches is neither read nor written. markers (nframes * cap) and
 * counts (nframes) have the layout arucohip_detect_batch writes with out_on_device: frame f draws its first min(counts[f], cap)
 * markers, none when counts[f] <= 0. markers_on_device covers both arrays. With device frames AND device markers the call is
 * asynchronous on the handle's stream, behind whatever detection is queued there (a detect -> draw chain needs no host round trip);
 * otherwise it returns when the frames are done (host frames are copied up, drawn and copied back). K (9 floats) is required for AXIS /
 * CUBE, dist: ndist (0, 4, 5, 8) floats. A primitive with an endpoint that is not finite, lies in the camera's plane or beyond +-2^20
 * is dropped whole. style NULL: OUTLINE | IDS, width 1, red (0, 0, 255), the reference's defaults. ARUCOHIP_E_INVALID: channels not 1
 * or 3, line_width outside 1..7, AXIS / CUBE without K, row_stride < width * channels, frames that overlap; ARUCOHIP_E_UNSUPPORTED:
 * frames wider or taller than the handle, cap above 65535. Uses scratch of its own: the single-frame graph and the last batch stay valid. */
int arucohip_draw_markers_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                size_t frame_stride, int frames_on_device, const arucohip_marker_t* markers, int cap, const int32_t* counts,
                                int markers_on_device, const float* K, const float* dist, int ndist, const arucohip_overlay_t* style);
/* CvDrawingUtils::draw3dAxis / draw3dCube for boards: boards[f] (rvec / tvec; nothing is drawn without has_pose) goes into frame f. The
 * axis has length 2 * marker_size and width 2 with labels X Y Z, the cube has edge marker_size (B[0].ssize in the reference). flags:
 * ARUCOHIP_DRAW_AXIS | ARUCOHIP_DRAW_CUBE | ARUCOHIP_DRAW_Y_PERPENDICULAR. K is required. Board::draw is arucohip_draw_markers_batch on
 * the board's markers. */
int arucohip_draw_boards_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                               size_t frame_stride, int frames_on_device, const arucohip_board_t* boards, int boards_on_device, float marker_size,
                               const float* K, const float* dist, int ndist, int flags);

/* ---- Plane rectification: the fronto-parallel ("bird's-eye") view of the plane a board lies in, resampled from every frame with a
 * map of its own (k_rectify.hip). No reference counterpart. With K = NULL it is what cv::warpPerspective(src, dst, M, size,
 * INTER_LINEAR | WARP_INVERSE_MAP, BORDER_CONSTANT 0) computes, up to OpenCV's own blocking (OpenCV interpolates the source position
 * inside blocks; here every pixel is projected).
 * The rule for a pixel. Frame f has the 3 x 3 row-major double map M = maps + 9 f. Output pixel (u, v), integer indices = pixel
 * centres, is computed in double, in this order, no operation fused:
 *   1. X = (M0 u + M1 v) + M2, Y = (M3 u + M4 v) + M5, W = (M6 u + M7 v) + M8. Unless W > 0 (NaN included) the pixel is 0.
 *   2. x = X / W, y = Y / W (true divisions).
 *   3. K = NULL: px = x, py = y. Otherwise the Brown model as arucohip_undistort's map applies it, k = dist[0..7] with absent
 *      coefficients 0 (k1 k2 p1 p2 k3 k4 k5 k6), fx = K[0], fy = K[4], cx = K[2], cy = K[5] (nothing else of K is used):
 *        r2 = x x + y y, kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
 *        px = fx (x kr + p1 2xy + p2 (r2 + 2 x x)) + cx, py = fy (y kr + p1 (r2 + 2 y y) + p2 2xy) + cy
 *   4. If px or py is not finite the pixel is 0.
 *   5. iu = the nearest integer, ties to even, of px * 32 clamped to [-2^31, 2^31 - 1]; sx = iu >> 5, ax = iu & 31; iv, sy, ay from py.
 *   6. Per channel the bilinear sample of arucohip_undistort's remap at (sx + ax / 32, sy + ay / 32): weights (32 - ax)(32 - ay) * 32
 *      and so on, sum + (1 << 14) >> 15, taps outside the source count 0.
 * src: nframes frames of `channels` (1 or 3) interleaved 8-bit channels; dst: nframes images of out_width x out_height (1..16383 each)
 * with the same channels. Bytes between out_width * channels and dst_row_stride are never written. valid (nframes, may be NULL: all
 * valid): a frame with valid[f] == 0 becomes all zero and its source is not read. maps_on_device covers maps and valid. K (may be
 * NULL) and dist (ndist = 0, 4, 5 or 8 floats; needs K) are host arrays. When src, maps and dst are all on the device the call is
 * asynchronous on the handle's stream, behind whatever is queued there; otherwise it returns when dst is complete. Uses scratch of its
 * own: the single-frame graph and the last batch stay valid. ARUCOHIP_E_INVALID, with a message that names it and before anything runs:
 * a null pointer, channels not 1 or 3, ndist not 0, 4, 5 or 8 (or dist without K), a stride smaller than a row or a frame, a size
 * below 1 or an output above 16383, nframes < 1, dst overlapping src. */
int arucohip_warp_plane_batch(arucohip_handle* h, const uint8_t* src, int nframes, int width, int height, int channels, size_t row_stride,
                              size_t frame_stride, int src_on_device, const double* maps, const int32_t* valid, int maps_on_device,
                              const float* K, const float* dist, int ndist, uint8_t* dst, int out_width, int out_height,
                              size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device);

typedef struct arucohip_rectify {   /* a window of the board plane, in the units the pose was solved in */
    int32_t out_width, out_height;
    float x0, y0;                   /* plane point of output pixel (0, 0) */
    float ux, uy, vx, vy;           /* plane step per output column / per output row */
} arucohip_rectify_t;

/* Host arithmetic: the window that shows a board's bounding box plus `margin` (plane units) at px_per_unit, u along +x, v along +y
 * (flip_y: v along -y, for y-up boards such as arucohip_hrm_board_image's). Object points are scaled as arucohip_board_detect
 * scales them (PIX: marker_size / first side; METERS: 1). With the box [xmin, xmax] x [ymin, ymax] of the scaled points and
 * step = 1 / px_per_unit: out_width = ceil((xmax - xmin + 2 margin) * px_per_unit), where an extent within 1e-6 (relative) above a whole
 * number of pixels counts as that number; x0 = xmin - margin + step / 2 (output pixel 0 covers the first step of the box, its centre is
 * half a step in), ux = step, uy = vx = 0; rows likewise with vy = step, or y0 = ymax + margin - step / 2 and vy = -step with flip_y.
 * For a PIX board painted by arucohip_fiducial_board_image, px_per_unit = first side / marker_size and margin 0 give one output pixel per
 * board pixel. ARUCOHIP_E_INVALID: a null pointer, nboard < 1, px_per_unit not positive and finite, margin not finite, a window of
 * less than one pixel or more than 16383. */
int arucohip_rectify_board_window(const float* obj, int nboard, int info_type, float marker_size, float px_per_unit, float margin,
                                  int flip_y, arucohip_rectify_t* win);

/* Frame f is resampled on the plane of boards[f] (rvec / tvec as the board calls return them; y_perpendicular poses are the
 * caller's to undo): maps[f] has the columns R (ux, uy, 0), R (vx, vy, 0) and R (x0, y0, 0) + t with R = Rodrigues(rvec), and the
 * rest is arucohip_warp_plane_batch with win's size. K is required. status[f] (host, may be NULL) = 1, or 0 when the frame had no
 * pose (has_pose == 0, or a map entry that is not finite) and its image is all zero. maps_out (host, may be NULL): the nframes x 9 maps
 * that were used (zeros for a frame without pose). With frames, boards and dst on the device and neither status nor maps_out the call
 * is asynchronous on the handle's stream; otherwise it returns when dst, status and maps_out are complete. ARUCOHIP_E_INVALID as above,
 * and for a window whose u and v steps are parallel, zero or not finite. */
int arucohip_board_rectify_batch(arucohip_handle* h, const uint8_t* frames, int nframes, int width, int height, int channels,
                                 size_t row_stride, size_t frame_stride, int frames_on_device, const arucohip_board_t* boards,
                                 int boards_on_device, const float* K, const float* dist, int ndist, const arucohip_rectify_t* win,
                                 uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride, int dst_on_device, int32_t* status,
                                 double* maps_out);

/* ---- Plane compositing: a texture (a label, a replacement print, a video) blended onto the plane of every frame, in place, seen through
 * the camera and its lens and hidden where a mask says so (k_composite.hip). The inverse direction of plane rectification: it runs over
 * frame pixels and leaves everything outside the texture's footprint untouched. No reference counterpart. */
typedef struct arucohip_texture {
    const uint8_t* data;
    int32_t width, height;      /* 1..16383 each */
    int32_t channels;           /* the frames' channels, or one more: the last channel is then straight (not premultiplied) alpha */
    int32_t on_device;
    size_t row_stride;          /* >= width * channels */
    size_t frame_stride;        /* 0: one texture for every frame; otherwise frame f takes data + f * frame_stride (a video on the board) */
    int32_t opacity;            /* 0..255 */
    int32_t pad_;
} arucohip_texture_t;

/* The rule for a pixel. Frame f has the 3 x 3 row-major double map N = maps + 9 f, which takes a normalised camera ray to homogeneous
 * texel coordinates. Frame pixel (u, v), integer indices = pixel centres, is computed in double, in this order, no operation fused:
 *   1. valid (nframes, may be NULL: all valid) with valid[f] == 0: the frame is untouched; neither its map nor its texture is read.
 *   2. masks (may be NULL) with masks[(f * height + v) * width + u] == 0: the pixel is untouched. Masks are nframes x height x width
 *      bytes, tightly packed: the layout arucohip_chromatic_classify_batch writes, where 1 means the board is visible.
 *   3. The ray. K = NULL: x = u, y = v. Otherwise fx = K[0], fy = K[4], cx = K[2], cy = K[5] as doubles (nothing else of K is used),
 *      ifx = 1 / fx, ify = 1 / fy, x0 = (u - cx) * ifx, y0 = (v - cy) * ify. ndist == 0: x = x0, y = y0. ndist > 0: the inverse
 *      Brown model as the pose solvers apply it (cvUndistortPoints), k = dist[0..7] with absent coefficients 0 (k1 k2 p1 p2 k3 k4 k5 k6);
 *      from x = x0, y = y0, exactly five times:
 *        r2 = x x + y y, ic = (1 + ((k[7] r2 + k[6]) r2 + k[5]) r2) / (1 + ((k[4] r2 + k[1]) r2 + k[0]) r2)
 *        dx = 2 k[2] x y + k[3] (r2 + 2 x x), dy = k[2] (r2 + 2 y y) + 2 k[3] x y, x = (x0 - dx) ic, y = (y0 - dy) ic
 *      The poses were solved through the same function, so the picture lands where the solver thinks the board is.
 *   4. S = (N0 x + N1 y) + N2, T = (N3 x + N4 y) + N5, Q = (N6 x + N7 y) + N8. Unless Q > 0 (NaN included) the pixel is untouched.
 *      s = S / Q, t = T / Q (true divisions); if either is not finite the pixel is untouched.
 *   5. is = the nearest integer, ties to even, of s * 32 clamped to [-2^31, 2^31 - 1]; it from t. The pixel is painted iff
 *      0 <= is <= 32 (tex.width - 1) and 0 <= it <= 32 (tex.height - 1): the sampling position lies inside the box of texel centres, so
 *      every tap with a non-zero weight is inside the texture and nothing darkens at the rim. Integer texel coordinates are texel
 *      centres: the outermost half texel of the texture is therefore not shown.
 *   6. Per frame channel c, C_c = the bilinear sample of arucohip_undistort's remap (as step 6 of arucohip_warp_plane_batch) of the
 *      texture at (is >> 5, it >> 5, is & 31, it & 31). A = 255 without an alpha channel, else the same sample of the texture's last
 *      channel. w = (A * opacity + 127) / 255 by integer division. w == 0: the pixel is untouched. Otherwise
 *      out_c = (C_c * w + frame_c * (255 - w) + 127) / 255; with w == 255 that is C_c exactly.
 * A pixel that is not painted keeps its value; bytes between width * channels and row_stride are never written. Minification aliases:
 * every frame pixel takes one bilinear sample, so the caller brings a texture of a resolution that suits the board's size in the frame.
 * frames: nframes frames of `channels` (1 or 3) interleaved 8-bit channels, width and height 1..16383. maps_on_device covers maps and
 * valid. K (may be NULL) and dist (ndist = 0, 4, 5 or 8 floats; needs K) are host arrays. With frames, texture, maps and masks all on the
 * device the call is asynchronous on the handle's stream, behind whatever is queued there (detect -> board pose -> classify -> composite
 * needs no host round trip); otherwise it returns when the frames are done: host frames go up, are painted and come back row by row, so
 * the caller's padding stays as it was. Uses scratch of its own: the single-frame graph and the last batch stay valid.
 * ARUCOHIP_E_INVALID, with a message that names it and before anything runs: a null h, frames, tex, tex->data or maps; channels not 1
 * or 3; tex->channels not channels or channels + 1; opacity outside 0..255; a size below 1 or above 16383 (frames and texture); a stride
 * smaller than a row or a frame (tex->frame_stride may be 0); ndist not 0, 4, 5 or 8, dist without K, ndist > 0 with dist NULL;
 * nframes < 1; the texture or the masks overlapping the frames. */
int arucohip_composite_plane_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels,
                                   size_t row_stride, size_t frame_stride, int frames_on_device, const arucohip_texture_t* tex,
                                   const double* maps, const int32_t* valid, int maps_on_device, const float* K, const float* dist,
                                   int ndist, const uint8_t* masks, int masks_on_device);

/* The texture is laid on the plane of boards[f] in frame f. The window has the meaning it has for arucohip_board_rectify_batch: texel
 * (s, t) lies at plane point (x0 + s ux + t vx, y0 + s uy + t vy); win->out_width / out_height must equal the texture's size. K is
 * required. With M the map of arucohip_board_rectify_batch (texel -> camera-frame point), the map is its signed adjugate, products unfused:
 *   N0 = M4 M8 - M5 M7, N1 = M2 M7 - M1 M8, N2 = M1 M5 - M2 M4, N3 = M5 M6 - M3 M8, N4 = M0 M8 - M2 M6, N5 = M2 M3 - M0 M5,
 *   N6 = M3 M7 - M4 M6, N7 = M1 M6 - M0 M7, N8 = M0 M4 - M1 M3, det = (M0 N0 + M1 N3) + M2 N6
 * det > 0 keeps N, det < 0 negates all nine entries: Q > 0 then holds exactly for rays that meet the plane in front of the camera,
 * whichever way the window is handed. With det zero or not finite, or without a pose, the frame is invalid: a zero map, status[f] = 0,
 * the frame untouched. The rest is arucohip_composite_plane_batch. status (host, may be NULL) and maps_out (host, may be NULL: the
 * nframes x 9 maps N actually used) make the call wait; without them, and with frames, boards, texture and masks on the device, it is
 * asynchronous on the handle's stream. ARUCOHIP_E_INVALID as above, and for null boards or win, a missing K, a window whose size differs
 * from the texture's or whose u and v steps are parallel, zero or not finite. */
int arucohip_board_composite_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels,
                                   size_t row_stride, size_t frame_stride, int frames_on_device, const arucohip_board_t* boards,
                                   int boards_on_device, const float* K, const float* dist, int ndist, const arucohip_rectify_t* win,
                                   const arucohip_texture_t* tex, const uint8_t* masks, int masks_on_device, int32_t* status,
                                   double* maps_out);

/* ---- Mesh rendering: a solid, flat-shaded triangle mesh at the pose of every marker, or of every frame's board, painted into the frames
 * in place with a depth test and hidden where a mask says so (k_render.hip, DESIGN.md "Mesh rendering"). What the reference's
 * aruco_test_gl, aruco_test_board_gl and aruco_test_board_gl_mask hand to OpenGL; a device without a graphics pipeline draws it itself.
 * The rule below is this library's own definition and does not claim to match any GL implementation. */
typedef struct arucohip_mesh {
    const float* vertices;     /* nverts * 3, the pose's object frame */
    const int32_t* triangles;  /* ntris * 3 vertex indices; counter-clockwise seen from outside (right-handed) */
    const uint8_t* colors;     /* ntris * 3, B G R per triangle; NULL: style->color for all */
    int32_t nverts, ntris;     /* 1..65536, 1..16384 */
    int32_t on_device;         /* covers the three arrays */
    int32_t pad_;
} arucohip_mesh_t;

enum {
    ARUCOHIP_RENDER_CULL_BACK = 1,   /* triangles that face away from the camera are dropped */
    ARUCOHIP_RENDER_UNLIT = 2,       /* q = 255: the base colours as they are */
    ARUCOHIP_RENDER_EDGES_INT64 = 4  /* evaluate the edge functions in int64 instead of double: the same bytes, for measurement */
};
typedef struct arucohip_render {
    int32_t flags;       /* ARUCOHIP_RENDER_* */
    int32_t opacity;     /* 0..255 */
    int32_t ambient;     /* 0..255 */
    float scale;         /* > 0, finite */
    float light[3];      /* direction towards the light, camera frame; default (0, 0, -1): a headlight */
    uint8_t color[4];    /* B G R when mesh->colors is NULL; [3] is ignored */
} arucohip_render_t;
/* CULL_BACK, opacity 255, ambient 64, scale 1, light (0, 0, -1), colour (0, 200, 0) */
void arucohip_default_render(arucohip_render_t* r);

/* Instances. Markers: every marker i < min(counts[f], cap) of frame f with has_pose is one instance at (rvec, tvec) with the object
 * point s * v for mesh vertex v, s = (double) style->scale * (double) ssize: the mesh is a shape in units of the marker's side. Boards:
 * frame f has one instance when boards[f].has_pose, with s = (double) style->scale, in the units the pose was solved in. All instances of
 * a frame share one depth test.
 * The rule for a pixel, in double unless it says integer, in this order, no operation fused:
 *   1. Vertex. R = Rodrigues(rvec) and the projection are those of the pose solvers and the overlay (cv::projectPoints): with
 *      (X, Y, Z) = (s vx, s vy, s vz) as doubles, x = ((R0 X + R1 Y) + R2 Z) + t0, y and z likewise from rows 1 and 2; the pixel
 *      (px, py) = K * Brown(x / z, y / z) with k = dist[0..7], absent coefficients 0. A triangle is dropped whole if any of its vertices
 *      has a depth z that is not > 0 (NaN included: there is no near-plane clipping), or a px or py that is not finite or lies beyond
 *      +-2^20. Edges between distorted vertices stay straight: under lens distortion that is an approximation, good for meshes whose
 *      triangles are small against the lens's curvature.
 *   2. Snap. X = the nearest integer, ties to even, of px * 16; Y from py. Integer pixel indices are pixel centres: pixel (u, v) is the
 *      point P = (16 u, 16 v). Everything up to step 5 is integer.
 *   3. Area and facing. E_ij(P) = (Xj - Xi)(Py - Yi) - (Yj - Yi)(Px - Xi) and A = E_ab(c) for the triangle's vertices a, b, c in index
 *      order. A == 0: dropped. A < 0 is front-facing: sign(A) = sign(det[a b c]) is the sign of the outward normal dotted with the
 *      view ray. With CULL_BACK triangles with A > 0 are dropped. If A < 0, b and c are swapped and A negated, so that the interior has
 *      all of E_bc, E_ca, E_ab > 0.
 *   4. Coverage. The pixel is covered iff each of E_bc(P), E_ca(P), E_ab(P) is > 0, or is == 0 on an edge that owns its points: an edge
 *      i -> j of the reordered triangle owns its points when Yj - Yi < 0 (a left edge), or Yj - Yi == 0 and Xj - Xi > 0 (a top edge).
 *      Two triangles that share an edge therefore paint every pixel of their union once. All values stay below 2^53: int64 and double
 *      evaluate them exactly.
 *   5. Depth. iz = ((E_bc / A) (1 / z_a) + (E_ca / A) (1 / z_b)) + (E_ab / A) (1 / z_c), true divisions, each E with the depth of its
 *      opposite vertex as they stand after the swap. Over the frame's instances in slot order, and each instance's triangles in index
 *      order, the first triangle that covers the pixel takes it and a later one replaces it only if its iz is strictly greater.
 *   6. Colour, per triangle, with a, b, c the camera-frame vertices (x, y, z) in the mesh's index order: n = (b - a) x (c - a),
 *      len = sqrt((nx nx + ny ny) + nz nz), d = (nx lx + ny ly) + nz lz with l = light / sqrt((lx lx + ly ly) + lz lz) computed in
 *      double from the floats; d is negated when A > 0 (the normal is turned towards the camera); lam = d / len, or 0 unless that is
 *      > 0. q = the nearest integer, ties to even, of ambient + (255 - ambient) * lam, clamped to 0..255; with UNLIT q = 255.
 *      C_c = (base_c * q + 127) / 255 in integers, base = the triangle's colour. On a one-channel frame
 *      C = (1868 C_b + 9617 C_g + 4899 C_r + 8192) >> 14, the grey of arucohip_bgr_to_gray.
 *   7. Blend. masks (may be NULL) with masks[(f * height + v) * width + u] == 0: the pixel is untouched; the layout is that of
 *      arucohip_composite_plane_batch, which arucohip_chromatic_classify_batch writes. Otherwise
 *      out_c = (C_c * opacity + frame_c * (255 - opacity) + 127) / 255 in integers: opacity 255 gives C_c exactly, opacity 0 leaves
 *      the frame untouched.
 * A pixel that no triangle covers keeps its value; bytes between width * channels and row_stride are never written, and a 64 x 16 tile
 * that nothing covers is neither read nor written. The result is the same on every run.
 * frames, markers, cap and counts as arucohip_draw_markers_batch takes them (markers_on_device covers markers and counts); K (9 floats,
 * required) and dist (ndist = 0, 4, 5 or 8 floats) are host arrays; style NULL: arucohip_default_render's. With frames, markers, mesh and
 * masks all on the device the call is asynchronous on the handle's stream, behind whatever is queued there (detect -> board pose ->
 * classify -> render -> export needs no host round trip); otherwise it returns when the frames are done. A device mesh cannot be
 * checked on the host: a triangle with an index outside 0..nverts-1 is dropped, and nothing outside the vertex array is read. Uses
 * scratch of its own, 64 MiB for a chunk of frames at a time: the single-frame graph and the last batch stay valid.
 * ARUCOHIP_E_INVALID, with a message that names it and before anything runs: a null h, frames, markers, counts, mesh, mesh->vertices or
 * mesh->triangles; K missing; channels not 1 or 3; opacity or ambient outside 0..255; a scale that is not positive and finite; a light
 * that is zero or not finite; nframes, width, height or cap below 1; nverts outside 1..65536 or ntris outside 1..16384; ndist not 0, 4,
 * 5 or 8, or dist NULL with ndist > 0; a stride smaller than a row or a frame; mesh arrays or masks overlapping the frames; a host mesh
 * with an index outside 0..nverts-1. ARUCOHIP_E_UNSUPPORTED: frames wider or taller than the handle, cap above 65535, or
 * cap * (80 + 40 nverts + 64 ntris) bytes, the scratch of one frame, above 1 GiB. */
int arucohip_render_markers_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                  size_t frame_stride, int frames_on_device, const arucohip_marker_t* markers, int cap,
                                  const int32_t* counts, int markers_on_device, const float* K, const float* dist, int ndist,
                                  const arucohip_mesh_t* mesh, const arucohip_render_t* style, const uint8_t* masks, int masks_on_device);
/* One instance per frame at boards[f] (rvec / tvec as the board calls return them; nothing is drawn without has_pose). The rest is
 * arucohip_render_markers_batch. */
int arucohip_render_boards_batch(arucohip_handle* h, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride,
                                 size_t frame_stride, int frames_on_device, const arucohip_board_t* boards, int boards_on_device,
                                 const float* K, const float* dist, int ndist, const arucohip_mesh_t* mesh, const arucohip_render_t* style,
                                 const uint8_t* masks, int masks_on_device);
/* After arucohip_enable_timing(h, 1) every render call brackets its build kernels (instances, vertices, triangles) and its raster
 * kernel with events and waits for them. *build_ms / *raster_ms (may be NULL): their averages per call since then; returns the calls. */
int arucohip_render_times(arucohip_handle* h, float* build_ms, float* raster_ms);

/* Execution time of the dominant streaming kernel (the 16-pixel-per-lane adaptive threshold kernel) from the device's constant-rate
 * clock: every wave leaves its first and last reading, *total_ms = sum over the launches since arucohip_enable_timing(h, 1) of
 * (last wave's end - first wave's start), *launches = their number (0 when another threshold kernel ran: use the event times).
 * Unlike the hipEvent interval of arucohip_kernel_times this excludes the time a dispatch queues behind other batches' kernels
 * when several batches are in flight; it is what rocprofv3 --kernel-trace reports per dispatch. No reference counterpart. */
int arucohip_threshold_exec_ms(arucohip_handle* h, double* total_ms, int* launches);

/* Per-stage device time per batch in milliseconds (hipEvent pairs on the handle's stream), the reference's
 * ARUCO_MARKER_BENCHMARK stages (markerdetector.cpp:472-476): names via arucohip_stage_name. Returns count. */
int arucohip_stage_times(arucohip_handle* h, float* ms, int cap);
const char* arucohip_stage_name(int i);
/* on = 1 starts recording (and resets the average); up to 32 batches are averaged. on = 2: no hipEvents, only the device-clock stamps behind
 * arucohip_threshold_exec_ms (an otherwise uninstrumented run). on = 0 stops both. */
int arucohip_enable_timing(arucohip_handle* h, int on);
/* Per-kernel average device time (ms per batch) since arucohip_enable_timing; names via arucohip_kernel_name. */
int arucohip_kernel_times(arucohip_handle* h, float* ms, int cap);
const char* arucohip_kernel_name(int i);

/* ---- Frame sharding over the GPUs of one node (no reference counterpart — the reference is single-process
 * CPU code; the caller shape is the frame loop of utils/aruco_test.cpp:140-160 with one detector per GPU behind one call).
 * Frames are independent units: frame f goes to device slot f mod G, there is no collective on the data path. The per-frame
 * marker blocks {n, arucohip_marker_t[cap]} are gathered once per call: each slot copies its block to pinned host memory, or
 * with ARUCOHIP_MGPU_GATHER_PEER device-to-device (xGMI) into one buffer on the first device that a single copy brings to
 * the host. One host thread per slot keeps the devices busy concurrently. (Across PROCESSES, one rank per GPU, the same
 * blocks are gathered with RCCL: bench.py / aruco_amd/dist.py.) */
enum { ARUCOHIP_MGPU_GATHER_HOST = 0, ARUCOHIP_MGPU_GATHER_PEER = 1 };
typedef struct arucohip_mgpu arucohip_mgpu;
int arucohip_mgpu_device_count(void);
/* devices: ndevices HIP device ids (NULL: 0..ndevices-1; an id may repeat, every slot gets its own handle and stream).
 * Every slot takes up to max_frames_per_device frames per call; cap = marker slots per frame in the gathered blocks. */
int arucohip_mgpu_create(const arucohip_params_t* params, const int* devices, int ndevices, int max_width, int max_height,
                         int max_frames_per_device, int cap, int flags, arucohip_mgpu** out);
void arucohip_mgpu_destroy(arucohip_mgpu* m);
int arucohip_mgpu_size(const arucohip_mgpu* m);
arucohip_handle* arucohip_mgpu_handle(arucohip_mgpu* m, int slot);   /* a slot's own handle (dictionary, callback, timing) */
int arucohip_mgpu_set_params(arucohip_mgpu* m, const arucohip_params_t* p);
const char* arucohip_mgpu_last_error_string(const arucohip_mgpu* m);
/* nframes host frames (frame f at frames + f*frame_stride), frame f -> slot f mod G; out[f*cap ..], n_out[f] in frame order. */
int arucohip_mgpu_detect_batch(arucohip_mgpu* m, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                               size_t frame_stride, const float* K, const float* dist, int ndist, float marker_size,
                               int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out);
/* One camera stream per slot, frames already resident in that slot's HBM (BASELINE config 5): frames_dev[g] = device pointer
 * on slot g's device, nframes[g] <= max_frames_per_device. Results camera-major: frame j of slot g at index
 * g*max_frames_per_device + j of out (x cap) and n_out. */
int arucohip_mgpu_detect_streams(arucohip_mgpu* m, const uint8_t* const* frames_dev, const int* nframes, int width, int height,
                                 size_t row_stride, size_t frame_stride, const float* K, const float* dist, int ndist,
                                 float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out);

/* Asynchronous form (round 3): every device slot keeps `depth` batches in flight (arucohip_set_pipeline_depth on its handle) and has one
 * persistent host thread, created with the detector, that submits a ticket's sub-batch as soon as a lane of its handle is free and waits
 * for the oldest otherwise. arucohip_mgpu_set_depth(m, d): 1 <= d <= 8 tickets outstanding (default 1; rebuilds the lanes, nothing may be
 * in flight). arucohip_mgpu_submit_batch / _submit_streams take the arguments of arucohip_mgpu_detect_batch / _detect_streams and return
 * at once with a ticket; arucohip_mgpu_wait(ticket) blocks until every slot's sub-batch is complete and the gathered blocks are in `out` /
 * `n_out` (same layout as the synchronous calls, which are submit + wait). Frames and output arrays of a ticket stay untouched until
 * its wait returns; tickets are waited for in the order they were submitted. */
int arucohip_mgpu_set_depth(arucohip_mgpu* m, int depth);   /* transactional: on failure the previous depth keeps running */
/* The gather in use: ARUCOHIP_MGPU_GATHER_PEER only if it was asked for AND every device can reach the first one (hipDeviceCanAccessPeer);
 * otherwise the blocks go through pinned host memory (ARUCOHIP_MGPU_GATHER_HOST). */
int arucohip_mgpu_gather_mode(const arucohip_mgpu* m);
int arucohip_mgpu_submit_batch(arucohip_mgpu* m, const uint8_t* frames, int nframes, int width, int height, size_t row_stride,
                               size_t frame_stride, const float* K, const float* dist, int ndist, float marker_size,
                               int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out, int* ticket);
int arucohip_mgpu_submit_streams(arucohip_mgpu* m, const uint8_t* const* frames_dev, const int* nframes, int width, int height,
                                 size_t row_stride, size_t frame_stride, const float* K, const float* dist, int ndist,
                                 float marker_size, int y_perpendicular, arucohip_marker_t* out, int cap, int32_t* n_out, int* ticket);
int arucohip_mgpu_wait(arucohip_mgpu* m, int ticket);

/* Across PROCESSES (one rank per GPU, RCCL): the block a rank contributes to the gather. arucohip_compact_markers packs the device arrays a
 * batch left with out_on_device (blocks_dev: nframes x cap markers, counts_dev: nframes int32) into ONE contiguous device block
 *   { int32 total, nframes, cap_total, overflow;  int32 counts[nframes] (padded to 16 bytes);  arucohip_marker_t markers[cap_total] }
 * with the frames' markers back to back (frame f at offset sum over j < f of min(max(counts[j], 0), cap)); overflow != 0 says that total
 * exceeded cap_total and the tail is missing. One kernel on `hip_stream` (the current device), no handle, no host round trip;
 * arucohip_compact_bytes gives the size of the block. At the bench's config 2 the block is a third of the fixed-capacity arrays.
 * No reference counterpart. */
size_t arucohip_compact_bytes(int nframes, int cap_total);
int arucohip_compact_markers(const arucohip_marker_t* blocks_dev, const int32_t* counts_dev, int nframes, int cap, void* dst_dev,
                             int cap_total, void* hip_stream);

/* ---- OpenGL / Ogre conversions of the pose results (host arithmetic, no handle, no device work).
 * GetGLModelViewMatrix (src/utils.cpp:32-69; Marker::glGetModelViewMatrix src/marker.h:90, Board:: src/board.h:109):
 * column-major 4x4 from rvec / tvec (3 doubles each). */
int arucohip_gl_modelview(const double* rvec, const double* tvec, double* modelview16);
/* The same for n markers that carry a pose (has_pose), modelview16: n*16 doubles. */
int arucohip_gl_modelview_n(const arucohip_marker_t* markers, int n, double* modelview16);
/* ... and for every marker of the LAST batch on the device (one launch, a lane per marker): modelview = host array of
 * nframes*cap*16 doubles (frame-major, zero matrices for slots without a posed marker), n_out[f] = markers of frame f. */
int arucohip_gl_modelview_batch(arucohip_handle* h, int nframes, int cap, double* modelview, int32_t* n_out);
/* GetOgrePoseParameters (src/utils.cpp:71-147): position[3], orientation[4] = quaternion (w, x, y, z). */
int arucohip_ogre_pose(const double* rvec, const double* tvec, double* position3, double* orientation4);
/* CameraParameters::glGetProjectionMatrix (src/cameraparameters.cpp:226-266) including the CameraParameters::resize
 * (:166-179) to width x height it starts with. K: 9 floats row-major, valid for cam_width x cam_height (= CamSize, which
 * the reference keeps using for the right / bottom planes after the resize). */
int arucohip_gl_projection(const float* K, int cam_width, int cam_height, int width, int height, double gnear, double gfar,
                           int invert, double* proj16);
/* CameraParameters::OgreGetProjectionMatrix (src/cameraparameters.cpp:271-295). */
int arucohip_ogre_projection(const float* K, int cam_width, int cam_height, int width, int height, double gnear, double gfar,
                             int invert, double* proj16);

#ifdef __cplusplus
}
#endif
#endif /* ARUCOHIP_H */
