// Host side of the chessboard-corner (ChArUco) boards (k_charuco.hip; the painter is k_fiducial.hip's).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "handle.h"

namespace {
constexpr int CH_MAX_SIDE = 16383, CH_MAX_MARKERS = 1024, CH_IDS = 1024;

struct CharucoPlan {
    int W = 0, H = 0, markers = 0, corners = 0;
};
// false: outside the limits of arucohip.h
bool charuco_plan(const arucohip_charuco_t* L, CharucoPlan* p) {
    if (!L || L->squares_x < 2 || L->squares_x > 64 || L->squares_y < 2 || L->squares_y > 64 || L->marker_px < 7 || L->square_px > CH_MAX_SIDE ||
        (long)L->square_px - L->marker_px < 2)
        return false;
    const long W = (long)L->squares_x * L->square_px, H = (long)L->squares_y * L->square_px;
    if (W > CH_MAX_SIDE || H > CH_MAX_SIDE) return false;
    p->W = (int)W, p->H = (int)H;
    p->markers = L->squares_x * L->squares_y / 2;   // the white squares: sx + sy odd
    p->corners = (L->squares_x - 1) * (L->squares_y - 1);
    return p->corners <= ARUCOHIP_CALIB_MAX_VIEW_POINTS && p->markers <= CH_MAX_MARKERS;
}

// d_charuco: the corner records [frames][corners] at its start (where the consumers read them), then n_found [frames], then the layout's ids
size_t charuco_layout(uint8_t* base, int nframes, int corners, int nids, arucohip_charuco_corner_t** rec, int32_t** nfound, int32_t** ids) {
    Carver c{base};
    *rec = c.take<arucohip_charuco_corner_t>((size_t)nframes * corners), *nfound = c.take<int32_t>((size_t)nframes), *ids = c.take<int32_t>((size_t)nids);
    return c.at;
}

// what one unit of the board's pixels is in the caller's unit
double charuco_scale(const arucohip_charuco_t& L, float square_size) { return square_size > 0 ? (double)square_size / (double)L.square_px : 1.0; }
}  // namespace

extern "C" {

void arucohip_default_charuco(arucohip_charuco_opt_t* o) {
    if (!o) return;
    o->min_markers = 2, o->max_win = 5;
}

int arucohip_charuco_board_size(const arucohip_charuco_t* layout, int* width, int* height, int* markers, int* corners) {
    CharucoPlan p;
    if (!charuco_plan(layout, &p)) return ARUCOHIP_E_INVALID;
    if (width) *width = p.W;
    if (height) *height = p.H;
    if (markers) *markers = p.markers;
    if (corners) *corners = p.corners;
    return ARUCOHIP_OK;
}

int arucohip_charuco_board_image(arucohip_handle* h, const arucohip_charuco_t* layout, int centered, const int32_t* ids, int nids, uint8_t* image,
                                 size_t row_stride, int image_on_device, float* obj, float* corner_obj) {
    if (!h) return ARUCOHIP_E_INVALID;
    CharucoPlan p;
    if (!charuco_plan(layout, &p))
        return fail(h, ARUCOHIP_E_INVALID,
                    "charuco: squares 2..64 each, marker_px 7 or more, square_px - marker_px 2 or more, at most 512 inner corners and 1024 markers, "
                    "image at most 16383 a side");
    const arucohip_charuco_t L = *layout;
    if (!ids || !image || row_stride < (size_t)p.W) return fail(h, ARUCOHIP_E_INVALID, "charuco_board_image: NULL ids / image or row_stride too small");
    if (nids != p.markers) return fail(h, ARUCOHIP_E_INVALID, "charuco_board_image: nids is not the layout's marker count");
    for (int i = 0; i < nids; i++)
        if (ids[i] < 0 || ids[i] >= CH_IDS) return fail(h, ARUCOHIP_E_INVALID, "charuco_board_image: an id outside 0..1023");
    // a slot per square; the white ones carry the ids in row-major order
    std::vector<int32_t> slots((size_t)L.squares_x * L.squares_y, -1);
    const int m = (L.square_px - L.marker_px) / 2;
    int k = 0;
    for (int sy = 0; sy < L.squares_y; sy++)
        for (int sx = 0; sx < L.squares_x; sx++)
            if ((sx + sy) & 1) {
                slots[(size_t)sy * L.squares_x + sx] = ids[k];
                if (obj) {
                    const int x0 = sx * L.square_px + m, y0 = sy * L.square_px + m;
                    const int px[4] = {x0, x0 + L.marker_px, x0 + L.marker_px, x0}, py[4] = {y0, y0, y0 + L.marker_px, y0 + L.marker_px};
                    for (int c = 0; c < 4; c++) {
                        float* o = obj + (size_t)k * 12 + 3 * c;
                        o[0] = (float)(px[c] - (centered ? p.W / 2 : 0)), o[1] = (float)(py[c] - (centered ? p.H / 2 : 0)), o[2] = 0.f;
                    }
                }
                k++;
            }
    if (corner_obj)
        for (int c = 0; c < p.corners; c++) {
            const int ix = c % (L.squares_x - 1), iy = c / (L.squares_x - 1);
            corner_obj[3 * c] = (float)((ix + 1) * L.square_px - (centered ? p.W / 2 : 0));
            corner_obj[3 * c + 1] = (float)((iy + 1) * L.square_px - (centered ? p.H / 2 : 0));
            corner_obj[3 * c + 2] = 0.f;
        }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t rs = ((size_t)p.W + 15) & ~(size_t)15;
    int32_t* d_slots;
    uint8_t* d_img;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_slots = cv.take<int32_t>(slots.size());
            d_img = cv.take<uint8_t>(image_on_device ? 0 : rs * p.H);
        }))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_slots, slots.data(), slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const FidLayout FL{p.W, p.H, p.W, p.H, 0, L.squares_x, L.squares_y, L.marker_px, L.square_px, L.marker_px / 7, L.square_px, m};
    if (image_on_device) {
        launch_fid_paint(s, FL, d_slots, 1, image, row_stride, 0);
        HIPCHK(h, hipGetLastError());
    } else {
        launch_fid_paint(s, FL, d_slots, 1, d_img, rs, 0);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpy2DAsync(image, row_stride, d_img, rs, p.W, p.H, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_charuco_corners_batch(arucohip_handle* h, const arucohip_charuco_t* layout, const int32_t* ids, int nids, const uint8_t* frames, int nframes,
                                   int W, int H, size_t row_stride, size_t frame_stride, int frames_on_device, const arucohip_charuco_opt_t* opt,
                                   arucohip_charuco_corner_t* out, int32_t* n_found, int out_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    CharucoPlan p;
    if (!charuco_plan(layout, &p)) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: a layout outside the limits");
    if (!ids || !frames || !out) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: NULL ids / frames / out");
    if (nids != p.markers) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: nids is not the layout's marker count");
    arucohip_charuco_opt_t o;
    arucohip_default_charuco(&o);
    if (opt) o = *opt;
    if (o.min_markers < 1 || o.min_markers > 2) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: min_markers is 1 or 2");
    if (o.max_win < 2 || o.max_win > 15) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: max_win is 2..15");
    if (nframes < 1 || nframes > h->last.frames) return fail(h, ARUCOHIP_E_INVALID, "nframes exceeds the last batch");
    if (W != h->last.frame_w || H != h->last.frame_h) return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: width / height are not the last batch's");
    if (h->last.ideal)
        return fail(h, ARUCOHIP_E_UNSUPPORTED, "charuco_corners_batch: the markers hold ideal corners (arucohip_fisheye_undistort_markers_batch); undistort the frames instead");
    if (row_stride < (size_t)W || (nframes > 1 && frame_stride < row_stride * (size_t)(H - 1) + W))
        return fail(h, ARUCOHIP_E_INVALID, "charuco_corners_batch: strides too small");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch b = h->last.cut(nframes);
    arucohip_handle* w0 = b.span[0].w;   // the worker of the batch's first chunk: copies run on its stream
    hipStream_t s0 = w0->stream;
    h->charuco.frames = 0;               // nothing resident until this call completes
    arucohip_charuco_corner_t* d_rec;
    int32_t *d_nf, *d_ids;
    HIPCHK(h, h->d_charuco.reserve(charuco_layout(nullptr, nframes, p.corners, nids, &d_rec, &d_nf, &d_ids)));
    charuco_layout(h->d_charuco, nframes, p.corners, nids, &d_rec, &d_nf, &d_ids);
    HIPCHK(h, hipMemcpyAsync(d_ids, ids, (size_t)nids * sizeof(int32_t), hipMemcpyHostToDevice, s0));
    HIPCHK(h, hipMemsetAsync(d_nf, 0, (size_t)nframes * sizeof(int32_t), s0));
    CharucoArgs a{};
    a.L = *layout, a.ids = d_ids, a.width = W, a.height = H, a.min_markers = o.min_markers, a.max_win = o.max_win;
    const Images in = images(frames, nframes, H, (size_t)W, row_stride, frame_stride, frames_on_device);
    size_t frames_at;   // host frames are staged in the first worker's arena, on its stream (after a waited ticket w0 is a lane, not h)
    if (const int rc = carve_scratch(w0, h, [&](Carver& cv) {
            frames_at = cv.take_at(frames_on_device ? 0 : in.packed_bytes());
        }))
        return rc;
    DevImages gray;
    if (const int rc = stage_input(h, s0, in, w0->scratch, frames_at, &gray)) return rc;
    a.row_stride = gray.row, a.frame_stride = gray.frame;
    // every worker interpolates the corners of the frames it detected, on its own stream
    const int rc = on_workers(h, b, [&](const Span& s) {
        a.gray = gray.p + (size_t)s.first * gray.frame;
        launch_charuco_corners(s.w->stream, s.count, s.w->buf, a, d_rec + (size_t)s.first * p.corners, d_nf + s.first);
        return 0;
    });
    if (rc) return rc;
    h->charuco.n_found.assign((size_t)nframes, 0);
    HIPCHK(h, hipMemcpyAsync(h->charuco.n_found.data(), d_nf, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s0));
    HIPCHK(h, hipMemcpyAsync(out, d_rec, (size_t)nframes * p.corners * sizeof(arucohip_charuco_corner_t),
                             out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s0));
    HIPCHK(h, hipStreamSynchronize(s0));
    if (n_found) std::memcpy(n_found, h->charuco.n_found.data(), (size_t)nframes * sizeof(int32_t));
    h->charuco.layout = *layout, h->charuco.frames = nframes;
    return ARUCOHIP_OK;
}

int arucohip_charuco_calibrate_batch(arucohip_handle* h, float square_size, int min_corners, int W, int H, int flags, double* K, double* dist,
                                     int32_t* used, double* rvecs, double* tvecs, double* rms) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!K || !dist || W <= 0 || H <= 0) return fail(h, ARUCOHIP_E_INVALID, "charuco_calibrate_batch: NULL K / dist or an empty image size");
    if (min_corners < 4) return fail(h, ARUCOHIP_E_INVALID, "charuco_calibrate_batch: min_corners must be 4 or more");
    const int nframes = h->charuco.frames;
    if (nframes < 1) return fail(h, ARUCOHIP_E_INVALID, "charuco_calibrate_batch: no arucohip_charuco_corners_batch before");
    const arucohip_charuco_t L = h->charuco.layout;
    const int nc = (L.squares_x - 1) * (L.squares_y - 1);
    std::vector<int2> views;
    int total = 0;
    for (int f = 0; f < nframes; f++) {
        const int n = h->charuco.n_found[f];
        const bool take = n >= min_corners;
        if (used) used[f] = take ? 1 : 0;
        if (take) views.push_back(make_int2(f, total)), total += n;
    }
    if (views.empty()) return fail(h, ARUCOHIP_E_INVALID, "no frame holds min_corners chessboard corners");
    HIPCHK(h, hipSetDevice(h->device));
    const int V = (int)views.size();
    // the views live in a Mem of their own, not in the arena: arucohip_calibrate_camera below reads them and carves the arena itself
    int2* d_views;
    int32_t* d_npt;
    float *d_obj, *d_img;
    auto layout = [&](uint8_t* base) {
        Carver cv{base};
        d_views = cv.take<int2>((size_t)V), d_npt = cv.take<int32_t>((size_t)V);
        d_obj = cv.take<float>((size_t)total * 3), d_img = cv.take<float>((size_t)total * 2);
        return cv.at;
    };
    HIPCHK(h, h->d_charuco_views.reserve(layout(nullptr)));
    layout(h->d_charuco_views);
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_views, views.data(), (size_t)V * sizeof(int2), hipMemcpyHostToDevice, s));
    launch_charuco_gather(s, L, charuco_scale(L, square_size), (const arucohip_charuco_corner_t*)(uint8_t*)h->d_charuco, d_views, V, d_obj, d_img, d_npt);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    // the device solver, unchanged, on the device-resident views
    return arucohip_calibrate_camera(h, d_obj, d_img, d_npt, V, 1, W, H, flags, K, dist, rvecs, tvecs, nullptr, rms);
}

int arucohip_charuco_pose_batch(arucohip_handle* h, int nframes, const float* K, const float* dist, int ndist, float square_size, int min_corners,
                                int y_perp, arucohip_board_t* out) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!out) return fail(h, ARUCOHIP_E_INVALID, "charuco_pose_batch: NULL out");
    if (min_corners < 4) return fail(h, ARUCOHIP_E_INVALID, "charuco_pose_batch: min_corners must be 4 or more");
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8)) return fail(h, ARUCOHIP_E_INVALID, "ndist must be 0, 4, 5 or 8");
    if (ndist > 0 && !dist) return fail(h, ARUCOHIP_E_INVALID, "charuco_pose_batch: dist is NULL with ndist > 0");
    if (nframes < 1 || nframes > h->charuco.frames) return fail(h, ARUCOHIP_E_INVALID, "charuco_pose_batch: nframes exceeds the last arucohip_charuco_corners_batch");
    CamModel cam;
    fill_cam(&cam, K, dist, ndist, square_size, y_perp);
    HIPCHK(h, hipSetDevice(h->device));
    const arucohip_charuco_t L = h->charuco.layout;
    arucohip_board_t* d_out;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_out = cv.take<arucohip_board_t>((size_t)nframes);
        }))
        return rc;
    hipStream_t s = h->stream;
    launch_charuco_pose(s, L, charuco_scale(L, square_size), (const arucohip_charuco_corner_t*)(uint8_t*)h->d_charuco, nframes, min_corners, cam, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)nframes * sizeof(arucohip_board_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
