// ---------------------------------------------------------------------------------------------
// The default 5x5 Hamming markers (k_fiducial.hip): FiducidalMarkers::createMarkerImage, getMarkerMat, createBoardImage,
// createBoardImage_ChessBoard, createBoardImage_Frame and the id shuffle behind them (src/arucofidmarkers.cpp:40-61, :214-430),
// utils/aruco_board_pix2meters.cpp and utils/aruco_selectoptimalmarkers.cpp. The scratch is carved from the handle's arena.
// ---------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "handle.h"

namespace {
constexpr int FID_IDS = 1024;          // markers of the family
constexpr int FID_MAX_SIDE = 16383;    // the largest frame side a handle accepts
constexpr size_t FID_MAX_STAGE = (size_t)1 << 30;   // bytes of marker images staged for a host destination in one call

// The cells of a board that carry a marker, row by row, and the image's size. false: outside the limits, or a chessboard that places
// more markers than it draws ids (CV_Assert at :362).
struct BoardPlan {
    int W = 0, H = 0, pitch = 0, drawn = 0;
    std::vector<int> cell;   // y * grid_w + x of every placed marker, in order
};
bool board_plan(int type, int gw, int gh, int size, int dist, BoardPlan* p) {
    if (type < 0 || type > 2 || gw < 1 || gh < 1 || gw > 128 || gh > 128 || size < 7 || size > FID_MAX_SIDE || dist < 0 || dist > FID_MAX_SIDE) return false;
    if (type == 1) dist = 0;
    const long W = (long)gw * size + (long)(gw - 1) * dist, H = (long)gh * size + (long)(gh - 1) * dist;
    if (W > FID_MAX_SIDE || H > FID_MAX_SIDE) return false;
    p->W = (int)W, p->H = (int)H, p->pitch = size + dist;
    p->drawn = type == 0 ? gw * gh : type == 1 ? 3 * (gw * gh) / 4 : 2 * gh * 2 * gw;
    p->cell.clear();
    for (int y = 0; y < gh; y++) {
        bool to_write = y % 2 != 0;
        for (int x = 0; x < gw; x++) {
            to_write = !to_write;
            const bool place = type == 0 ? true : type == 1 ? to_write : (y == 0 || y == gh - 1 || x == 0 || x == gw - 1);
            if (place) p->cell.push_back(y * gw + x);
        }
    }
    if (type == 1 && (int)p->cell.size() > p->drawn) return false;
    return (int)p->cell.size() <= FID_IDS;
}
}  // namespace

extern "C" {

int arucohip_fiducial_marker_side(int size, int locked) {
    if (size < 7 || size > FID_MAX_SIDE) return 0;
    const int side = locked ? size + 2 * (int)((float)size * 0.25f) : size;
    return side <= FID_MAX_SIDE ? side : 0;
}

int arucohip_fiducial_marker_mat(int id, uint8_t* out25) {
    if (id < 0 || id >= FID_IDS || !out25) return ARUCOHIP_E_INVALID;
    static const int words[4] = {0x10, 0x17, 0x09, 0x0e};
    for (int y = 0; y < 5; y++) {
        const int val = words[(id >> 2 * (4 - y)) & 3];
        for (int x = 0; x < 5; x++) out25[5 * y + x] = (uint8_t)((val >> (4 - x)) & 1);
    }
    return ARUCOHIP_OK;
}

int arucohip_fiducial_marker_images(arucohip_handle* h, const int32_t* ids, int n, int size, int locked, uint8_t* images, size_t row_stride,
                                    size_t image_stride, int images_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const int side = arucohip_fiducial_marker_side(size, locked);
    if (!side) return fail(h, ARUCOHIP_E_INVALID, "fiducial_marker_images: size must be 7 or more and the image side at most 16383");
    if (!ids || !images || n < 1 || n > FID_IDS) return fail(h, ARUCOHIP_E_INVALID, "fiducial_marker_images: NULL ids / images, or n outside 1..1024");
    if (row_stride < (size_t)side || (n > 1 && image_stride < (size_t)(side - 1) * row_stride + side))
        return fail(h, ARUCOHIP_E_INVALID, "fiducial_marker_images: row_stride below the side, or image_stride below an image");
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= FID_IDS) return fail(h, ARUCOHIP_E_INVALID, "fiducial_marker_images: an id outside 0..1023 (CV_Assert in the reference)");
    const size_t rs = ((size_t)side + 15) & ~(size_t)15, is = rs * side;
    if (!images_on_device && is * n > FID_MAX_STAGE)
        return fail(h, ARUCOHIP_E_INVALID, "fiducial_marker_images: more than 2^30 bytes of images for a host destination in one call");
    HIPCHK(h, hipSetDevice(h->device));
    int32_t* d_ids;
    uint8_t* d_img;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_ids = cv.take<int32_t>((size_t)n);
            d_img = cv.take<uint8_t>(images_on_device ? 0 : is * n);
        }))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_ids, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int q = (side - size) / 2;
    const FidLayout L{side, side, size, size, q, 1, 1, size, size, size / 7};
    if (images_on_device) {
        launch_fid_paint(s, L, d_ids, n, images, row_stride, image_stride);
        HIPCHK(h, hipGetLastError());
    } else {
        launch_fid_paint(s, L, d_ids, n, d_img, rs, is);
        HIPCHK(h, hipGetLastError());
        if (n == 1 || image_stride == (size_t)side * row_stride) {
            HIPCHK(h, hipMemcpy2DAsync(images, row_stride, d_img, rs, side, (size_t)side * n, hipMemcpyDeviceToHost, s));
        } else {
            for (int i = 0; i < n; i++)
                HIPCHK(h, hipMemcpy2DAsync(images + (size_t)i * image_stride, row_stride, d_img + (size_t)i * is, rs, side, side,
                                           hipMemcpyDeviceToHost, s));
        }
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_fiducial_shuffle_ids(uint64_t* rng_state, int n, const int32_t* excluded, int nexcluded, int32_t* ids_out) {
    if (!rng_state || n < 0 || nexcluded < 0 || (nexcluded && !excluded) || (n && !ids_out) || (long)n + nexcluded > FID_IDS) return ARUCOHIP_E_INVALID;
    int list[FID_IDS];
    for (int i = 0; i < FID_IDS; i++) list[i] = i;
    for (int i = 0; i < nexcluded; i++) {
        if (excluded[i] < 0 || excluded[i] >= FID_IDS) return ARUCOHIP_E_INVALID;   // the reference writes outside its list
        list[excluded[i]] = -1;
    }
    // std::random_shuffle(first, last, cv::theRNG()) as libstdc++ runs it; cv::RNG is a multiply-with-carry generator
    uint64_t state = *rng_state;
    for (int i = 1; i < FID_IDS; i++) {
        state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32);
        const int j = (int)((uint32_t)state % (uint32_t)(i + 1));
        if (i != j) std::swap(list[i], list[j]);
    }
    *rng_state = state;
    for (int i = 0, k = 0; k < n; i++)
        if (list[i] != -1) ids_out[k++] = list[i];
    return ARUCOHIP_OK;
}

int arucohip_fiducial_board_size(int type, int grid_w, int grid_h, int marker_size, int marker_distance, int* width, int* height, int* ids_drawn,
                                 int* markers) {
    BoardPlan p;
    if (!board_plan(type, grid_w, grid_h, marker_size, marker_distance, &p)) return ARUCOHIP_E_INVALID;
    if (width) *width = p.W;
    if (height) *height = p.H;
    if (ids_drawn) *ids_drawn = p.drawn;
    if (markers) *markers = (int)p.cell.size();
    return ARUCOHIP_OK;
}

int arucohip_fiducial_board_image(arucohip_handle* h, int type, int grid_w, int grid_h, int marker_size, int marker_distance, int centered,
                                  const int32_t* ids, int nids, uint8_t* image, size_t row_stride, int image_on_device, float* obj) {
    if (!h) return ARUCOHIP_E_INVALID;
    BoardPlan p;
    if (!board_plan(type, grid_w, grid_h, marker_size, marker_distance, &p))
        return fail(h, ARUCOHIP_E_INVALID,
                    "fiducial_board_image: type 0..2, grid 1..128 x 1..128, marker size 7 or more, distance 0 or more, image at most 16383 x 16383 "
                    "and 1024 markers; a chessboard must not place more markers than 3 (w h) / 4 (CV_Assert in the reference)");
    const int nm = (int)p.cell.size();
    if (!ids || !image || row_stride < (size_t)p.W) return fail(h, ARUCOHIP_E_INVALID, "fiducial_board_image: NULL ids / image or row_stride too small");
    if (nids < nm) return fail(h, ARUCOHIP_E_INVALID, "fiducial_board_image: fewer ids than the layout places markers");
    for (int i = 0; i < nm; i++)
        if (ids[i] < 0 || ids[i] >= FID_IDS) return fail(h, ARUCOHIP_E_INVALID, "fiducial_board_image: an id outside 0..1023 (CV_Assert in the reference)");
    std::vector<int32_t> slots((size_t)grid_w * grid_h, -1);
    for (int k = 0; k < nm; k++) slots[p.cell[k]] = ids[k];
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
    const FidLayout L{p.W, p.H, p.W, p.H, 0, grid_w, grid_h, marker_size, p.pitch, marker_size / 7};
    if (image_on_device) {
        launch_fid_paint(s, L, d_slots, 1, image, row_stride, 0);
        HIPCHK(h, hipGetLastError());
    } else {
        launch_fid_paint(s, L, d_slots, 1, d_img, rs, 0);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpy2DAsync(image, row_stride, d_img, rs, p.W, p.H, hipMemcpyDeviceToHost, s));
    }
    if (obj) {   // TInfo.objPoints: integer pixel positions as float, minus the integer centre (the panel always, the others on request)
        const bool centre = type == 0 || centered;
        const float cx = (float)(p.W / 2), cy = (float)(p.H / 2);
        for (int k = 0; k < nm; k++) {
            const int x0 = (p.cell[k] % grid_w) * p.pitch, y0 = (p.cell[k] / grid_w) * p.pitch;
            const int px[4] = {x0, x0 + marker_size, x0 + marker_size, x0}, py[4] = {y0, y0, y0 + marker_size, y0 + marker_size};
            for (int c = 0; c < 4; c++) {
                float* o = obj + (size_t)k * 12 + 3 * c;
                o[0] = centre ? (float)px[c] - cx : (float)px[c];
                o[1] = centre ? (float)py[c] - cy : (float)py[c];
                o[2] = 0.f;
            }
        }
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_board_pix_to_meters(const float* obj, int nmarkers, float marker_size_m, float* obj_out) {
    if (!obj || !obj_out || nmarkers < 1) return ARUCOHIP_E_INVALID;
    // int markerSizePix = cv::norm(objPoints[0][0] - objPoints[0][1]): a float difference, its norm in double, truncated
    const float d[3] = {obj[0] - obj[3], obj[1] - obj[4], obj[2] - obj[5]};
    const int pix = (int)std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    if (pix <= 0) return ARUCOHIP_E_INVALID;   // the reference divides by zero
    const float scale = marker_size_m / (float)pix;
    for (size_t i = 0; i < (size_t)nmarkers * 12; i++) obj_out[i] = obj[i] * scale;
    return ARUCOHIP_OK;
}

int arucohip_board_place(const float* obj, int nmarkers, const double rvec[3], const double tvec[3], float* obj_out) {
    if (!obj || !obj_out || !rvec || !tvec || nmarkers < 0) return ARUCOHIP_E_INVALID;
    // Rodrigues in double: R = cos I + (1 - cos) u u^T + sin [u]x
    const double th = std::sqrt(rvec[0] * rvec[0] + rvec[1] * rvec[1] + rvec[2] * rvec[2]);
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0) {
        const double u[3] = {rvec[0] / th, rvec[1] / th, rvec[2] / th}, c = std::cos(th), s = std::sin(th);
        const double ux[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i * 3 + j] = c * (i == j) + (1.0 - c) * u[i] * u[j] + s * ux[i * 3 + j];
    }
    for (size_t i = 0; i < (size_t)nmarkers * 4; i++) {   // one rounding to float per coordinate; obj_out may be obj
        const double p[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
        for (int c = 0; c < 3; c++) obj_out[3 * i + c] = (float)(R[c * 3] * p[0] + R[c * 3 + 1] * p[1] + R[c * 3 + 2] * p[2] + tvec[c]);
    }
    return ARUCOHIP_OK;
}

int arucohip_fiducial_distances(arucohip_handle* h, int32_t* dist, int on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!dist) return fail(h, ARUCOHIP_E_INVALID, "fiducial_distances: NULL dist");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)FID_IDS * FID_IDS * sizeof(int32_t);
    hipStream_t s = h->stream;
    if (on_device) {
        launch_fid_distances(s, dist);
        HIPCHK(h, hipGetLastError());
    } else {
        int32_t* d_dist;
        if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
                d_dist = cv.take<int32_t>((size_t)FID_IDS * FID_IDS);
            }))
            return rc;
        launch_fid_distances(s, d_dist);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(dist, d_dist, bytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

int arucohip_fiducial_select(arucohip_handle* h, int n_markers, int min_entropy, int32_t* ids_out, int* n_selected, int* min_dist) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (n_markers < 1 || n_markers > FID_IDS || !ids_out) return fail(h, ARUCOHIP_E_INVALID, "fiducial_select: n_markers must be 1..1024 and ids_out not NULL");
    HIPCHK(h, hipSetDevice(h->device));
    int32_t* d_sel;   // the ids, then the four result words: one array, read back in one copy
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_sel = cv.take<int32_t>(FID_IDS + 4);
        }))
        return rc;
    hipStream_t s = h->stream;
    launch_fid_select(s, n_markers, min_entropy, d_sel, d_sel + FID_IDS);
    HIPCHK(h, hipGetLastError());
    int32_t out[FID_IDS + 4];
    HIPCHK(h, hipMemcpyAsync(out, d_sel, sizeof(out), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const int32_t* res = out + FID_IDS;
    const int found = std::min(std::max(res[0], 0), n_markers);
    for (int i = 0; i < found; i++) ids_out[i] = out[i];
    if (n_selected) *n_selected = found;
    if (min_dist) *min_dist = res[2];
    if (!res[1])
        return fail(h, ARUCOHIP_E_INVALID, "fiducial_select: no further marker at a distance above 1 (COUDL NOT ADD ANY MARKER in the reference)");
    return ARUCOHIP_OK;
}

}  // extern "C"
