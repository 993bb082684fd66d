// Host side of the board occlusion mask (k_chromatic.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "handle.h"

extern "C" {

// The object's buffers are its own. Calls run on the handle's current stream and return after it has drained.
struct arucohip_chromatic {
    arucohip_handle* h = nullptr;
    int device = 0;           // destroy() may run after the handle's
    ChromaCam cam{};
    int ncell = 0;
    double thresh = 0;
    bool valid = false;       // isValid(): a train has run
    int last_batch = 0;       // frames of the last classify_batch (debug_geometry)
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
    HIPCHK(h, m->d_frame.reserve(px));
    HIPCHK(h, m->d_cellmap.reserve(px));
    HIPCHK(h, m->d_mask.reserve(px));
    HIPCHK(h, m->d_raw.reserve(tab * sizeof(uint32_t)));
    HIPCHK(h, m->d_hcount.reserve(tab * sizeof(uint32_t)));
    HIPCHK(h, m->d_fitted.reserve(m->ncell * sizeof(int32_t)));
    HIPCHK(h, m->d_trained.reserve(m->ncell * sizeof(int32_t)));
    HIPCHK(h, m->d_prob.reserve(tab * sizeof(double)));
    HIPCHK(h, m->d_inside.reserve(tab));
    HIPCHK(h, m->d_geom.reserve(sizeof(ChromaGeom)));
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
    DevImages v;
    if (const int rc = stage_input(h, h->stream, images(plane, 1, m->cam.H, (size_t)m->cam.W, row_stride, 0, on_device), m->d_frame, 0, &v)) return rc;
    *dev = v.p, *dev_stride = v.row;
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

// EMClassifier::train of one cell by chroma_em_kernel, in the handle's arena
int arucohip_em_fit(arucohip_handle* h, const uint32_t samples_hist[256], double thresh_prob, double prob[256], uint8_t inside[256], int* trained) {
    if (!h) return ARUCOHIP_E_INVALID;
    if (!samples_hist || !prob || !inside || !trained) return fail(h, ARUCOHIP_E_INVALID, "em_fit: NULL argument");
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t *d_hist, *d_hcount;
    int32_t *d_fit, *d_tr;
    double* d_prob;
    uint8_t* d_in;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_hist = cv.take<uint32_t>(256), d_hcount = cv.take<uint32_t>(256);
            d_fit = cv.take<int32_t>(1), d_tr = cv.take<int32_t>(1);
            d_prob = cv.take<double>(256), d_in = cv.take<uint8_t>(256);
        }))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_hist, samples_hist, 1024, hipMemcpyHostToDevice, s));
    launch_chroma_em(s, 1, d_hist, 0, thresh_prob, d_hcount, d_fit, d_prob, d_in, d_tr);
    HIPCHK(h, hipGetLastError());
    int32_t fitted = 0;
    HIPCHK(h, hipMemcpyAsync(&fitted, d_fit, sizeof(fitted), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *trained = fitted == 1;
    if (fitted == 1) {
        HIPCHK(h, hipMemcpyAsync(prob, d_prob, 256 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(inside, d_in, 256, hipMemcpyDeviceToHost, s));
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
    HIPCHK(mh, m->d_bgeom.reserve((size_t)nframes * sizeof(ChromaGeom)));
    if (npix) {
        HIPCHK(mh, m->d_npix.reserve((size_t)nframes * sizeof(int32_t)));
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
    if (!frames_on_device) HIPCHK(mh, m->d_bframes.reserve(std::min(nframes, piece) * px));
    if (!masks_on_device) HIPCHK(mh, m->d_bmasks.reserve(std::min(nframes, piece) * px));
    for (int first = 0; first < nframes; first += piece) {
        const int cnt = std::min(piece, nframes - first);
        DevImages src;
        if (const int rc = stage_input(mh, s, images(frames + (size_t)first * frame_stride, cnt, H, (size_t)W, row_stride, frame_stride, frames_on_device),
                                       m->d_bframes, 0, &src))
            return rc;
        uint8_t* dst = masks_on_device ? masks + (size_t)first * px : (uint8_t*)m->d_bmasks;
        launch_chroma_classify(s, m->cam, method, m->thresh, cnt, src.p, src.row, src.frame, m->d_bgeom + first, m->d_prob, m->d_inside, dst,
                               npix ? (int32_t*)m->d_npix + first : nullptr);
        HIPCHK(mh, hipGetLastError());
        if (!masks_on_device) HIPCHK(mh, hipMemcpyAsync(masks + (size_t)first * px, dst, (size_t)cnt * px, hipMemcpyDeviceToHost, s));
    }
    if (npix) HIPCHK(mh, hipMemcpyAsync(npix, m->d_npix, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(mh, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
