// ---------------------------------------------------------------------------------------------
// Highly reliable marker dictionaries and boards (k_hrm.hip): HighlyReliableMarkers::createDicitionary and createBoardImage
// (src/highlyreliablemarkers.cpp:498-608). The scratch is carved from the handle's arena.
// ---------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include <vector>

#include "handle.h"

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
    HrmBufs bufs;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            bufs.jumps = cv.take<uint32_t>((size_t)(HRM_LANE_BITS + 1) * S31 * S31);
            bufs.state = cv.take<uint32_t>(S31);
            bufs.ctl = cv.take<HrmCtl>(1);
            bufs.code = cv.take<uint64_t>(HRM_WINDOW);
            bufs.selfd = cv.take<uint8_t>(HRM_WINDOW);
            bufs.dmin = cv.take<uint8_t>(HRM_WINDOW);
            bufs.dict = cv.take<uint64_t>((size_t)4096 * 4);
        }))
        return rc;
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
    const size_t pbytes = (size_t)HRM_POW_BITS * S31 * S31 * sizeof(uint32_t);
    uint32_t *d_pow2, *d_state, *d_out;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_pow2 = cv.take<uint32_t>((size_t)HRM_POW_BITS * S31 * S31);
            d_state = cv.take<uint32_t>(S31);
            d_out = cv.take<uint32_t>((size_t)count);
        }))
        return rc;
    std::vector<uint32_t> pow2;
    M31 P = m31_pow(1);
    for (int bit = 0; bit < HRM_POW_BITS; bit++) {
        pow2.insert(pow2.end(), P.begin(), P.end());
        P = m31_mul(P, P);
    }
    uint32_t st[S31];
    hrm_state0(seed, st);
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_pow2, pow2.data(), pbytes, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_state, st, sizeof(st), hipMemcpyHostToDevice, s));
    launch_hrm_stream(s, d_state, d_pow2, offset, count, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
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
    const size_t stride = ((size_t)W * ch + 15) & ~(size_t)15;
    uint64_t* d_codes;
    uint8_t* d_img;
    if (const int rc = carve_scratch(h, h, [&](Carver& cv) {
            d_codes = cv.take<uint64_t>((size_t)nb);
            d_img = cv.take<uint8_t>(stride * H);
        }))
        return rc;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(d_codes, codes, (size_t)nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    launch_hrm_board(s, d_codes, n, grid_w, grid_h, chromatic ? 1 : 0, W, H, ch, stride, d_img);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy2DAsync(image, row_stride, d_img, stride, (size_t)W * ch, H, image_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
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
