// Board occlusion mask: ChromaticMask / EMClassifier of the reference (src/chromaticmask.cpp) on the device.
//
//   chroma_geometry_kernel : projectPoints of the 4 board corners and the two getPerspectiveTransform solves, one wave per frame
//   chroma_grid_kernel     : calculateGridImage, the cell map of the 2x2 blocks (:222-268)
//   chroma_hist_kernel     : the raw-sample histogram of every cell (train :271-313, update :440-460), LDS first, then global
//   chroma_em_kernel       : EMClassifier::train (:55-120), one wave per cell over its 256 grey levels, in double
//   chroma_classify_kernel : classify (:317-354) or classify2 (:372-438) per pixel with the 3x3 MORPH_CLOSE fused (2-pixel halo)
//
// Every float / double operation is in the restatement's order (tests/chromatic_ref.py); the library is built with -ffp-contract=off.
// The reference's quirks are restated as written ("Board occlusion mask").
#include <float.h>

#include "internal.h"
#include "decode_device.h"
#include "pnp_device.h"

namespace ah {

// ---- geometry
__global__ __launch_bounds__(64) void chroma_geometry_kernel(ChromaCam c, const arucohip_board_t* boards, const float* prob, float min_prob,
                                                             double r0, double r1, double r2, double t0, double t1, double t2, ChromaGeom* out) {
    __shared__ float s_c[8];
    __shared__ double sA[2][64], sb[2][8];
    const int f = blockIdx.x, lane = threadIdx.x;
    double r[3] = {r0, r1, r2}, t[3] = {t0, t1, t2};
    int valid = 1;
    if (boards) {
        const arucohip_board_t& b = boards[f];
        for (int k = 0; k < 3; k++) r[k] = b.rvec[k], t[k] = b.tvec[k];
        valid = b.has_pose && (!prob || prob[f] > min_prob);
    }
    if (lane < 4) {   // cv::projectPoints of corner `lane`, stored as Point2f
        double R[9], mx, my;
        rodrigues_vec2mat(r, R, nullptr);
        const float* p = c.corners3d + 3 * lane;
        project_point(p[0], p[1], p[2], R, nullptr, t, c.K, c.k, &mx, &my, nullptr, nullptr);
        s_c[2 * lane] = (float)mx, s_c[2 * lane + 1] = (float)my;
    }
    __syncthreads();
    ChromaGeom* g = out + f;
    if (lane < 2) {   // lane 0: calculateGridImage's transform, lane 1: classify2's
        const float ex = lane == 0 ? (float)CHROMA_CELL * (float)c.mc - 1 : (float)(c.mc - 1);
        const float ey = lane == 0 ? (float)CHROMA_CELL * (float)c.nc - 1 : (float)(c.nc - 1);
        const float dst[8] = {0, 0, ex, 0, ex, ey, 0, ey};
        perspective_transform_solve(s_c, dst, sA[lane], sb[lane], true);
        double* H = lane == 0 ? g->Ht : g->Hc;
        for (int i = 0; i < 8; i++) H[i] = sb[lane][i];
        H[8] = 1.0;
    }
    if (lane == 0) {
        // cv::boundingRect of the float corners (floor of the extremes, width = floor(max) - floor(min) + 1), then fitRectToSize as
        // written: x and y are clamped to 0 FIRST and the end is the clamped start plus the unclamped width (a rectangle that starts
        // left of / above the frame is scanned that many columns / rows further; restated), then clipped to the frame. The extremes
        // are clamped so that a corner far outside the frame cannot overflow the int conversion; the end is formed in 64 bits.
        float x0 = s_c[0], x1 = s_c[0], y0 = s_c[1], y1 = s_c[1];
        for (int i = 1; i < 4; i++) {
            x0 = fminf(x0, s_c[2 * i]), x1 = fmaxf(x1, s_c[2 * i]);
            y0 = fminf(y0, s_c[2 * i + 1]), y1 = fmaxf(y1, s_c[2 * i + 1]);
        }
        const float lim = 1e9f;
        const int ix0 = (int)floorf(fminf(fmaxf(x0, -lim), lim)), ix1 = (int)floorf(fminf(fmaxf(x1, -lim), lim)) + 1;
        const int iy0 = (int)floorf(fminf(fmaxf(y0, -lim), lim)), iy1 = (int)floorf(fminf(fmaxf(y1, -lim), lim)) + 1;
        for (int i = 0; i < 8; i++) g->corners[i] = s_c[i];
        const int rx0 = max(ix0, 0), ry0 = max(iy0, 0);
        g->rx0 = rx0, g->ry0 = ry0;
        g->rx1 = (int)min((long long)rx0 + ((long long)ix1 - ix0), (long long)c.W);
        g->ry1 = (int)min((long long)ry0 + ((long long)iy1 - iy0), (long long)c.H);
        g->valid = valid, g->pad_ = 0;
    }
}

void launch_chroma_geometry(hipStream_t s, const ChromaCam& c, int nframes, const arucohip_board_t* boards, const float* prob, float min_prob,
                            const double* rvec, const double* tvec, ChromaGeom* out) {
    const double z[3] = {0, 0, 0};
    const double* r = rvec ? rvec : z;
    const double* t = tvec ? tvec : z;
    hipLaunchKernelGGL(chroma_geometry_kernel, dim3(nframes), dim3(64), 0, s, c, boards, prob, min_prob, r[0], r[1], r[2], t[0], t[1], t[2], out);
}

// calculateGridImage for the 2x2 block whose top-left pixel is (x, y) (both even): cv::perspectiveTransform in double on the float
// pixel (|w| <= FLT_EPSILON gives (0, 0)), the float result / 20, Point2f::inside(Rect(0, 0, mc, nc)), then the cell number
// (uint)y * nc + (uint)x as a uchar (nc, not mc: restated). Returns 1 + cell, or 0 outside.
__device__ __forceinline__ int chroma_cell(const double* m, int x, int y, int mc, int nc) {
    const float fx = (float)x, fy = (float)y;
    double w = fx * m[6] + fy * m[7] + m[8];
    float px = 0, py = 0;
    if (fabs(w) > (double)FLT_EPSILON) {
        w = 1. / w;
        px = (float)((fx * m[0] + fy * m[1] + m[2]) * w);
        py = (float)((fx * m[3] + fy * m[4] + m[5]) * w);
    }
    px /= (float)CHROMA_CELL;
    py /= (float)CHROMA_CELL;
    if (!(0.f <= px && px < (float)mc && 0.f <= py && py < (float)nc)) return 0;
    return 1 + (int)(uint8_t)((unsigned)py * (unsigned)nc + (unsigned)px);
}

// one thread per 2x2 block of the even part of the frame; an odd last row / column is never written (it keeps the create-time 0)
__global__ void chroma_grid_kernel(ChromaCam c, const ChromaGeom* g, uint8_t* cellmap) {
    const int bw = c.W / 2, bh = c.H / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bw * bh) return;
    const int by = i / bw, bx = i - by * bw;
    const int x = 2 * bx, y = 2 * by;
    const uint8_t v = (uint8_t)chroma_cell(g->Ht, x, y, c.mc, c.nc);
    uint8_t* p = cellmap + (size_t)y * c.W + x;
    p[0] = v, p[1] = v, p[c.W] = v, p[c.W + 1] = v;
}

void launch_chroma_grid(hipStream_t s, const ChromaCam& c, const ChromaGeom* g, uint8_t* cellmap) {
    const int n = (c.W / 2) * (c.H / 2);
    if (n > 0) hipLaunchKernelGGL(chroma_grid_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c, g, cellmap);
}

// ---- raw-sample histograms: a 64 x 16 tile touches a few cells; the first HIST_SLOTS of them count in LDS, the rest go straight to
// global atomics. Integer counts: the result does not depend on the order.
constexpr int HIST_TW = 64, HIST_TH = 16, HIST_SLOTS = 8;
__global__ __launch_bounds__(256) void chroma_hist_kernel(int W, int H, const uint8_t* in, size_t stride, const uint8_t* cellmap, const uint8_t* mask,
                                                          uint32_t* raw) {
    __shared__ uint32_t s_h[HIST_SLOTS * 256];
    __shared__ int s_slot[256];
    const int tid = threadIdx.x;
    for (int i = tid; i < HIST_SLOTS * 256; i += 256) s_h[i] = 0;
    s_slot[tid] = 0;
    __syncthreads();
    const int x0 = blockIdx.x * HIST_TW, y0 = blockIdx.y * HIST_TH;
    auto cell_at = [&](int x, int y) -> int {
        int v = cellmap[(size_t)y * W + x];
        if (mask) v = min(v * (int)mask[(size_t)y * W + x], 255);   // _cellMap.mul(_mask), saturating
        return v;
    };
    for (int i = tid; i < HIST_TW * HIST_TH; i += 256) {
        const int x = x0 + (i % HIST_TW), y = y0 + i / HIST_TW;
        if (x < W && y < H) {
            const int v = cell_at(x, y);
            if (v) s_slot[v] = 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int v = 1; v < 256; v++) s_slot[v] = s_slot[v] ? (n < HIST_SLOTS ? n++ : HIST_SLOTS) : -1;
    }
    __syncthreads();
    for (int i = tid; i < HIST_TW * HIST_TH; i += 256) {
        const int x = x0 + (i % HIST_TW), y = y0 + i / HIST_TW;
        if (x >= W || y >= H) continue;
        const int v = cell_at(x, y);
        if (!v) continue;
        const int g = in[(size_t)y * stride + x];
        const int sl = s_slot[v];
        if (sl < HIST_SLOTS)
            atomicAdd(&s_h[sl * 256 + g], 1u);
        else
            atomicAdd(&raw[(size_t)(v - 1) * 256 + g], 1u);
    }
    __syncthreads();
    for (int v = 1; v < 256; v++) {
        const int sl = s_slot[v];
        if (sl < 0 || sl >= HIST_SLOTS) continue;
        const uint32_t cnt = s_h[sl * 256 + tid];
        if (cnt) atomicAdd(&raw[(size_t)(v - 1) * 256 + tid], cnt);
    }
}

void launch_chroma_hist(hipStream_t s, int W, int H, const uint8_t* in, size_t row_stride, const uint8_t* cellmap, const uint8_t* mask, uint32_t* raw) {
    hipLaunchKernelGGL(chroma_hist_kernel, dim3((W + HIST_TW - 1) / HIST_TW, (H + HIST_TH - 1) / HIST_TH), dim3(256), 0, s, W, H, in, row_stride,
                       cellmap, mask, raw);
}

// ---- EM: lane l holds grey levels 4l .. 4l+3. Every sum over the 256 levels is the lane's 4 terms in order, then a butterfly over
// the wave (xor 32, 16, .., 1): a fixed order, so the model is bit-reproducible (tests/chromatic_ref.py restates the same order).
__device__ __forceinline__ double em_sum(const double v[4]) {
    double s = v[0];
    s += v[1];
    s += v[2];
    s += v[3];
    return wave_sum_d<64>(s);
}

// log(pi N(v; mu, var)) of a component, -inf for a component without weight
__device__ __forceinline__ double em_logl(double v, double pi, double mu, double var) {
    if (!(pi > 0)) return -INFINITY;
    const double d = v - mu;
    return log(pi) - 0.5 * log(2.0 * M_PI * var) - d * d / (2.0 * var);
}

__global__ __launch_bounds__(64) void chroma_em_kernel(const uint32_t* raw, uint32_t min_raw, double thresh, uint32_t* hcount, int32_t* fitted,
                                                       double* prob, uint8_t* inside, int32_t* trained) {
    __shared__ uint32_t s_raw[256];
    __shared__ double s_c[256];
    __shared__ double s_init[6];
    const int cell = blockIdx.x, lane = threadIdx.x;
    const uint32_t* r = raw + (size_t)cell * 256;
    for (int j = 0; j < 4; j++) s_raw[lane + 64 * j] = r[lane + 64 * j];
    __syncthreads();
    double tmp[4];
    for (int j = 0; j < 4; j++) tmp[j] = (double)s_raw[4 * lane + j];
    const double nraw = em_sum(tmp);   // exact: integers
    if (min_raw > 0 && !(nraw > (double)min_raw)) {
        if (lane == 0) fitted[cell] = -1;
        return;
    }
    // the smoothed histogram (weights 3 / 2 / 1 at 0 / +-1 / +-2, nothing past 0 or 255): exact integers in double
    double h[4], c[4];
    for (int j = 0; j < 4; j++) {
        const int v = 4 * lane + j;
        uint64_t a = 3ull * s_raw[v];
        if (v > 0) a += 2ull * s_raw[v - 1];
        if (v < 255) a += 2ull * s_raw[v + 1];
        if (v > 1) a += s_raw[v - 2];
        if (v < 254) a += s_raw[v + 2];
        h[j] = (double)a;
    }
    const double hsum = em_sum(h);
    // histCount[v] = (unsigned)(200 * (hist[v] / sum)); a cell without samples has none (the reference divides 0 by 0 there)
    for (int j = 0; j < 4; j++) {
        c[j] = hsum > 0 ? (double)(uint32_t)(200.0 * (h[j] / hsum)) : 0.0;
        hcount[(size_t)cell * 256 + 4 * lane + j] = (uint32_t)c[j];
        s_c[4 * lane + j] = c[j];
    }
    const double N = em_sum(c);
    if (N < CHROMA_MIN_FIT) {   // EMClassifier::train returns and keeps its previous model
        if (lane == 0) fitted[cell] = 0;
        return;
    }
    __syncthreads();
    // start: the 2-means split with the least within-cluster sum of squares (S2 - S1^2 / S0 per side), ties to the lowest split
    if (lane == 0) {
        double T0 = 0, T1 = 0, T2 = 0;
        for (int v = 0; v < 256; v++) T0 += s_c[v], T1 += s_c[v] * v, T2 += s_c[v] * v * v;
        double A0 = 0, A1 = 0, A2 = 0, best = INFINITY, bA0 = 0, bA1 = 0;
        int split = -1;
        for (int v = 0; v < 255; v++) {
            A0 += s_c[v], A1 += s_c[v] * v, A2 += s_c[v] * v * v;
            const double B0 = T0 - A0, B1 = T1 - A1, B2 = T2 - A2;
            if (A0 > 0 && B0 > 0) {
                const double sse = (A2 - A1 * A1 / A0) + (B2 - B1 * B1 / B0);
                if (sse < best) best = sse, split = v, bA0 = A0, bA1 = A1;
            }
        }
        s_init[0] = split, s_init[1] = bA0 / T0, s_init[2] = (T0 - bA0) / T0;
        s_init[3] = bA1 / bA0, s_init[4] = (T1 - bA1) / (T0 - bA0), s_init[5] = T0 - bA0;
    }
    __syncthreads();
    const int split = (int)s_init[0];
    double pi[2] = {s_init[1], s_init[2]}, mu[2] = {s_init[3], s_init[4]}, var[2];
    {
        const double nk[2] = {N - s_init[5], s_init[5]};
        for (int k = 0; k < 2; k++) {
            for (int j = 0; j < 4; j++) {
                const int v = 4 * lane + j;
                const double d = v - mu[k];
                tmp[j] = ((v <= split) == (k == 0)) ? c[j] * d * d : 0.0;
            }
            var[k] = fmax(em_sum(tmp) / nk[k], DBL_EPSILON);
        }
    }
    // E, M three times: responsibilities in log space with the maximum subtracted, the M-step weighted by histCount
    for (int it = 0; it < 3; it++) {
        double rk[2][4];
        for (int j = 0; j < 4; j++) {
            const double v = 4 * lane + j;
            const double l0 = em_logl(v, pi[0], mu[0], var[0]), l1 = em_logl(v, pi[1], mu[1], var[1]);
            const double m = fmax(l0, l1);
            const double e0 = exp(l0 - m), e1 = exp(l1 - m), s = e0 + e1;
            rk[0][j] = e0 / s, rk[1][j] = e1 / s;
        }
        for (int k = 0; k < 2; k++) {
            double w[4], wv[4];
            for (int j = 0; j < 4; j++) w[j] = c[j] * rk[k][j], wv[j] = w[j] * (double)(4 * lane + j);
            const double W = em_sum(w), S = em_sum(wv);
            pi[k] = W / N;
            if (!(W > 0)) continue;   // no weight: mean and variance kept, the component contributes nothing
            mu[k] = S / W;
            for (int j = 0; j < 4; j++) {
                const double d = (double)(4 * lane + j) - mu[k];
                wv[j] = w[j] * d * d;
            }
            var[k] = fmax(em_sum(wv) / W, DBL_EPSILON);
        }
    }
    // _prob[v] = exp(log-likelihood(v)), _inside[v] = _prob[v] > threshProb
    for (int j = 0; j < 4; j++) {
        const int v = 4 * lane + j;
        const double l0 = em_logl(v, pi[0], mu[0], var[0]), l1 = em_logl(v, pi[1], mu[1], var[1]);
        const double m = fmax(l0, l1);
        const double p = exp(m + log(exp(l0 - m) + exp(l1 - m)));
        prob[(size_t)cell * 256 + v] = p;
        inside[(size_t)cell * 256 + v] = p > thresh ? 1 : 0;
    }
    if (lane == 0) fitted[cell] = 1, trained[cell] = 1;
}

void launch_chroma_em(hipStream_t s, int ncell, const uint32_t* raw, uint32_t min_raw, double thresh, uint32_t* hcount, int32_t* fitted,
                      double* prob, uint8_t* inside, int32_t* trained) {
    hipLaunchKernelGGL(chroma_em_kernel, dim3(ncell), dim3(64), 0, s, raw, min_raw, thresh, hcount, fitted, prob, inside, trained);
}

// ---- classification. A block owns a 64 x 16 tile of the mask (4 pixels per thread); it evaluates the sparse mask over the tile and a
// 2-pixel halo in LDS, dilates (tile + 1), erodes (tile). Outside the frame nothing dilates or erodes (OpenCV's default border).
// The model tables stay in global memory (L2): see DESIGN.md §5 for the measurement behind that.
constexpr int CL_TW = 64, CL_TH = 16;
// tiles down a column per block: classify2's dead tiles are only a store, 4 per block took 1024 1080p frames from 4.46 to 4.09 ms;
// classify evaluates every pixel and went from 11.0 to 12.0 ms with 4, so it keeps one
template <int METHOD>
constexpr int cl_tiles() { return METHOD == 2 ? 4 : 1; }

struct ClassifyArgs {
    int mc, nc, W, H;
    double thresh;
    const uint8_t* frames;
    size_t row_stride, frame_stride;
    const ChromaGeom* geom;
    const double* prob;     // [cell][256]
    const uint8_t* inside;  // [cell][256]
    uint8_t* masks;         // W x H per frame
    int32_t* npix;
};

// classify2 at one sample pixel (x, y): the float homography, the reciprocal in double stored to float, c = int(point + 0.5)
// (truncation toward zero: restated), the neighbour list of c weighted with the centres of the list ORDINALS (restated)
__device__ __forceinline__ uint8_t classify2_at(const ClassifyArgs& a, const float* Hf, int x, int y, int g) {
    const float fx = (float)(unsigned)x, fy = (float)(unsigned)y;
    const float inv = (float)(1. / (double)(fx * Hf[6] + fy * Hf[7] + Hf[8]));
    const float px = inv * (fx * Hf[0] + fy * Hf[1] + Hf[2]);
    const float py = inv * (fx * Hf[3] + fy * Hf[4] + Hf[5]);
    const double vx = (double)px + 0.5, vy = (double)py + 0.5;
    // c in [0, mc-1] x [0, nc-1]  <=>  point + 0.5 in (-1, mc) x (-1, nc); NaN and out-of-range values are skipped
    if (!(vx > -1.0 && vx < (double)a.mc && vy > -1.0 && vy < (double)a.nc)) return 0;
    const int cx = (int)vx, cy = (int)vy;
    // the reference's unsigned loops leave the lists of the first row and column empty: 0 / 0, never set
    if (cx == 0 || cy == 0) return 0;
    const int nb[4] = {(cy - 1) * a.mc + cx - 1, (cy - 1) * a.mc + cx, cy * a.mc + cx - 1, cy * a.mc + cx};
    float prob = 0.0f, totalW = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float ckx = (float)(k % a.mc) + 0.5f, cky = (float)(k / a.mc) + 0.5f;   // _centers[k]
        const float dist = fabsf(px - ckx) + fabsf(py - cky);
        float w = 2 - dist;
        w *= w;
        totalW += w;
        prob = (float)((double)prob + (double)w * a.prob[(size_t)nb[k] * 256 + g]);
    }
    prob /= totalW;
    return (double)prob > a.thresh ? 1 : 0;
}

template <int METHOD>
__global__ __launch_bounds__(256) void chroma_classify_kernel(ClassifyArgs a) {
    __shared__ uint8_t s_sp[CL_TH + 4][CL_TW + 4];
    __shared__ uint8_t s_d[CL_TH + 2][CL_TW + 2];
    __shared__ uint8_t s_cell[(CL_TH + 4) / 2][(CL_TW + 4) / 2];   // classify: the cell of each 2x2 block of the tile and halo
    __shared__ int s_cnt;
    const int f = blockIdx.z, tid = threadIdx.x;
    const int W = a.W, H = a.H;
    const ChromaGeom* g = a.geom + f;
    const int rx0 = g->rx0, ry0 = g->ry0, rx1 = g->rx1, ry1 = g->ry1;
    const bool valid = g->valid != 0;
    const uint8_t* in = a.frames + (size_t)f * a.frame_stride;
    float Hf[9];
    if (METHOD == 2)
        for (int i = 0; i < 9; i++) Hf[i] = (float)g->Hc[i];   // _perpTrans.convertTo(pT_32, CV_32F)
    const int W2 = W & ~1, H2 = H & ~1;
    const int x0 = blockIdx.x * CL_TW;
    const int tx = (tid % (CL_TW / 4)) * 4, ty = tid / (CL_TW / 4);
    const int ox = x0 + tx;
    const bool wide = (W & 3) == 0 && ((uintptr_t)a.masks & 3) == 0;
    if (tid == 0) s_cnt = 0;
    int ones = 0;
    for (int t = 0; t < cl_tiles<METHOD>(); t++) {
        const int y0 = (blockIdx.y * cl_tiles<METHOD>() + t) * CL_TH;
        if (y0 >= H) break;
        const int oy = y0 + ty;
        uint8_t* mrow = a.masks + (size_t)f * W * H + (size_t)oy * W;
        auto store = [&](const uint8_t v[4]) {
            if (oy >= H) return;
            if (wide && ox + 3 < W)
                *(uint32_t*)(mrow + ox) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
            else
                for (int k = 0; k < 4; k++)
                    if (ox + k < W) mrow[ox + k] = v[k];
        };
        bool live = valid;
        if (METHOD == 2) live = live && x0 - 2 < rx1 && x0 + CL_TW + 2 > rx0 && y0 - 2 < ry1 && y0 + CL_TH + 2 > ry0;
        if (!live) {   // uniform over the block: no pose, or the tile is out of classify2's reach
            const uint8_t z[4] = {0, 0, 0, 0};
            store(z);
            continue;
        }
        if (METHOD == 1) {   // one transform per 2x2 block (x0 - 2 and y0 - 2 are even: the halo starts on a block)
            for (int i = tid; i < (CL_TH + 4) / 2 * ((CL_TW + 4) / 2); i += 256) {
                const int by = i / ((CL_TW + 4) / 2), bx = i - by * ((CL_TW + 4) / 2);
                const int x = x0 - 2 + 2 * bx, y = y0 - 2 + 2 * by;
                s_cell[by][bx] = (x >= 0 && y >= 0 && x < W2 && y < H2) ? (uint8_t)chroma_cell(g->Ht, x, y, a.mc, a.nc) : 0;
            }
            __syncthreads();
        }
        for (int i = tid; i < (CL_TH + 4) * (CL_TW + 4); i += 256) {
            const int ly = i / (CL_TW + 4), lx = i - ly * (CL_TW + 4);
            const int x = x0 - 2 + lx, y = y0 - 2 + ly;
            uint8_t v = 0;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                if (METHOD == 1) {
                    const int cm = s_cell[ly >> 1][lx >> 1];
                    if (cm) v = a.inside[(size_t)(cm - 1) * 256 + in[(size_t)y * a.row_stride + x]];
                } else if (y >= ry0 && y < ry1 && ((y - ry0) & 1) == 0) {
                    const int sx = rx0 + (((y - ry0) >> 1) & 1);   // rows alternate their first column
                    if (x >= sx && x < rx1 && ((x - sx) & 1) == 0) v = classify2_at(a, Hf, x, y, in[(size_t)y * a.row_stride + x]);
                }
            }
            s_sp[ly][lx] = v;
        }
        __syncthreads();
        for (int i = tid; i < (CL_TH + 2) * (CL_TW + 2); i += 256) {   // dilate; outside the frame: 1, neutral for the erosion
            const int ly = i / (CL_TW + 2), lx = i - ly * (CL_TW + 2);
            const int x = x0 - 1 + lx, y = y0 - 1 + ly;
            uint8_t v = 1;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                v = 0;
                for (int dy = 0; dy < 3; dy++)
                    for (int dx = 0; dx < 3; dx++) v |= s_sp[ly + dy][lx + dx];
            }
            s_d[ly][lx] = v;
        }
        __syncthreads();
        uint8_t o[4];
        for (int k = 0; k < 4; k++) {
            uint8_t v = 1;
            for (int dy = 0; dy < 3; dy++)
                for (int dx = 0; dx < 3; dx++) v &= s_d[ty + dy][tx + k + dx];
            o[k] = v;
            ones += (v && ox + k < W && oy < H) ? 1 : 0;
        }
        store(o);
        // the next tile's first phase writes only s_sp, which nobody reads after the second barrier
    }
    if (a.npix) {
        for (int off = 32; off > 0; off >>= 1) ones += __shfl_xor(ones, off, 64);
        __syncthreads();
        if ((tid & 63) == 0 && ones) atomicAdd(&s_cnt, ones);
        __syncthreads();
        if (tid == 0 && s_cnt) atomicAdd(&a.npix[f], s_cnt);
    }
}

void launch_chroma_classify(hipStream_t s, const ChromaCam& c, int method, double thresh, int nframes, const uint8_t* frames, size_t row_stride,
                            size_t frame_stride, const ChromaGeom* geom, const double* prob, const uint8_t* inside, uint8_t* masks, int32_t* npix) {
    ClassifyArgs a;
    a.mc = c.mc, a.nc = c.nc, a.W = c.W, a.H = c.H, a.thresh = thresh;
    a.frames = frames, a.row_stride = row_stride, a.frame_stride = frame_stride;
    a.geom = geom, a.prob = prob, a.inside = inside, a.masks = masks, a.npix = npix;
    const int rows = CL_TH * (method == 1 ? cl_tiles<1>() : cl_tiles<2>());
    const dim3 grid((c.W + CL_TW - 1) / CL_TW, (c.H + rows - 1) / rows, nframes);
    if (method == 1)
        hipLaunchKernelGGL(chroma_classify_kernel<1>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(chroma_classify_kernel<2>, grid, dim3(256), 0, s, a);
}

}  // namespace ah
