// Image pyramid of MarkerDetector::pyrDown(level): cv::pyrDown for 8-bit single-channel frames, and the lift that brings what the
// rectangle stage found on the reduced image back to full-frame coordinates.
//
// pyr_down_kernel restates cv::pyrDown as an exact integer definition (OpenCV's documentation: the 5x5 kernel {1,4,6,4,1}^2 / 256,
// BORDER_REFLECT_101, every second row and column, rounded to nearest):
//   Wo = (W + 1) / 2, Ho = (H + 1) / 2
//   R(p, n): n == 1 -> 0; otherwise reflect p at 0 and n - 1 until 0 <= p < n
//   h(y, xo)    = sum_t k[t] * src(y, R(2 xo - 2 + t, W))
//   dst(yo, xo) = (sum_t k[t] * h(R(2 yo - 2 + t, H), xo) + 128) >> 8
//
// A streaming stencil like the threshold pass (k_threshold.hip): a lane owns four adjacent output pixels, per source row it reads its
// eight source bytes with one 8-byte load and takes the two bytes to its left and the one to its right from the neighbouring lanes (DPP
// wave shifts), forms the four horizontal sums as two dwords of 16-bit pairs (a sum is at most 16 * 255) and keeps the sums of the last
// five source rows in registers while it walks down a strip of output rows. The vertical sum of a pair stays below 2^16 per half
// (256 * 255 + 128), so it is packed arithmetic as well. Lanes whose bytes leave the row, the first and last lane of a wave, and
// frames whose rows are not 8-byte aligned read single bytes through R.
#include "internal.h"

namespace ah {

__host__ __device__ inline int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

struct PyrArgs {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_row, src_frame, dst_row, dst_frame;
    int W, H, Wo, Ho;
    int strip;       // output rows per workgroup
    int src_vec;     // rows of src are 8-byte aligned: 8-byte loads
    int dst_vec;     // rows of dst are 4-byte aligned: dword stores
};

// the eight bytes of a lane and, on the first / last lane of a wave, the bytes it cannot take from a neighbour
struct PyrRow {
    uint32_t d0, d1, el, er;
};

__global__ __launch_bounds__(256) void pyr_down_kernel(PyrArgs a) {
    const int lane = threadIdx.x & 63;
    const int L = blockIdx.x * 256 + threadIdx.x;   // lane along the row: source columns 8L .. 8L+7, output columns 4L .. 4L+3
    const int x0 = 8 * L;
    if (4 * (L - lane) >= a.Wo) return;             // the whole wave lies right of the image
    const int yo0 = blockIdx.y * a.strip, yo1 = min(yo0 + a.strip, a.Ho);
    const uint8_t* src = a.src + (size_t)blockIdx.z * a.src_frame;
    uint8_t* dst = a.dst + (size_t)blockIdx.z * a.dst_frame;
    const int W = a.W, H = a.H;
    const bool out_lane = 4 * L < a.Wo;
    const bool fast = a.src_vec && x0 + 8 <= W;
    const bool live = x0 < W + 8;                   // some lane may ask for one of these bytes (byte 0 of the lane right of the last output lane)
    // column of byte j on the slow path, and of the edge bytes
    int xc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) xc[j] = (!fast && live) ? reflect101(x0 + j, W) : 0;
    const bool edge_l = lane == 0 && out_lane, edge_r = lane == 63 && out_lane;
    const int xl2 = edge_l ? reflect101(x0 - 2, W) : 0, xl1 = edge_l ? reflect101(x0 - 1, W) : 0, xr = edge_r ? reflect101(x0 + 8, W) : 0;

    auto load_row = [&](int v) -> PyrRow {   // v: virtual row, reflected here
        const uint8_t* row = src + (size_t)reflect101(v, H) * a.src_row;
        PyrRow r;
        r.d0 = r.d1 = r.el = r.er = 0;
        if (fast) {
            const uint2 d = *(const uint2*)(row + x0);
            r.d0 = d.x, r.d1 = d.y;
        } else if (live) {
            r.d0 = (uint32_t)row[xc[0]] | ((uint32_t)row[xc[1]] << 8) | ((uint32_t)row[xc[2]] << 16) | ((uint32_t)row[xc[3]] << 24);
            r.d1 = (uint32_t)row[xc[4]] | ((uint32_t)row[xc[5]] << 8) | ((uint32_t)row[xc[6]] << 16) | ((uint32_t)row[xc[7]] << 24);
        }
        if (edge_l) r.el = ((uint32_t)row[xl2] << 16) | ((uint32_t)row[xl1] << 24);
        if (edge_r) r.er = (uint32_t)row[xr];
        return r;
    };
    // horizontal sums of one row: h01 = h(4L) | h(4L+1) << 16, h23 = h(4L+2) | h(4L+3) << 16
    auto hsum = [&](const PyrRow& r, uint32_t& h01, uint32_t& h23) {
        const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp((int)r.el, (int)r.d1, 0x138, 0xF, 0xF, false);    // lane - 1: bytes -4 .. -1
        const uint32_t right = (uint32_t)__builtin_amdgcn_update_dpp((int)r.er, (int)r.d0, 0x130, 0xF, 0xF, false);   // lane + 1: bytes 8 .. 11
        // pairs of bytes (i, i + 2) as 16-bit halves
        const uint32_t em = __builtin_amdgcn_perm(r.d0, left, 0x0C040C02u);    // -2, 0
        const uint32_t om = __builtin_amdgcn_perm(r.d0, left, 0x0C050C03u);    // -1, 1
        const uint32_t e01 = __builtin_amdgcn_perm(0u, r.d0, 0x0C020C00u);     //  0, 2
        const uint32_t o01 = __builtin_amdgcn_perm(0u, r.d0, 0x0C030C01u);     //  1, 3
        const uint32_t e12 = __builtin_amdgcn_perm(r.d1, r.d0, 0x0C040C02u);   //  2, 4
        const uint32_t o12 = __builtin_amdgcn_perm(r.d1, r.d0, 0x0C050C03u);   //  3, 5
        const uint32_t e23 = __builtin_amdgcn_perm(0u, r.d1, 0x0C020C00u);     //  4, 6
        const uint32_t o23 = __builtin_amdgcn_perm(0u, r.d1, 0x0C030C01u);     //  5, 7
        const uint32_t e34 = __builtin_amdgcn_perm(right, r.d1, 0x0C040C02u);  //  6, 8
        h01 = em + e12 + 6u * e01 + 4u * (om + o01);
        h23 = e12 + e34 + 6u * e23 + 4u * (o12 + o23);
    };

    // window of the horizontal sums of virtual rows 2 yo - 2 .. 2 yo + 2: A B C are carried, D E enter with every output row
    uint32_t A01, A23, B01, B23, C01, C23;
    {
        const PyrRow ra = load_row(2 * yo0 - 2), rb = load_row(2 * yo0 - 1), rc = load_row(2 * yo0);
        hsum(ra, A01, A23), hsum(rb, B01, B23), hsum(rc, C01, C23);
    }
    PyrRow nd = load_row(2 * yo0 + 1), ne = load_row(2 * yo0 + 2);
    for (int yo = yo0; yo < yo1; yo++) {
        const PyrRow rd = nd, re = ne;
        if (yo + 1 < yo1) nd = load_row(2 * yo + 3), ne = load_row(2 * yo + 4);   // the next output row's loads fly during this one's sums
        uint32_t D01, D23, E01, E23;
        hsum(rd, D01, D23), hsum(re, E01, E23);
        const uint32_t v01 = A01 + E01 + 4u * (B01 + D01) + 6u * C01 + 0x00800080u;
        const uint32_t v23 = A23 + E23 + 4u * (B23 + D23) + 6u * C23 + 0x00800080u;
        const uint32_t o4 = __builtin_amdgcn_perm(v23, v01, 0x07050301u);   // the high byte of every half
        if (out_lane) {
            uint8_t* orow = dst + (size_t)yo * a.dst_row + 4 * L;
            if (a.dst_vec && 4 * L + 4 <= a.Wo) {
                __builtin_nontemporal_store(o4, (uint32_t*)orow);
            } else {
                for (int j = 0; j < 4 && 4 * L + j < a.Wo; j++) orow[j] = (uint8_t)(o4 >> (8 * j));
            }
        }
        A01 = C01, A23 = C23, B01 = D01, B23 = D23, C01 = E01, C23 = E23;
    }
}

void launch_pyr_down(hipStream_t s, const uint8_t* src, size_t src_row, size_t src_frame, int W, int H, int nframes, uint8_t* dst, size_t dst_row,
                     size_t dst_frame) {
    PyrArgs a;
    a.src = src, a.dst = dst, a.src_row = src_row, a.src_frame = src_frame, a.dst_row = dst_row, a.dst_frame = dst_frame;
    a.W = W, a.H = H, a.Wo = (W + 1) / 2, a.Ho = (H + 1) / 2;
    a.src_vec = ((uintptr_t)src % 8 == 0 && src_row % 8 == 0 && src_frame % 8 == 0) ? 1 : 0;
    a.dst_vec = ((uintptr_t)dst % 4 == 0 && dst_row % 4 == 0 && dst_frame % 4 == 0) ? 1 : 0;
    const int gx = ((a.Wo + 3) / 4 + 255) / 256;
    // 16 output rows per workgroup read 35 source rows for 32 (the three shared rows come from the L2): a 1080p batch of a few frames already has
    // thousands of waves then. Few frames take shorter strips, so that one frame still spreads over the chip.
    a.strip = (size_t)gx * ((a.Ho + 15) / 16) * nframes >= 1024 ? 16 : 4;
    const int gy = (a.Ho + a.strip - 1) / a.strip;
    for (int f0 = 0; f0 < nframes; f0 += 65535) {   // grid.z holds at most 65535 frames
        const int nf = nframes - f0 < 65535 ? nframes - f0 : 65535;
        PyrArgs c = a;
        c.src = src + (size_t)f0 * src_frame, c.dst = dst + (size_t)f0 * dst_frame;
        hipLaunchKernelGGL(pyr_down_kernel, dim3(gx, gy, nf), dim3(256), 0, s, c);
    }
}

// ---------------------------------------------------------------------------------------------
// Lift: everything the rectangle stage left in reduced-image coordinates times s = 1 << shift, in place. Workgroups [0, 2 * nplanes): the
// eight waves of a plane share its kept borders (the list from slot 0 upwards and the late list from the top of the plane's array downwards),
// one wave per border: every point in the pool and the descriptor's start pixel. The workgroups behind them: one lane per candidate slot,
// its integer quad and its corners. Full-frame coordinates are at most 16383, so the 16-bit fields hold them.
// ---------------------------------------------------------------------------------------------
struct LiftArgs {
    ContourDesc* cdesc;
    short2* pool;
    const uint32_t* trig_cnt;
    Cand* cands;
    const int32_t* ncands;
    uint32_t cap_cdesc;
    int cap_cands, nplanes, nframes, shift;
};

constexpr int LIFT_WAVES = 8;   // per plane, in two workgroups of 256

__global__ __launch_bounds__(256) void lift_contours_kernel(LiftArgs a) {
    const int nborder_blocks = 2 * a.nplanes;
    if ((int)blockIdx.x < nborder_blocks) {
        const int plane = blockIdx.x >> 1, lane = threadIdx.x & 63;
        const uint32_t w = (blockIdx.x & 1) * 4 + (threadIdx.x >> 6);
        const uint32_t n = min(a.trig_cnt[(size_t)plane * TRIG_CNT_STRIDE + TC_CDESC], a.cap_cdesc);
        const uint32_t nlate = min(a.trig_cnt[(size_t)plane * TRIG_CNT_STRIDE + TC_LATE], a.cap_cdesc - n);
        ContourDesc* base = a.cdesc + (size_t)plane * a.cap_cdesc;
        for (uint32_t i = w; i < n + nlate; i += LIFT_WAVES) {
            ContourDesc* cd = base + (i < n ? i : a.cap_cdesc - 1u - (i - n));
            const int cnt = cd->n;
            short2* P = a.pool + cd->pool_off;
            for (int j = lane; j < cnt; j += WAVE) {
                short2 p = P[j];
                p.x = (short)(p.x << a.shift), p.y = (short)(p.y << a.shift);
                P[j] = p;
            }
            if (lane == 0 && cnt > 0) cd->x0 = (int16_t)(cd->x0 << a.shift), cd->y0 = (int16_t)(cd->y0 << a.shift);
        }
        return;
    }
    const int gid = ((int)blockIdx.x - nborder_blocks) * 256 + threadIdx.x;
    const int frame = gid / a.cap_cands, i = gid - frame * a.cap_cands;
    if (frame >= a.nframes || i >= min(a.ncands[frame], a.cap_cands)) return;
    Cand* c = a.cands + (size_t)frame * a.cap_cands + i;
    const float sf = (float)(1 << a.shift);
    for (int k = 0; k < 4; k++) c->qx[k] = (int16_t)(c->qx[k] << a.shift), c->qy[k] = (int16_t)(c->qy[k] << a.shift);
    for (int k = 0; k < 8; k++) c->c[k] *= sf;
}

void launch_lift(hipStream_t s, int nframes, const DetectParams& p, const Buffers& b) {
    LiftArgs a;
    a.cdesc = b.cdesc, a.pool = b.pool, a.trig_cnt = b.trig_cnt, a.cands = b.cands, a.ncands = b.ncands;
    a.cap_cdesc = b.cap_cdesc, a.cap_cands = b.cap_cands, a.nplanes = nframes * p.nthr, a.nframes = nframes, a.shift = p.pyr;
    const int cand_blocks = (nframes * b.cap_cands + 255) / 256;
    hipLaunchKernelGGL(lift_contours_kernel, dim3(2 * a.nplanes + cand_blocks), dim3(256), 0, s, a);
}

}  // namespace ah
