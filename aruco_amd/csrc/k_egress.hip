// Frames out (include/arucohip.h, "Frames out"): the 8-bit grey or interleaved B,G,R frames the library produces, turned into what an
// encoder (NV12), a capture sink (YUYV / UYVY) or a display (BGRA / RGBA) takes. The mirror of k_ingest.hip; no reference counterpart.
//
// A streaming kernel of ingest_kernel's shape: a lane turns 4 pixels of one row, block y is the row, block z the frame. For NV12 a lane owns
// a 4 x 2 block and block y is the row pair: two rows of source dwords in, one Y dword per row and one chroma dword (U V of the left 2 x 2
// block, U V of the right one) out. A quad whose source and destination dwords are whole and aligned moves as dwords; any other quad
// (unaligned base, stride or chroma offset, the last pixels of a row) fills the same little-endian words and moves byte by byte, so every
// definition below is written once, on words.
// Two instances restate work that exists elsewhere, as in k_ingest.hip: B,G,R to GRAY8 is bgr2gray_kernel's arithmetic (gray_of of
// convert_device.h) and grey to GRAY8 / B,G,R to BGR8 are 2-D copies; they are here so that every destination has the same strides.
#include "convert_device.h"   // gray_of, ld32, byte_of
#include "internal.h"

namespace ah {

struct EgressArgs {
    const uint8_t* src;
    size_t srs, sfs;
    uint8_t* dst;
    size_t drs, dfs, chroma_offset;
    int width, height;
    int p0;     // PACKED: 1 when the first byte is R; YUV422: byte of Y0 (0 YUYV, 1 UYVY)
    int luma;   // a grey source is Y already (ARUCOHIP_EXPORT_GREY_IS_LUMA)
    int fast;
};

enum EgressKind { EK_GRAY8 = 0, EK_PACKED3, EK_PACKED4, EK_YUV422, EK_NV12 };

// the low nbytes bytes of the little-endian word v to p; whole: p is dword aligned and all four bytes are the row's
__device__ __forceinline__ void st32(uint8_t* p, uint32_t v, int nbytes, bool whole) {
    if (whole) {
        *(uint32_t*)p = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < nbytes) p[j] = (uint8_t)(v >> (8 * j));
}

// BT.601 video range in 20-bit fixed point, round(c * 2^20 / 255) of the standard matrix; the luma row sums to 900542, both chroma rows to 0
__device__ __forceinline__ uint32_t luma_of(uint32_t b, uint32_t g, uint32_t r) {
    return (269262u * r + 528618u * g + 102662u * b + (16u << 20) + (1u << 19)) >> 20;
}
// U | V << 8 of the channel sums over 2^K pixels (the box filter); every sum is non-negative and below 2^30
template <int K>
__device__ __forceinline__ uint32_t chroma_of(int sb, int sg, int sr) {
    constexpr int bias = (128 << (20 + K)) + (1 << (19 + K));
    const int u = (-155424 * sr - 305127 * sg + 460551 * sb + bias) >> (20 + K);
    const int v = (460551 * sr - 385654 * sg - 74897 * sb + bias) >> (20 + K);
    return (uint32_t)u | ((uint32_t)v << 8);
}

// Pixels x .. x + 3 of the source row (n of them exist; the others read as 0). C = 1: the grey value in all three.
template <int C>
__device__ __forceinline__ void src_quad(const uint8_t* row, int x, int n, bool whole, uint32_t* b, uint32_t* g, uint32_t* r) {
    uint32_t w[C];
#pragma unroll
    for (int k = 0; k < C; k++) w[k] = ld32(row + (size_t)x * C + 4 * k, n * C - 4 * k, whole);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (C == 1)
            b[j] = g[j] = r[j] = byte_of(w, j);
        else
            b[j] = byte_of(w, 3 * j), g[j] = byte_of(w, 3 * j + 1), r[j] = byte_of(w, 3 * j + 2);
    }
}

// the Y bytes of a quad as one word
template <int C>
__device__ __forceinline__ uint32_t luma_word(const EgressArgs& a, const uint32_t* b, const uint32_t* g, const uint32_t* r) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) w |= (C == 1 && a.luma ? b[j] : luma_of(b[j], g[j], r[j])) << (8 * j);
    return w;
}

template <int KIND, int C>
__global__ __launch_bounds__(256) void egress_kernel(EgressArgs a) {
    constexpr int ROWS = KIND == EK_NV12 ? 2 : 1;
    const int frame = blockIdx.z, y = blockIdx.y * ROWS;
    const uint8_t* srow = a.src + (size_t)frame * a.sfs + (size_t)y * a.srs;
    uint8_t* df = a.dst + (size_t)frame * a.dfs;
    uint8_t* drow = df + (size_t)y * a.drs;
    const int quads = (a.width + 3) / 4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const int x = 4 * q, n = min(4, a.width - x);
        const bool whole = a.fast && n == 4;   // source and destination start on dword boundaries and the quad is complete
        uint32_t b[4], g[4], r[4];
        if (KIND == EK_NV12) {
            int sb[2] = {0, 0}, sg[2] = {0, 0}, sr[2] = {0, 0};   // channel sums of the left and the right 2 x 2 block
#pragma unroll
            for (int i = 0; i < 2; i++) {
                src_quad<C>(srow + (size_t)i * a.srs, x, n, whole, b, g, r);
                st32(drow + (size_t)i * a.drs + x, luma_word<C>(a, b, g, r), n, whole);
                if (C == 3) {
#pragma unroll
                    for (int j = 0; j < 4; j++) sb[j >> 1] += (int)b[j], sg[j >> 1] += (int)g[j], sr[j >> 1] += (int)r[j];
                }
            }
            const uint32_t wc = C == 1 ? 0x80808080u : chroma_of<2>(sb[0], sg[0], sr[0]) | (chroma_of<2>(sb[1], sg[1], sr[1]) << 16);
            st32(df + a.chroma_offset + (size_t)blockIdx.y * a.drs + x, wc, n, whole);
        } else {
            constexpr int BPP = KIND == EK_GRAY8 ? 1 : KIND == EK_PACKED3 ? 3 : KIND == EK_PACKED4 ? 4 : 2;
            uint32_t w[4];   // the quad's 4 * BPP destination bytes: BPP words
            src_quad<C>(srow, x, n, whole, b, g, r);
            if (KIND == EK_GRAY8) {
                w[0] = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) w[0] |= (C == 1 ? b[j] : gray_of(b[j], g[j], r[j])) << (8 * j);
            } else if (KIND == EK_PACKED3 || KIND == EK_PACKED4) {
                uint32_t c0[4], c2[4];   // the pixel's first and third byte
#pragma unroll
                for (int j = 0; j < 4; j++) c0[j] = a.p0 ? r[j] : b[j], c2[j] = a.p0 ? b[j] : r[j];
                if (KIND == EK_PACKED3) {   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                    w[0] = c0[0] | (g[0] << 8) | (c2[0] << 16) | (c0[1] << 24);
                    w[1] = g[1] | (c2[1] << 8) | (c0[2] << 16) | (g[2] << 24);
                    w[2] = c2[2] | (c0[3] << 8) | (g[3] << 16) | (c2[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) w[j] = c0[j] | (g[j] << 8) | (c2[j] << 16) | 0xFF000000u;
                }
            } else {   // EK_YUV422
                const uint32_t wy = luma_word<C>(a, b, g, r);
                const int ys = 8 * a.p0, us = 8 * (1 - a.p0), vs = 8 * (3 - a.p0);   // bit positions of Y0, U, V in a pair's word; Y1 is 16 above Y0
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int j = 2 * k;
                    const uint32_t uv = C == 1 ? 0x8080u : chroma_of<1>((int)(b[j] + b[j + 1]), (int)(g[j] + g[j + 1]), (int)(r[j] + r[j + 1]));
                    w[k] = (byte_of(&wy, j) << ys) | (byte_of(&wy, j + 1) << (ys + 16)) | ((uv & 0xFFu) << us) | ((uv >> 8) << vs);
                }
            }
#pragma unroll
            for (int k = 0; k < BPP; k++) st32(drow + (size_t)x * BPP + 4 * k, w[k], n * BPP - 4 * k, whole);
        }
    }
}

template <int KIND>
static void launch_kind(hipStream_t s, const EgressArgs& a, int nframes, int C) {
    const int quads = (a.width + 3) / 4;
    dim3 grid((quads + 255) / 256, KIND == EK_NV12 ? a.height / 2 : a.height, nframes);
    if (C == 1)
        hipLaunchKernelGGL((egress_kernel<KIND, 1>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((egress_kernel<KIND, 3>), grid, dim3(256), 0, s, a);
}

// the caller has validated fmt, the geometry and the strides (capi_egress.hip)
void launch_egress(hipStream_t s, const uint8_t* src, int src_channels, size_t src_row_stride, size_t src_frame_stride, int width, int height, int nframes,
                   const FrameFmt& fmt, bool grey_is_luma, uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride) {
    EgressArgs a{};
    a.src = src, a.srs = src_row_stride, a.sfs = src_frame_stride;
    a.dst = dst, a.drs = dst_row_stride, a.dfs = dst_frame_stride;
    a.chroma_offset = fmt.chroma_offset ? fmt.chroma_offset : dst_row_stride * (size_t)height;
    a.width = width, a.height = height, a.luma = grey_is_luma;
    // what decides the dword path: only strides and offsets the kernel uses (one frame: no frame stride; the chroma offset only for NV12)
    size_t align = (uintptr_t)src | src_row_stride | (uintptr_t)dst | dst_row_stride;
    if (nframes > 1) align |= src_frame_stride | dst_frame_stride;
    if (fmt.format == ARUCOHIP_PIX_NV12) align |= a.chroma_offset;
    a.fast = (align & 3) == 0;
    switch (fmt.format) {
        case ARUCOHIP_PIX_GRAY8: launch_kind<EK_GRAY8>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_BGR8: launch_kind<EK_PACKED3>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_RGB8: a.p0 = 1; launch_kind<EK_PACKED3>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_BGRA8: launch_kind<EK_PACKED4>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_RGBA8: a.p0 = 1; launch_kind<EK_PACKED4>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_YUYV: launch_kind<EK_YUV422>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_UYVY: a.p0 = 1; launch_kind<EK_YUV422>(s, a, nframes, src_channels); break;
        case ARUCOHIP_PIX_NV12: launch_kind<EK_NV12>(s, a, nframes, src_channels); break;
        default: break;
    }
}

}  // namespace ah
