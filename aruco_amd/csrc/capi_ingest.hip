// Host side of the camera-native input stage (k_ingest.hip): the formats' arithmetic, the argument checks and the conversion as a stage of
// its own. The detection entry points are untouched: a caller converts to grey on the device and hands arucohip_detect_batch the result.
#include <hip/hip_runtime.h>

#include "handle.h"

namespace {

bool is_bayer(int f) { return f >= ARUCOHIP_PIX_BAYER_RGGB && f <= ARUCOHIP_PIX_BAYER_GBRG; }
bool is_yuv(int f) { return f == ARUCOHIP_PIX_YUYV || f == ARUCOHIP_PIX_UYVY || f == ARUCOHIP_PIX_NV12; }

// the bytes of a row that are read (0: invalid format, bits or width)
size_t frame_min_row_stride(const FrameFmt& fmt, int W) {
    if (W < 1) return 0;
    switch (fmt.format) {
        case ARUCOHIP_PIX_GRAY8: return (size_t)W;
        case ARUCOHIP_PIX_BGR8:
        case ARUCOHIP_PIX_RGB8: return (size_t)W * 3;
        case ARUCOHIP_PIX_BGRA8:
        case ARUCOHIP_PIX_RGBA8: return (size_t)W * 4;
        case ARUCOHIP_PIX_GRAY16: return fmt.bits >= 8 && fmt.bits <= 16 ? (size_t)W * 2 : 0;
        case ARUCOHIP_PIX_YUYV:
        case ARUCOHIP_PIX_UYVY: return W % 2 == 0 ? (size_t)W * 2 : 0;
        case ARUCOHIP_PIX_NV12: return W % 2 == 0 ? (size_t)W : 0;
        default: return is_bayer(fmt.format) && W >= 2 ? (size_t)W : 0;
    }
}

// the bytes of a frame from its first to its last byte read (0: invalid)
size_t frame_min_stride(const FrameFmt& fmt, int W, int H, size_t row_stride) {
    const size_t row = frame_min_row_stride(fmt, W);
    if (!row || H < 1 || row_stride < row) return 0;
    if (is_bayer(fmt.format) && H < 2) return 0;
    if (fmt.format != ARUCOHIP_PIX_NV12) return row_stride * (size_t)(H - 1) + row;
    if (H % 2) return 0;
    const size_t luma = row_stride * (size_t)H;
    if (fmt.chroma_offset && fmt.chroma_offset < luma) return 0;
    return (fmt.chroma_offset ? fmt.chroma_offset : luma) + row_stride * (size_t)(H / 2 - 1) + row;
}

}  // namespace

// the caller's record as the host code carries it; bits and chroma_offset only where the format has them
int take_format(arucohip_handle* h, const arucohip_frame_format_t* fmt, FrameFmt* f) {
    if (!fmt) return fail(h, ARUCOHIP_E_INVALID, "frame format: fmt is NULL");
    f->format = fmt->format;
    f->bits = fmt->format == ARUCOHIP_PIX_GRAY16 ? fmt->bits : 0;
    f->chroma_offset = fmt->format == ARUCOHIP_PIX_NV12 ? (size_t)fmt->chroma_offset : 0;
    return ARUCOHIP_OK;
}

// a format against a geometry, with the limits of the detection calls (check_geometry of capi.hip): one message per refusal
int check_frame_format(arucohip_handle* h, const FrameFmt& fmt, int nframes, int W, int H, size_t row_stride, size_t frame_stride) {
    if (fmt.format < ARUCOHIP_PIX_GRAY8 || fmt.format > ARUCOHIP_PIX_BAYER_GBRG) return fail(h, ARUCOHIP_E_INVALID, "frame format: unknown pixel format");
    if (fmt.format == ARUCOHIP_PIX_GRAY16 && (fmt.bits < 8 || fmt.bits > 16)) return fail(h, ARUCOHIP_E_INVALID, "frame format: GRAY16 bits outside 8..16");
    if (nframes < 1 || nframes > h->lim.max_batch) return fail(h, ARUCOHIP_E_INVALID, "nframes outside 1..max_batch");
    if (W < 1 || H < 1 || W > h->lim.max_width || H > h->lim.max_height) return fail(h, ARUCOHIP_E_INVALID, "frame wider or taller than the handle was created for");
    if (is_yuv(fmt.format) && W % 2) return fail(h, ARUCOHIP_E_INVALID, "frame format: YUYV / UYVY / NV12 need an even width");
    if (fmt.format == ARUCOHIP_PIX_NV12 && H % 2) return fail(h, ARUCOHIP_E_INVALID, "frame format: NV12 needs an even height");
    if (is_bayer(fmt.format) && (W < 2 || H < 2)) return fail(h, ARUCOHIP_E_INVALID, "frame format: a Bayer frame is at least 2 x 2");
    if (row_stride < frame_min_row_stride(fmt, W)) return fail(h, ARUCOHIP_E_INVALID, "frame format: row_stride below the format's row bytes");
    if (fmt.format == ARUCOHIP_PIX_NV12 && fmt.chroma_offset && fmt.chroma_offset < row_stride * (size_t)H)
        return fail(h, ARUCOHIP_E_INVALID, "frame format: NV12 chroma_offset inside the Y plane");
    const size_t need = frame_min_stride(fmt, W, H, row_stride);
    if (!need) return fail(h, ARUCOHIP_E_INVALID, "frame format: invalid geometry");
    if (nframes > 1 && frame_stride < need) return fail(h, ARUCOHIP_E_INVALID, "frame format: frame_stride does not cover a frame");
    return ARUCOHIP_OK;
}

extern "C" {

size_t arucohip_frame_min_row_stride(const arucohip_frame_format_t* fmt, int width) {
    FrameFmt f;
    if (take_format(nullptr, fmt, &f)) return 0;
    return frame_min_row_stride(f, width);
}

size_t arucohip_frame_min_stride(const arucohip_frame_format_t* fmt, int width, int height, size_t row_stride) {
    FrameFmt f;
    if (take_format(nullptr, fmt, &f)) return 0;
    return frame_min_stride(f, width, height, row_stride);
}

int arucohip_convert_batch(arucohip_handle* h, const void* src_, const arucohip_frame_format_t* fmt, int nframes, int W, int H, size_t row_stride,
                           size_t frame_stride, int src_on_device, int C, uint8_t* dst, size_t drs, size_t dfs, int dst_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    const uint8_t* src = (const uint8_t*)src_;
    if (!src || !dst) return fail(h, ARUCOHIP_E_INVALID, "convert: src or dst is NULL");
    FrameFmt f;
    int rc = take_format(h, fmt, &f);
    if (rc) return rc;
    if ((rc = check_frame_format(h, f, nframes, W, H, row_stride, frame_stride))) return rc;
    if (C != 1 && C != 3) return fail(h, ARUCOHIP_E_INVALID, "convert: dst_channels must be 1 or 3");
    const Images out = images(dst, nframes, H, (size_t)W * C, drs, dfs, dst_on_device);
    if ((rc = check_strides(h, "convert", "dst_", out))) return rc;
    // the raw source as planes of rows: the one plane of a format, or NV12's Y plane and, where colour is wanted, its U,V plane behind it
    const size_t row = frame_min_row_stride(f, W);
    const bool nv12 = f.format == ARUCOHIP_PIX_NV12;
    const Images luma = images(src, nframes, H, row, row_stride, frame_stride, src_on_device);
    Images chroma = luma;
    chroma.p += f.chroma_offset ? f.chroma_offset : row_stride * (size_t)H, chroma.rows = H / 2;
    // what a raw frame spans from its first to its last byte read, as one row: of NV12 both planes and what lies between them
    const Images span = images(src, nframes, 1, frame_min_stride(f, W, H, row_stride), 0, frame_stride, src_on_device);
    if ((rc = check_disjoint(h, "convert", "dst", out, "src", span))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const bool with_chroma = nv12 && C == 3;
    const size_t staged_frame = luma.packed_frame() + (with_chroma ? chroma.packed_frame() : 0);
    // the arena holds the raw host frames of the call and the converted frames a host caller gets
    size_t src_at, dst_at;
    if ((rc = carve_scratch(h, h, [&](Carver& cv) {
             src_at = cv.take_at(src_on_device ? 0 : (size_t)nframes * staged_frame);
             dst_at = cv.take_at(dst_on_device ? 0 : out.packed_bytes());
         })))
        return rc;
    DevImages sdev, cdev, ddev;
    FrameFmt sf = f;
    if ((rc = stage_input(h, s, luma, h->scratch, src_at, &sdev, staged_frame))) return rc;
    if (!src_on_device) {
        sf.chroma_offset = 0;   // the staged chroma plane follows the Y plane
        if (with_chroma && (rc = stage_input(h, s, chroma, h->scratch, src_at + luma.packed_frame(), &cdev, staged_frame))) return rc;
    }
    if ((rc = stage_output(h, out, h->scratch, dst_at, &ddev))) return rc;
    launch_ingest(s, sf, sdev.p, sdev.row, sdev.frame, W, H, nframes, C, ddev.p, ddev.row, ddev.frame);
    HIPCHK(h, hipGetLastError());
    if ((rc = unstage(h, s, out, ddev))) return rc;
    if (!dst_on_device) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
