// Host side of the frames-out stage (k_egress.hip): the argument checks and the export as a stage of its own, the mirror of
// arucohip_convert_batch (capi_ingest.hip), whose format record, stride arithmetic and checks it shares. The detection path is untouched.
#include <hip/hip_runtime.h>

#include "handle.h"

extern "C" {

int arucohip_export_batch(arucohip_handle* h, const uint8_t* src, int C, int nframes, int W, int H, size_t srs, size_t sfs, int src_on_device,
                          const arucohip_frame_format_t* fmt, int flags, void* dst_, size_t drs, size_t dfs, int dst_on_device) {
    if (!h) return ARUCOHIP_E_INVALID;
    uint8_t* dst = (uint8_t*)dst_;
    if (!src || !dst) return fail(h, ARUCOHIP_E_INVALID, "export: src or dst is NULL");
    FrameFmt f;
    int rc = take_format(h, fmt, &f);
    if (rc) return rc;
    if (f.format == ARUCOHIP_PIX_GRAY16) return fail(h, ARUCOHIP_E_INVALID, "export: GRAY16 is not a destination format");
    if (f.format >= ARUCOHIP_PIX_BAYER_RGGB && f.format <= ARUCOHIP_PIX_BAYER_GBRG)
        return fail(h, ARUCOHIP_E_INVALID, "export: a Bayer mosaic is not a destination format");
    if (C != 1 && C != 3) return fail(h, ARUCOHIP_E_INVALID, "export: src_channels must be 1 or 3");
    if (flags & ~ARUCOHIP_EXPORT_GREY_IS_LUMA) return fail(h, ARUCOHIP_E_INVALID, "export: unknown flag bits");
    if ((rc = check_frame_format(h, f, nframes, W, H, drs, dfs))) return rc;
    const Images in = images(src, nframes, H, (size_t)W * C, srs, sfs, src_on_device);
    if ((rc = check_strides(h, "export", "src_", in))) return rc;
    // the destination as planes of rows: the one plane of a format, or NV12's Y plane and its U,V plane behind it
    const size_t drow = arucohip_frame_min_row_stride(fmt, W);
    const bool nv12 = f.format == ARUCOHIP_PIX_NV12;
    const Images luma = images(dst, nframes, H, drow, drs, dfs, dst_on_device);
    Images chroma = luma;
    chroma.p += f.chroma_offset ? f.chroma_offset : drs * (size_t)H, chroma.rows = H / 2;
    // what an exported frame spans from its first to its last byte written, as one row: of NV12 both planes and what lies between them
    const Images span = images(dst, nframes, 1, arucohip_frame_min_stride(fmt, W, H, drs), 0, dfs, dst_on_device);
    if ((rc = check_disjoint(h, "export", "dst", span, "src", in))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t staged_frame = luma.packed_frame() + (nv12 ? chroma.packed_frame() : 0);
    // the arena holds the host frames of the call and the exported frames a host caller gets
    size_t src_at, dst_at;
    if ((rc = carve_scratch(h, h, [&](Carver& cv) {
             src_at = cv.take_at(src_on_device ? 0 : in.packed_bytes());
             dst_at = cv.take_at(dst_on_device ? 0 : (size_t)nframes * staged_frame);
         })))
        return rc;
    DevImages sdev, ddev, cdev;
    FrameFmt df = f;
    if ((rc = stage_input(h, s, in, h->scratch, src_at, &sdev))) return rc;
    if ((rc = stage_output(h, luma, h->scratch, dst_at, &ddev, staged_frame))) return rc;
    if (!dst_on_device) {
        df.chroma_offset = 0;   // the staged chroma plane follows the Y plane
        if (nv12 && (rc = stage_output(h, chroma, h->scratch, dst_at + luma.packed_frame(), &cdev, staged_frame))) return rc;
    }
    launch_egress(s, sdev.p, C, sdev.row, sdev.frame, W, H, nframes, df, (flags & ARUCOHIP_EXPORT_GREY_IS_LUMA) != 0, ddev.p, ddev.row, ddev.frame);
    HIPCHK(h, hipGetLastError());
    // down by rows: the bytes between rows, between the planes and between frames stay the caller's
    if ((rc = unstage(h, s, luma, ddev))) return rc;
    if (nv12 && !dst_on_device && (rc = unstage(h, s, chroma, cdev))) return rc;
    if (!dst_on_device) HIPCHK(h, hipStreamSynchronize(s));
    return ARUCOHIP_OK;
}

}  // extern "C"
