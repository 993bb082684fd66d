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
    const size_t srow = (size_t)W * C, sframe = srs * (size_t)(H - 1) + srow;
    if (srs < srow) return fail(h, ARUCOHIP_E_INVALID, "export: src_row_stride below width * src_channels");
    if (nframes > 1 && sfs < sframe) return fail(h, ARUCOHIP_E_INVALID, "export: src_frame_stride does not cover a frame");
    const size_t drow = arucohip_frame_min_row_stride(fmt, W), dframe = arucohip_frame_min_stride(fmt, W, H, drs);
    const size_t src_extent = (size_t)(nframes - 1) * sfs + sframe;
    const size_t dst_extent = (size_t)(nframes - 1) * dfs + dframe;
    if ((uintptr_t)src < (uintptr_t)dst + dst_extent && (uintptr_t)dst < (uintptr_t)src + src_extent) return fail(h, ARUCOHIP_E_INVALID, "export: dst overlaps src");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const uint8_t* sdev = src;
    size_t rs = srs, fs = sfs;
    if (!src_on_device) {   // the rows' own bytes go up
        HIPCHK(h, h->d_egress_src.reserve((size_t)nframes * srow * H));
        if ((rc = copy_rows(h, const_cast<uint8_t*>(src), srs, nframes > 1 ? sfs : srs * (size_t)H, srow, H, nframes, h->d_egress_src, true))) return rc;
        sdev = h->d_egress_src, rs = srow, fs = srow * H;
    }
    // the rows of one frame: NV12 has H / 2 rows of chroma, which in the staging buffer follow the Y plane
    const bool nv12 = f.format == ARUCOHIP_PIX_NV12;
    const size_t rows = nv12 ? (size_t)H + H / 2 : (size_t)H;
    uint8_t* ddev = dst;
    size_t ors = drs, ofs = dfs;
    FrameFmt df = f;
    if (!dst_on_device) {
        HIPCHK(h, h->d_egress.reserve((size_t)nframes * drow * rows));
        ddev = h->d_egress, ors = drow, ofs = drow * rows, df.chroma_offset = 0;
    }
    launch_egress(s, sdev, C, rs, fs, W, H, nframes, df, (flags & ARUCOHIP_EXPORT_GREY_IS_LUMA) != 0, ddev, ors, ofs);
    HIPCHK(h, hipGetLastError());
    if (!dst_on_device) {   // down by rows: the bytes between rows, between the planes and between frames stay the caller's
        if (!nv12) {
            if ((rc = copy_rows(h, dst, drs, nframes > 1 ? dfs : drs * (size_t)H, drow, H, nframes, ddev, false))) return rc;
        } else {
            const size_t coff = f.chroma_offset ? f.chroma_offset : drs * (size_t)H;
            for (int i = 0; i < nframes; i++) {
                uint8_t* fr = dst + (size_t)i * dfs;
                const uint8_t* st = ddev + (size_t)i * ofs;
                HIPCHK(h, hipMemcpy2DAsync(fr, drs, st, drow, drow, H, hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipMemcpy2DAsync(fr + coff, drs, st + drow * H, drow, drow, H / 2, hipMemcpyDeviceToHost, s));
            }
        }
        HIPCHK(h, hipStreamSynchronize(s));
    }
    return ARUCOHIP_OK;
}

}  // extern "C"
