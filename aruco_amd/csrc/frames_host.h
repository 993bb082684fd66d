// A batch of strided byte images as the C ABI's image entry points take one: frames, destination images, a texture, a mask batch, a plane
// of an NV12 surface. Host-only and free of HIP types: tests/cpp/frames_check.cpp walks it on the CPU. The arithmetic of such a batch
// lives here once: what a row and an image span, what the strides must cover, when two batches may share bytes, and the copies between
// the caller's layout and the packed one (handle.h issues them).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ah {

// n images of `rows` rows of row_bytes bytes at p: `row` bytes from row to row, `frame` bytes from image to image. `frame` is ignored
// when n == 1. The bytes between the rows and between the images are the caller's: nothing reads or writes them.
struct Images {
    uint8_t* p;
    int n, rows;
    size_t row_bytes, row, frame;
    int on_device;

    size_t image_bytes() const { return (size_t)(rows - 1) * row + row_bytes; }   // first to last byte of one image
    size_t extent() const { return (size_t)(n - 1) * frame + image_bytes(); }     // first to last byte of the batch
    size_t packed_row() const { return row_bytes; }
    size_t packed_frame() const { return (size_t)rows * row_bytes; }
    size_t packed_bytes() const { return (size_t)n * packed_frame(); }

    enum Strides { STRIDES_OK, ROW_BELOW_ROW_BYTES, FRAME_BELOW_IMAGE };
    Strides check_strides() const {
        if (row < row_bytes) return ROW_BELOW_ROW_BYTES;
        if (n > 1 && frame < image_bytes()) return FRAME_BELOW_IMAGE;
        return STRIDES_OK;
    }

    // Whether [p, p + extent()) meets o's interval. Host and device addresses share one space, so one comparison serves every
    // combination. Conservative on purpose: two batches whose images interleave in each other's gaps count as overlapping.
    bool overlaps(const Images& o) const {
        const uintptr_t a = (uintptr_t)p, b = (uintptr_t)o.p;
        return a < b + o.extent() && b < a + extent();
    }

    // The 2-D copies between this layout and the packed one, image i at i * staged_frame (0: packed_frame(), the images back to back):
    // copy(offset here, pitch here, packed offset, packed pitch, width in bytes, rows) once for the batch when neither side has a gap
    // between its images, else once per image. Stops at the first copy that returns non-zero and returns that.
    template <class Copy>
    int for_each_copy(Copy copy, size_t staged_frame = 0) const {
        const size_t to = staged_frame ? staged_frame : packed_frame();
        const bool flat = n == 1 || (frame == row * (size_t)rows && to == packed_frame());
        const int calls = flat ? 1 : n;
        const size_t per = flat ? (size_t)n * rows : (size_t)rows;
        for (int i = 0; i < calls; i++)
            if (const int rc = copy((size_t)i * frame, row, (size_t)i * to, row_bytes, row_bytes, per)) return rc;
        return 0;
    }
};

// the record of a caller's pointer, whether the call reads or writes it
inline Images images(const void* p, int n, int rows, size_t row_bytes, size_t row, size_t frame, int on_device) {
    return Images{(uint8_t*)const_cast<void*>(p), n, rows, row_bytes, row, frame, on_device};
}

}  // namespace ah
