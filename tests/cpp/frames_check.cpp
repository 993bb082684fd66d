// Walks ah::Images (aruco_amd/csrc/frames_host.h) over a grid of small batches on the CPU: n 1..3, 1..7 bytes per row, 1..4 rows, row
// strides from one below the row's bytes to three above, frame strides from one below an image to a row and two bytes above, and the
// gap-free one. Every rule is restated here in arithmetic of its own, by enumerating (image, row, byte): what the stride check refuses,
// what the batch spans, when two batches overlap, and that the copy plan, replayed with memcpy on arrays of exactly extent() bytes,
// packs and unpacks the image bytes and nothing else. No tolerance: they are rules.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../aruco_amd/csrc/frames_host.h"

static long failures = 0, checked = 0;
#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        checked++;                                                                                                               \
        if (!(cond) && failures++ < 20)                                                                                          \
            fprintf(stderr, "FAIL %s (line %d): n %d rows %d row_bytes %zu row %zu frame %zu\n", #cond, __LINE__, im.n, im.rows, \
                    im.row_bytes, im.row, im.frame);                                                                             \
    } while (0)

static const uint8_t PAD = 0xA5;

static size_t offset_of(const ah::Images& im, int i, int r, size_t b) { return (size_t)i * im.frame + (size_t)r * im.row + b; }

struct CopyCall {
    size_t here, pitch, packed, packed_pitch, bytes, rows;
};

// The plan with the images `staged_frame` bytes apart on the packed side (0: back to back), replayed up and down.
static void check_copies(ah::Images im, size_t staged_frame) {
    const size_t ext = im.extent(), pframe = staged_frame ? staged_frame : im.packed_frame();
    const size_t pbytes = (size_t)(im.n - 1) * pframe + im.packed_frame();
    std::vector<uint8_t> host(ext, PAD), back(ext, PAD), packed(pbytes, 0xEE);
    std::vector<char> pixel(ext, 0), written(pbytes, 0);
    for (int i = 0; i < im.n; i++)
        for (int r = 0; r < im.rows; r++)
            for (size_t b = 0; b < im.row_bytes; b++) {
                const size_t o = offset_of(im, i, r, b);
                CHECK(!pixel[o]);   // valid strides: no two image bytes share an address
                pixel[o] = 1, host[o] = (uint8_t)(o * 37 + 11);
            }
    std::vector<CopyCall> calls;
    const int rc = im.for_each_copy(
        [&](size_t here, size_t pitch, size_t to, size_t packed_pitch, size_t bytes, size_t rows) {
            calls.push_back({here, pitch, to, packed_pitch, bytes, rows});
            return 0;
        },
        staged_frame);
    CHECK(rc == 0);
    const bool gap_free = im.n == 1 || (im.frame == im.row * (size_t)im.rows && pframe == im.packed_frame());
    CHECK(calls.size() == (size_t)(gap_free ? 1 : im.n));
    // up: only image bytes are read, each packed byte is written once
    bool inside = true;
    for (const CopyCall& c : calls)
        for (size_t r = 0; r < c.rows; r++)
            for (size_t b = 0; b < c.bytes; b++) {
                const size_t h = c.here + r * c.pitch + b, p = c.packed + r * c.packed_pitch + b;
                if (h >= ext || !pixel[h] || p >= pbytes || written[p]) {
                    inside = false;
                    continue;
                }
                written[p] = 1;
            }
    CHECK(inside);
    if (!inside) return;   // a replay would leave the arrays
    for (const CopyCall& c : calls)
        for (size_t r = 0; r < c.rows; r++) memcpy(packed.data() + c.packed + r * c.packed_pitch, host.data() + c.here + r * c.pitch, c.bytes);
    size_t nwritten = 0;
    for (char w : written) nwritten += w;
    CHECK(nwritten == im.packed_bytes());
    if (!staged_frame) CHECK(pbytes == im.packed_bytes());
    for (int i = 0; i < im.n; i++)
        for (int r = 0; r < im.rows; r++)
            for (size_t b = 0; b < im.row_bytes; b++)
                CHECK(packed[(size_t)i * pframe + (size_t)r * im.packed_row() + b] == host[offset_of(im, i, r, b)]);
    // down into a second array: the image bytes return, the padding keeps its sentinel
    for (const CopyCall& c : calls)
        for (size_t r = 0; r < c.rows; r++) memcpy(back.data() + c.here + r * c.pitch, packed.data() + c.packed + r * c.packed_pitch, c.bytes);
    CHECK(back == host);
}

static void check_overlap(ah::Images im, ah::Images other) {
    const long a0 = 4096, ea = (long)im.extent(), eb = (long)other.extent();
    im.p = (uint8_t*)(uintptr_t)a0;
    for (long b0 = a0 - eb - 1; b0 <= a0 + ea + 1; b0++) {   // from a byte apart through touching and one shared byte to a byte apart
        other.p = (uint8_t*)(uintptr_t)b0;
        const long lo = a0 > b0 ? a0 : b0, hi = a0 + ea < b0 + eb ? a0 + ea : b0 + eb;
        CHECK(im.overlaps(other) == (lo < hi));
        CHECK(other.overlaps(im) == (lo < hi));
    }
}

int main() {
    const ah::Images fixed = ah::images(nullptr, 2, 3, 5, 7, 30, 0);
    long layouts = 0;
    for (int n = 1; n <= 3; n++)
        for (size_t row_bytes = 1; row_bytes <= 7; row_bytes++)
            for (int rows = 1; rows <= 4; rows++)
                for (size_t row = row_bytes - 1; row <= row_bytes + 3; row++) {
                    const size_t image = (size_t)(rows - 1) * row + row_bytes;
                    std::vector<size_t> frames;
                    for (size_t f = image - 1; f <= image + row + 2; f++) frames.push_back(f);
                    frames.push_back(row * (size_t)rows);
                    for (size_t frame : frames) {
                        const ah::Images im = ah::images(nullptr, n, rows, row_bytes, row, frame, 0);
                        layouts++;
                        CHECK(im.image_bytes() == image);
                        const ah::Images::Strides want = row < row_bytes                ? ah::Images::ROW_BELOW_ROW_BYTES
                                                         : (n > 1 && frame < image) ? ah::Images::FRAME_BELOW_IMAGE
                                                                                    : ah::Images::STRIDES_OK;
                        CHECK(im.check_strides() == want);
                        size_t last = 0;
                        for (int i = 0; i < n; i++)
                            for (int r = 0; r < rows; r++)
                                for (size_t b = 0; b < row_bytes; b++) last = last > offset_of(im, i, r, b) ? last : offset_of(im, i, r, b);
                        CHECK(im.extent() == last + 1);
                        CHECK(im.packed_row() == row_bytes && im.packed_frame() == rows * row_bytes && im.packed_bytes() == n * rows * row_bytes);
                        check_overlap(im, im);
                        check_overlap(im, fixed);
                        if (want != ah::Images::STRIDES_OK) continue;
                        check_copies(im, 0);
                        check_copies(im, im.packed_frame());       // named, but back to back all the same
                        check_copies(im, im.packed_frame() + 3);   // a plane staged with another plane's rows behind each image
                    }
                }
    printf("%ld layouts, %ld checks, %ld failures\n", layouts, checked, failures);
    return failures ? 1 : 0;
}
