// The host planner of the multi-sample TIFF calls under AddressSanitizer / UBSan: a stand-alone
// program (no Python, no device call) that runs pbx_test_tiff_plan_samples on good and malformed
// offset tables.  The planner and its refusals are host code only.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/ (this file and csrc/source_plan.cpp
// compiled with the sanitizers by g++ alone).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbx.h"

static int failures = 0;

static void expect(const char* what, int rc, int want_rc, const char* want_msg) {
    const char* err = pbx_last_error();
    const bool ok = rc == want_rc && (!want_msg || strstr(err, want_msg));
    printf("%-58s rc %3d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED: ", ok ? "" : err);
    if (!ok) failures++;
}

struct Segs {
    std::vector<uint8_t> data;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    Segs(int32_t seg_w, int32_t seg_h, int32_t tiled, int32_t compression, int32_t predictor,
         const std::vector<uint64_t>& lens, uint8_t first = 0x80) {
        offsets.push_back(0);
        for (uint64_t l : lens) offsets.push_back(offsets.back() + l);
        data.assign(offsets.back() ? offsets.back() : 1, 0);  // exactly the bytes the offsets name
        for (size_t k = 0; k + 1 < offsets.size(); k++)
            if (offsets[k + 1] > offsets[k]) data[offsets[k]] = first;
        s = pbx_tiff_segments{seg_w, seg_h, tiled, compression, predictor, 0, data.data(), offsets.data()};
    }
};

int main() {
    uint64_t out[4];
    for (int spp = 1; spp <= 4; spp++)
        for (int bpp = 1; bpp <= 4; bpp *= 2) {
            const uint64_t row = 150ull * bpp * spp;
            Segs strips(150, 32, 0, PBX_TIFF_NONE, 2, {32 * row, 32 * row, 32 * row, 4 * row});
            expect("stored strips, whole plane", pbx_test_tiff_plan_samples(&strips.s, 150, 100, bpp, spp, 0, 0, out), 0, nullptr);
            if (out[1] != 100 * row) { printf("decoded sum %llu\n", (unsigned long long)out[1]); failures++; }
            Segs band(150, 32, 0, PBX_TIFF_NONE, 2, {32 * row, 32 * row});
            expect("stored strips, rows 33..72", pbx_test_tiff_plan_samples(&band.s, 150, 100, bpp, spp, 33, 40, out), 0, nullptr);
            Segs tiles(64, 64, 1, PBX_TIFF_LZW, 2, {5, 6, 7, 8, 9, 10});
            expect("LZW tiles, whole plane", pbx_test_tiff_plan_samples(&tiles.s, 150, 100, bpp, spp, 0, 0, out), 0, nullptr);
            if (out[0] != 6 || out[1] != 6ull * 64 * 64 * bpp * spp) failures++;
            Segs last(64, 64, 1, PBX_TIFF_DEFLATE, 1, {3, 3, 3});
            expect("deflate tiles, the last tile row", pbx_test_tiff_plan_samples(&last.s, 150, 100, bpp, spp, 99, 1, out), 0, nullptr);
        }
    const uint64_t row = 150 * 2 * 3;
    {
        Segs s(150, 32, 0, PBX_TIFF_NONE, 1, {32 * row, 32 * row, 32 * row, 4 * row});
        s.offsets[2] = s.offsets[1] - 1;  // decreasing
        expect("offsets that decrease", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "bad offsets");
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_NONE, 1, {32 * row, 32 * row, 32 * row, 4 * row});
        s.offsets[2] = s.offsets[4] + 1000;  // past the last offset
        expect("an offset past the end of the data", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "bad offsets");
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_NONE, 1, {32 * row, 32 * row, 32 * row, 4 * row});
        s.offsets[1] = ~0ull;  // wraps every length computed from it
        expect("a huge offset", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "bad offsets");
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_NONE, 1, {32 * row / 3, 32 * row / 3, 32 * row / 3, 4 * row / 3});
        expect("stored segments sized for one sample", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "uncompressed segment 0");
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_LZW, 1, {4, 0, 4, 4});
        expect("an empty segment", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "segment 1 is empty");
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_LZW, 1, {1, 1, 1, 1}, 0);  // one byte: the old-style test reads two
        expect("one-byte LZW segments", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 0, nullptr);
    }
    {
        Segs s(150, 32, 0, PBX_TIFF_LZW, 1, {4, 4, 4, 4});
        expect("samples_per_pixel 0", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 0, 0, 0, out), 400, "outside 1 .. 4");
        expect("samples_per_pixel 5", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 5, 0, 0, out), 400, "outside 1 .. 4");
        expect("64-bit samples", pbx_test_tiff_plan_samples(&s.s, 150, 100, 8, 3, 0, 0, out), 400, "64-bit samples");
        expect("rows past the plane", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 90, 11, out), 400, "outside the plane");
        expect("negative rows", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, -1, out), 400, "outside the plane");
        expect("a null table", pbx_test_tiff_plan_samples(nullptr, 150, 100, 2, 3, 0, 0, out), 400, "null argument");
        s.s.seg_h = 0;
        expect("seg_h 0", pbx_test_tiff_plan_samples(&s.s, 150, 100, 2, 3, 0, 0, out), 400, "bad segment shape");
    }
    {
        Segs s(1 << 19, 768, 0, PBX_TIFF_LZW, 1, {4});
        expect("a strip past 2^31 - 1 bytes with two samples", pbx_test_tiff_plan_samples(&s.s, 1 << 19, 768, 4, 2, 0, 0, out), 400, "too large");
        Segs t(0x7fffffff, 0x7fffffff, 0, PBX_TIFF_LZW, 1, {4});
        expect("the largest strip shape", pbx_test_tiff_plan_samples(&t.s, 0x7fffffff, 0x7fffffff, 4, 4, 0, 0, out), 400, "too large");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
