// The host planner's new ground -- Zstandard segments (Compression = 50000) and Predictor = 3 --
// under AddressSanitizer / UBSan: a stand-alone program (no Python, no device call) that runs
// pbx_test_tiff_plan, pbx_test_tiff_band_plan and pbx_test_tiff_plan_samples on good, damaged and
// cut-short zstd frames, each in a heap block of exactly its own bytes, so that a header or block
// walk that reads past a frame's end is caught.  The planner and its refusals are host code only.
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

typedef std::vector<uint8_t> Bytes;

// One zstd frame of raw blocks that decodes to n zero bytes.  fcs_bytes: 0 (none, with a window
// descriptor), 1 (single segment), 2, 4 or 8; blocks: how many raw blocks the bytes are cut into.
static Bytes frame(uint32_t n, int fcs_bytes = 1, int blocks = 1, uint64_t fcs = ~0ull, uint8_t fhd_or = 0) {
    Bytes f{0x28, 0xb5, 0x2f, 0xfd};
    if (fcs == ~0ull) fcs = n;
    const uint8_t flag = fcs_bytes == 2 ? 1 : fcs_bytes == 4 ? 2 : fcs_bytes == 8 ? 3 : 0;
    const bool single = fcs_bytes == 1;
    f.push_back((uint8_t)(flag << 6 | (single ? 0x20 : 0) | fhd_or));
    if (!single) f.push_back(0x58);  // window descriptor
    const uint64_t v = fcs_bytes == 2 ? fcs - 256 : fcs;
    for (int k = 0; k < fcs_bytes; k++) f.push_back((uint8_t)(v >> (8 * k)));
    for (int b = 0; b < blocks; b++) {
        const uint32_t len = b + 1 < blocks ? n / blocks : n - (n / blocks) * (blocks - 1);
        const uint32_t bh = len << 3 | (b + 1 == blocks ? 1u : 0u);
        f.push_back((uint8_t)bh); f.push_back((uint8_t)(bh >> 8)); f.push_back((uint8_t)(bh >> 16));
        f.insert(f.end(), len, 0);
    }
    return f;
}

// The segments in one heap block of exactly their bytes.
struct Segs {
    uint8_t* data;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    Segs(int32_t seg_w, int32_t seg_h, int32_t tiled, int32_t compression, int32_t predictor,
         const std::vector<Bytes>& segs) {
        offsets.push_back(0);
        for (const Bytes& b : segs) offsets.push_back(offsets.back() + b.size());
        data = new uint8_t[offsets.back() ? offsets.back() : 1];
        for (size_t k = 0; k < segs.size(); k++)
            if (!segs[k].empty()) memcpy(data + offsets[k], segs[k].data(), segs[k].size());
        s = pbx_tiff_segments{seg_w, seg_h, tiled, compression, predictor, 0, data, offsets.data()};
    }
    ~Segs() { delete[] data; }
    Segs(const Segs&) = delete;
};

int main() {
    uint64_t out[4];
    // a 300 x 5 plane in strips of 2 rows: strips of 2, 2 and 1 rows
    for (int bpp = 4; bpp <= 8; bpp *= 2)
        for (int pred = 1; pred <= 3; pred += 2) {
            const uint32_t row = 300u * bpp;
            for (int fb : {0, 1, 2, 4, 8}) {
                if (fb == 1 && 2 * row > 255) fb = 2;
                Segs z(300, 2, 0, PBX_TIFF_ZSTD, pred, {frame(2 * row, fb), frame(2 * row, fb, 3), frame(row, fb)});
                expect("zstd strips, whole plane", pbx_test_tiff_plan(&z.s, 300, 5, bpp, out), 0, nullptr);
                if (out[0] != 3 || out[1] != 5ull * row || out[3] != (pred == 3 ? 3u : 0u)) failures++;
                Segs b(300, 2, 0, PBX_TIFF_ZSTD, pred, {frame(2 * row, fb), frame(row, fb)});
                expect("zstd strips, rows 3..4", pbx_test_tiff_band_plan(&b.s, 300, 5, bpp, 3, 2, out), 0, nullptr);
                expect("zstd strips, rows 3..4 (samples hook)", pbx_test_tiff_plan_samples(&b.s, 300, 5, bpp, 1, 3, 2, out), 0, nullptr);
            }
            Segs st(300, 2, 0, PBX_TIFF_NONE, pred, {Bytes(2 * row), Bytes(2 * row), Bytes(row)});
            expect("stored strips, whole plane", pbx_test_tiff_plan(&st.s, 300, 5, bpp, out), 0, nullptr);
            if (pred == 3 && (out[0] != 0 || out[2] != 0 || out[3] != 3)) failures++;
        }
    // every prefix of a good frame, as the only segment of an 8 x 1 float plane (32 bytes)
    for (int fb : {0, 1, 2, 4, 8}) {
        const Bytes good = frame(32, fb == 2 ? 2 : fb, 2, fb == 2 ? 288 : 32);
        for (size_t cut = 1; cut < good.size(); cut++) {
            Segs s(fb == 2 ? 72 : 8, 1, 0, PBX_TIFF_ZSTD, 3, {Bytes(good.begin(), good.begin() + cut)});
            const int rc = pbx_test_tiff_plan(&s.s, fb == 2 ? 72 : 8, 1, 4, out);
            if (rc != 400) { printf("prefix of %zu bytes (fcs %d): rc %d\n", cut, fb, rc); failures++; }
        }
    }
    printf("%-58s %s\n", "every prefix of five frame shapes is refused", failures ? "FAILED" : "ok");
    {
        Bytes f = frame(32);
        f.push_back(0); f.push_back(0);
        Segs s(8, 1, 0, PBX_TIFF_ZSTD, 3, {f});
        expect("bytes after the frame", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "segment 0: 2 bytes after the zstd frame");
    }
    {
        Segs s(8, 1, 0, PBX_TIFF_ZSTD, 3, {frame(32, 1, 1, 31)});
        expect("content size 31 of 32", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "zstd content size 31 != segment bytes 32");
        Segs t(8, 1, 0, PBX_TIFF_ZSTD, 1, {frame(32, 8, 1, ~0ull - 1)});
        expect("content size 2^64 - 2", pbx_test_tiff_plan(&t.s, 8, 1, 4, out), 400, "zstd content size");
    }
    {
        Segs s(8, 1, 0, PBX_TIFF_ZSTD, 3, {frame(32, 1, 1, ~0ull, 1)});
        expect("a dictionary id", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "zstd frame with a dictionary id");
        Segs t(8, 1, 0, PBX_TIFF_ZSTD, 3, {frame(32, 1, 1, ~0ull, 8)});
        expect("the reserved header bit", pbx_test_tiff_plan(&t.s, 8, 1, 4, out), 400, "reserved zstd frame header bit");
    }
    {
        Bytes f = frame(32);
        f[6] |= 6;  // block type 3
        Segs s(8, 1, 0, PBX_TIFF_ZSTD, 3, {f});
        expect("a reserved block type", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "reserved zstd block type");
        Bytes g = frame(32);
        g[7] = 0xff; g[8] = 0xff;  // a block of 2 MiB in a frame of 41 bytes
        Segs t(8, 1, 0, PBX_TIFF_ZSTD, 3, {g});
        expect("a block past the frame's end", pbx_test_tiff_plan(&t.s, 8, 1, 4, out), 400, "truncated zstd frame");
        Bytes h = frame(32);
        h[6] &= ~1;  // the last block does not say so
        Segs u(8, 1, 0, PBX_TIFF_ZSTD, 3, {h});
        expect("no last block", pbx_test_tiff_plan(&u.s, 8, 1, 4, out), 400, "truncated zstd frame");
    }
    {
        Segs s(8, 1, 0, PBX_TIFF_ZSTD, 1, {Bytes{0x50, 0x2a, 0x4d, 0x18, 0, 0, 0, 0}});
        expect("a skippable frame", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "skippable zstd frame");
        Segs t(8, 1, 0, PBX_TIFF_ZSTD, 1, {Bytes{0x78, 0x9c, 3, 0, 0, 0, 0, 1}});
        expect("a zlib stream", pbx_test_tiff_plan(&t.s, 8, 1, 4, out), 400, "not a zstd frame");
    }
    {
        Segs s(8, 1, 0, PBX_TIFF_LZW, 3, {Bytes{0x80, 0, 1}});
        expect("predictor 3 on bytes", pbx_test_tiff_plan(&s.s, 8, 1, 1, out), 400, "bad predictor 3");
        expect("predictor 3 on shorts", pbx_test_tiff_band_plan(&s.s, 8, 1, 2, 0, 1, out), 400, "bad predictor 3");
        expect("predictor 3 on three samples", pbx_test_tiff_plan_samples(&s.s, 8, 1, 4, 3, 0, 0, out), 400, "bad predictor 3");
        s.s.predictor = 4;
        expect("predictor 4", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "bad predictor 4");
        s.s.predictor = 3;
        s.s.compression = 50001;
        expect("compression 50001", pbx_test_tiff_plan(&s.s, 8, 1, 4, out), 400, "bad compression 50001");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
