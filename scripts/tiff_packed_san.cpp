// The host planner of bit-packed samples and PackBits segments (tiff_packed_plan, through
// pbx_test_tiff_packed_plan) under AddressSanitizer / UBSan: a stand-alone program (no Python, no
// device call).  Every segment set lies in a heap block of exactly its own bytes and every offsets
// table holds exactly the entries the call may read, so a planner that walks past either is
// caught.  Row bytes that do and do not end on a byte, short last strips, edge tiles, band rows at
// a y0 that is no multiple of the segment height, and every refusal of the new path.
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

static void want(const char* what, uint64_t got, uint64_t exp) {
    if (got == exp) return;
    printf("%-58s %llu, not %llu\n", what, (unsigned long long)got, (unsigned long long)exp);
    failures++;
}

typedef std::vector<uint8_t> Bytes;

// The segments in one heap block of exactly their bytes, the offsets in one of exactly theirs.
struct Segs {
    uint8_t* data;
    uint64_t* offsets;
    pbx_tiff_segments s;
    Segs(int32_t seg_w, int32_t seg_h, int32_t tiled, int32_t compression, const std::vector<Bytes>& segs) {
        offsets = new uint64_t[segs.size() + 1];
        offsets[0] = 0;
        for (size_t k = 0; k < segs.size(); k++) offsets[k + 1] = offsets[k] + segs[k].size();
        data = new uint8_t[offsets[segs.size()] ? offsets[segs.size()] : 1];
        for (size_t k = 0; k < segs.size(); k++)
            if (!segs[k].empty()) memcpy(data + offsets[k], segs[k].data(), segs[k].size());
        s = pbx_tiff_segments{seg_w, seg_h, tiled, compression, 1, 0, data, offsets};
    }
    ~Segs() { delete[] data; delete[] offsets; }
    Segs(const Segs&) = delete;
};

static uint64_t row_bytes(uint64_t w, uint64_t spp, uint64_t bits) { return (w * spp * bits + 7) / 8; }

int main() {
    uint64_t out[6];
    // strips of 7 rows on 45 rows (6 full strips and one of 3), every width and sample count
    for (int bits = 1; bits <= 16; bits++)
        for (int spp = 1; spp <= 4; spp++)
            for (int w : {16, 41, 70, 333}) {
                const int32_t pt = bits > 8 ? PBX_UINT16 : PBX_UINT8;
                const uint64_t rb = row_bytes(w, spp, bits);
                const pbx_tiff_packed k{bits, bits < 16 ? 1 + (w & 1) : 1, spp, spp - 1};
                std::vector<Bytes> segs;
                for (int y = 0; y < 45; y += 7) segs.push_back(Bytes(rb * (y + 7 <= 45 ? 7 : 45 - y)));
                Segs st(w, 7, 0, PBX_TIFF_NONE, segs);
                if (pbx_test_tiff_packed_plan(&st.s, &k, w, 45, pt, 0, 0, out)) {
                    expect("stored strips, whole plane", 400, 0, nullptr);
                    continue;
                }
                want("stored strips: streams", out[0], 0);
                want("stored strips: bytes", out[1], 45 * rb);
                want("stored strips: scratch", out[2], 0);
                want("stored strips: segments", out[3], 7);
                want("stored strips: row bytes", out[4], rb);
                want("stored strips: rows", out[5], 45);
                // rows 40 .. 44: strips 5 (rows 35 .. 41) and 6 (rows 42 .. 44) only
                Segs bd(w, 7, 0, PBX_TIFF_PACKBITS, {Bytes{0x81, 0}, Bytes{0x81, 0}});
                if (pbx_test_tiff_packed_plan(&bd.s, &k, w, 45, pt, 40, 5, out)) {
                    expect("PackBits strips, rows 40..44", 400, 0, nullptr);
                    continue;
                }
                want("band: streams", out[0], 2);
                want("band: bytes", out[1], 10 * rb);
                want("band: scratch", out[2], ((7 * rb + 255) & ~255ull) + ((3 * rb + 255) & ~255ull));
                want("band: rows", out[5], 10);
            }
    printf("%-58s %s\n", "strips: 16 widths x 4 sample counts x 4 plane widths", failures ? "FAILED" : "ok");
    {
        const pbx_tiff_packed k12{12, 1, 1, 0}, k1{1, 2, 1, 0}, k10{10, 1, 1, 0};
        Segs a(41, 4, 0, PBX_TIFF_NONE, {Bytes(62 * 4)});
        expect("12 bits x 41 px", pbx_test_tiff_packed_plan(&a.s, &k12, 41, 4, PBX_UINT16, 0, 0, out), 0, nullptr);
        want("12 bits x 41 px: row bytes", out[4], 62);
        Segs b(70, 4, 0, PBX_TIFF_NONE, {Bytes(9 * 4)});
        expect("1 bit x 70 px", pbx_test_tiff_packed_plan(&b.s, &k1, 70, 4, PBX_UINT8, 0, 0, out), 0, nullptr);
        want("1 bit x 70 px: row bytes", out[4], 9);
        Segs c(16, 4, 0, PBX_TIFF_NONE, {Bytes(20 * 4)});
        expect("10 bits x 16 px", pbx_test_tiff_packed_plan(&c.s, &k10, 16, 4, PBX_UINT16, 0, 0, out), 0, nullptr);
        want("10 bits x 16 px: row bytes", out[4], 20);
    }
    {
        // 32 x 16 tiles on 70 x 45: a grid of 3 x 3 full tiles; rows 17 .. 33 cover tile rows 1 and 2
        const pbx_tiff_packed k{12, 1, 1, 0};
        Segs t(32, 16, 1, PBX_TIFF_NONE, std::vector<Bytes>(9, Bytes(48 * 16)));
        expect("stored tiles, whole plane", pbx_test_tiff_packed_plan(&t.s, &k, 70, 45, PBX_UINT16, 0, 0, out), 0, nullptr);
        want("tiles: segments", out[3], 9);
        want("tiles: rows", out[5], 9 * 16);
        Segs b(32, 16, 1, PBX_TIFF_NONE, std::vector<Bytes>(6, Bytes(48 * 16)));
        expect("stored tiles, rows 17..33", pbx_test_tiff_packed_plan(&b.s, &k, 70, 45, PBX_UINT16, 17, 17, out), 0, nullptr);
        want("tile band: segments", out[3], 6);
        Segs z(32, 16, 1, PBX_TIFF_DEFLATE, std::vector<Bytes>(9, Bytes{0x78, 0x9c, 3, 0, 0, 0, 0, 1}));
        expect("deflate tiles", pbx_test_tiff_packed_plan(&z.s, &k, 70, 45, PBX_UINT16, 0, 0, out), 0, nullptr);
        want("deflate tiles: streams", out[0], 9);
        want("deflate tiles: scratch", out[2], 9 * 768);
        Segs l(32, 16, 1, PBX_TIFF_LZW, std::vector<Bytes>(9, Bytes{0x80, 0x40, 0x40}));
        expect("LZW tiles", pbx_test_tiff_packed_plan(&l.s, &k, 70, 45, PBX_UINT16, 0, 0, out), 0, nullptr);
        Segs o(32, 16, 1, PBX_TIFF_LZW, std::vector<Bytes>(9, Bytes{0x00, 0x01, 0x40}));
        expect("old-style LZW", pbx_test_tiff_packed_plan(&o.s, &k, 70, 45, PBX_UINT16, 0, 0, out), 400, "old-style");
        Segs q(32, 16, 1, PBX_TIFF_ZSTD, std::vector<Bytes>(9, Bytes{0x28, 0xb5, 0x2f}));
        expect("a zstd frame cut short", pbx_test_tiff_packed_plan(&q.s, &k, 70, 45, PBX_UINT16, 0, 0, out), 400, nullptr);
    }
    {
        Segs s(41, 4, 0, PBX_TIFF_NONE, {Bytes(62 * 4)});
        pbx_tiff_packed k{12, 1, 1, 0};
        const auto plan = [&](int32_t pt = PBX_UINT16) { return pbx_test_tiff_packed_plan(&s.s, &k, 41, 4, pt, 0, 0, out); };
        k.bits = 0;  expect("bits 0", plan(), 400, "bad bits 0 (1 .. 16)");
        k.bits = 17; expect("bits 17", plan(), 400, "bad bits 17 (1 .. 16)");
        k.bits = 12;
        expect("12 bits on uint8", plan(PBX_UINT8), 400, "12-bit samples on a plane of pixel type");
        expect("12 bits on float", plan(PBX_FLOAT), 400, "12-bit samples on a plane of pixel type");
        expect("12 bits on uint32", plan(PBX_UINT32), 400, "12-bit samples on a plane of pixel type");
        k.bits = 4;  expect("4 bits on uint16", plan(), 400, "4-bit samples on a plane of pixel type");
        k.bits = 12;
        k.fill_order = 0; expect("fill_order 0", plan(), 400, "bad fill_order 0 (1 or 2)");
        k.fill_order = 3; expect("fill_order 3", plan(), 400, "bad fill_order 3 (1 or 2)");
        k.fill_order = 2; k.bits = 16; expect("fill_order 2 on 16 bits", plan(), 400, "fill_order 2 on 16-bit samples");
        k.fill_order = 1; k.bits = 12;
        s.s.predictor = 2; expect("predictor 2", plan(), 400, "bad predictor 2 (bit-packed samples take 1 only");
        s.s.predictor = 1;
        s.s.flags = 1; expect("flags 1", plan(), 400, "bad flags 0x1");
        s.s.flags = 0;
        k.samples_per_pixel = 0; expect("0 samples per pixel", plan(), 400, "samples_per_pixel 0 outside 1 .. 4");
        k.samples_per_pixel = 5; expect("5 samples per pixel", plan(), 400, "samples_per_pixel 5 outside 1 .. 4");
        k.samples_per_pixel = 1; k.sample = 1; expect("sample 1 of 1", plan(), 400, "sample 1 outside segments of 1 samples");
        k.sample = 0;
        s.s.compression = 2; expect("compression 2 (CCITT)", plan(), 400, "bad compression 2 (1 none, 5 LZW, 8 deflate, 50000 zstd, 32773 PackBits)");
        s.s.compression = 7; expect("compression 7", plan(), 400, "bad compression 7");
        s.s.compression = PBX_TIFF_NONE;
        s.s.seg_w = 40; expect("strip width 40 of 41", plan(), 400, "strip width 40 != plane width 41");
        s.s.seg_w = 41;
        k.bits = 11; expect("a stored strip of another width's bytes", plan(), 400, "uncompressed segment 0: 248 bytes, not 228");
        k.bits = 12;
        s.s.tiled = 1; s.s.seg_w = 24; s.s.seg_h = 16; expect("a 24 x 16 tile", plan(), 400, "multiples of 16");
        s.s.tiled = 0; s.s.seg_w = 41; s.s.seg_h = 4;
        s.offsets[1] = 0; expect("an empty segment", plan(), 400, "segment 0 is empty");
        s.offsets[1] = 248;
        expect("rows outside the plane", pbx_test_tiff_packed_plan(&s.s, &k, 41, 4, PBX_UINT16, 3, 2, out), 400, "outside the plane");
        expect("the layout that is left", plan(), 0, nullptr);
        uint64_t four[4];
        s.s.compression = PBX_TIFF_PACKBITS;
        expect("PackBits through pbx_test_tiff_plan", pbx_test_tiff_plan(&s.s, 41, 4, 2, four), 400,
               "bad compression 32773 (1 none, 5 LZW, 8 deflate, 50000 zstd)");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
