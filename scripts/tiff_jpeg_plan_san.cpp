// The JPEG header parser and planner (pbx_test_tiff_jpeg_plan: tag 347's tables, every segment's
// marker segments up to its SOS header, the Huffman decode tables, the plan) under
// AddressSanitizer / UBSan: a stand-alone program (no Python, no device call).  Every segment and
// every tables stream lies in a heap block of exactly its own bytes, so a marker walk that reads
// past a cut-short header is caught.  The stream below is a 16 x 16 baseline stream built here:
// one or three components, quantisers of ones, a one-code DC and a two-code AC table, and an
// all-zero scan (DC difference 0, End-of-Block), which is all the host ever looks at.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/ (this file and csrc/source_plan.cpp
// compiled with the sanitizers by g++ alone).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pbx.h"

static int failures = 0;

typedef std::vector<uint8_t> Bytes;

static void put(Bytes& b, std::initializer_list<int> v) {
    for (int x : v) b.push_back((uint8_t)x);
}

static Bytes tables() {
    Bytes t;
    put(t, {0xFF, 0xD8, 0xFF, 0xDB, 0x00, 0x43, 0x00});
    t.insert(t.end(), 64, 1);
    // DC table 0: one code of 1 bit for size 0.  AC table 0: codes of 2 bits for EOB and ZRL.
    put(t, {0xFF, 0xC4, 0x00, 0x14, 0x00, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x00});
    put(t, {0xFF, 0xC4, 0x00, 0x15, 0x10, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x00, 0xF0});
    put(t, {0xFF, 0xD9});
    return t;
}

// SOI [tables] [APP0] SOF0 [DRI] SOS, entropy bytes, EOI
static Bytes stream(int ncomp, int hv0, bool with_tables, int w = 16, int h = 16, int dri = 0) {
    Bytes s;
    put(s, {0xFF, 0xD8});
    if (with_tables) {
        const Bytes t = tables();
        s.insert(s.end(), t.begin() + 2, t.end() - 2);
    }
    put(s, {0xFF, 0xE0, 0x00, 0x04, 'x', 'y', 0xFF, 0xFF});  // an APP0, then a fill byte before SOF
    put(s, {0xFF, 0xC0, 0x00, 8 + 3 * ncomp, 8, h >> 8, h & 255, w >> 8, w & 255, ncomp});
    for (int c = 0; c < ncomp; c++) put(s, {c + 1, c ? 0x11 : hv0, 0});
    if (dri) put(s, {0xFF, 0xDD, 0x00, 0x04, dri >> 8, dri & 255});
    put(s, {0xFF, 0xDA, 0x00, 6 + 2 * ncomp, ncomp});
    for (int c = 0; c < ncomp; c++) put(s, {c + 1, 0x00});
    put(s, {0, 63, 0});
    s.insert(s.end(), 8, 0x00);
    put(s, {0xFF, 0xD9});
    return s;
}

static size_t header_len(const Bytes& s) { return s.size() - 10; }

// The segments in one heap block of exactly their bytes; the tables in another.
struct Case {
    uint8_t* data;
    uint8_t* tab;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    pbx_tiff_jpeg j;
    Case(int32_t seg_w, int32_t seg_h, int32_t tiled, const std::vector<Bytes>& segs, const Bytes* tables, int32_t ycbcr) {
        offsets.push_back(0);
        for (const Bytes& b : segs) offsets.push_back(offsets.back() + b.size());
        data = new uint8_t[offsets.back() ? offsets.back() : 1];
        for (size_t k = 0; k < segs.size(); k++)
            if (!segs[k].empty()) memcpy(data + offsets[k], segs[k].data(), segs[k].size());
        tab = nullptr;
        if (tables) {
            tab = new uint8_t[tables->size() ? tables->size() : 1];
            if (!tables->empty()) memcpy(tab, tables->data(), tables->size());
        }
        s = pbx_tiff_segments{seg_w, seg_h, tiled, PBX_TIFF_JPEG, 1, 0, data, offsets.data()};
        j = pbx_tiff_jpeg{tab, tables ? tables->size() : 0, ycbcr, 0};
    }
    ~Case() {
        delete[] data;
        delete[] tab;
    }
    Case(const Case&) = delete;
};

static void expect(const char* what, int rc, int want_rc, const char* want_msg) {
    const char* err = pbx_last_error();
    const bool ok = rc == want_rc && (!want_msg || strstr(err, want_msg));
    printf("%-58s rc %3d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED: ", ok ? "" : err);
    if (!ok) failures++;
}

int main() {
    uint64_t out[6];
    const Bytes tabs = tables();
    {
        // a 40 x 30 plane in 16 x 16 tiles (3 x 2), 4:2:0, tables in the tag
        std::vector<Bytes> segs(6, stream(3, 0x22, false));
        Case c(16, 16, 1, segs, &tabs, 1);
        expect("tiles, 4:2:0, tables in tag 347", pbx_test_tiff_jpeg_plan(&c.s, &c.j, 40, 30, 3, 0, 0, out), 0, nullptr);
        if (out[0] != 6 || out[3] != 1 || out[4] != 3 || out[2] != 6 * (256 + 2 * 256)) failures++;
        Case b(16, 16, 1, std::vector<Bytes>(3, stream(3, 0x22, false)), &tabs, 1);
        expect("tiles, rows 16 .. 29 (one tile row)", pbx_test_tiff_jpeg_plan(&b.s, &b.j, 40, 30, 3, 16, 14, out), 0, nullptr);
        if (out[0] != 3) failures++;
        // strips of 16 rows on a 16 x 40 plane: 16, 16 and 8 rows; tables in the segments; gray
        Case s(16, 16, 0, {stream(1, 0x11, true), stream(1, 0x11, true), stream(1, 0x11, true, 16, 8, 2)}, nullptr, 0);
        expect("strips, gray, tables in the segments, DRI", pbx_test_tiff_jpeg_plan(&s.s, &s.j, 16, 40, 1, 0, 0, out), 0, nullptr);
        if (out[0] != 3 || out[3] != 1 || out[4] != 0 || out[1] != 16 * 40) failures++;
        Case o(16, 16, 1, {stream(3, 0x21, true)}, &tabs, 1);
        expect("both: the segment's tables override", pbx_test_tiff_jpeg_plan(&o.s, &o.j, 16, 16, 3, 0, 0, out), 0, nullptr);
        if (out[4] != 2) failures++;
        Case r(16, 16, 1, {stream(3, 0x11, true)}, nullptr, 0);
        expect("three components stored as they are", pbx_test_tiff_jpeg_plan(&r.s, &r.j, 16, 16, 3, 0, 0, out), 0, nullptr);
        if (out[4] != 0) failures++;
    }
    // every prefix of a segment's header, with and without its own tables
    int before = failures;
    for (int own = 0; own < 2; own++) {
        const Bytes good = stream(3, 0x22, own != 0, 16, 16, 4);
        for (size_t cut = 0; cut < header_len(good); cut++) {
            Case c(16, 16, 1, {Bytes(good.begin(), good.begin() + cut)}, own ? nullptr : &tabs, 1);
            const int rc = pbx_test_tiff_jpeg_plan(&c.s, &c.j, 16, 16, 3, 0, 0, out);
            if (rc != 400) { printf("segment prefix of %zu bytes: rc %d\n", cut, rc); failures++; }
        }
        Case whole(16, 16, 1, {Bytes(good.begin(), good.begin() + header_len(good))}, own ? nullptr : &tabs, 1);
        expect("a header with no entropy data after it (the device's to say)",
               pbx_test_tiff_jpeg_plan(&whole.s, &whole.j, 16, 16, 3, 0, 0, out), 0, nullptr);
    }
    printf("%-58s %s\n", "every prefix of two segment headers is refused", failures != before ? "FAILED" : "ok");
    // every prefix of tag 347
    before = failures;
    for (size_t cut = 0; cut < tabs.size(); cut++) {
        const Bytes t(tabs.begin(), tabs.begin() + cut);
        Case c(16, 16, 1, {stream(3, 0x22, false)}, &t, 1);
        const int rc = pbx_test_tiff_jpeg_plan(&c.s, &c.j, 16, 16, 3, 0, 0, out);
        if (rc != 400) { printf("tables prefix of %zu bytes: rc %d\n", cut, rc); failures++; }
    }
    printf("%-58s %s\n", "every prefix of the tables stream is refused", failures != before ? "FAILED" : "ok");
    {
        Case c(16, 16, 1, {stream(3, 0x22, false)}, nullptr, 1);
        expect("no tables anywhere", pbx_test_tiff_jpeg_plan(&c.s, &c.j, 16, 16, 3, 0, 0, out), 400, "missing quantiser");
        Case d(16, 16, 1, {stream(3, 0x41, true)}, nullptr, 1);
        expect("sampling 4x1", pbx_test_tiff_jpeg_plan(&d.s, &d.j, 16, 16, 3, 0, 0, out), 400, "sampling factors 4x1");
        Case e(16, 16, 1, {stream(3, 0x22, true)}, nullptr, 0);
        expect("subsampling without ycbcr", pbx_test_tiff_jpeg_plan(&e.s, &e.j, 16, 16, 3, 0, 0, out), 400, "subsampling 2x2 without");
        Case f(16, 16, 1, {stream(3, 0x22, true, 16, 32)}, nullptr, 1);
        expect("SOF size", pbx_test_tiff_jpeg_plan(&f.s, &f.j, 16, 16, 3, 0, 0, out), 400, "SOF size 16 x 32 != segment size 16 x 16");
        Bytes over = tables();
        over[2 + 69 + 5] = 3;  // three codes of one bit
        Case g(16, 16, 1, {stream(1, 0x11, false)}, &over, 0);
        expect("an over-subscribed table", pbx_test_tiff_jpeg_plan(&g.s, &g.j, 16, 16, 1, 0, 0, out), 400, "over-subscribed Huffman table");
        Bytes big = tables();
        big[2 + 69 + 3] = 0xFF;  // a DHT length past the stream's end
        Case h(16, 16, 1, {stream(1, 0x11, false)}, &big, 0);
        expect("a DHT longer than the tables stream", pbx_test_tiff_jpeg_plan(&h.s, &h.j, 16, 16, 1, 0, 0, out), 400, "truncated header");
        Case i(16, 16, 1, {stream(1, 0x11, true)}, nullptr, 0);
        i.s.compression = PBX_TIFF_DEFLATE;
        expect("compression 8 in a JPEG call", pbx_test_tiff_jpeg_plan(&i.s, &i.j, 16, 16, 1, 0, 0, out), 400, "bad compression 8");
        i.s.compression = PBX_TIFF_JPEG;
        uint64_t o4[4];
        expect("compression 7 in a plain TIFF call", pbx_test_tiff_plan(&i.s, 16, 16, 1, o4), 400, "bad compression 7");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
