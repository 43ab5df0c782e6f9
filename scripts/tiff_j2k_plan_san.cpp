// The JPEG 2000 header parser and planner (pbx_test_tiff_j2k_plan) and the device's serial
// decoder code run on the host (pbx_test_tiff_j2k_decode: packet headers, MQ and bit-plane
// decoder, each code block's state in heap blocks of exactly the kernel's LDS sizes) under
// AddressSanitizer / UBSan: a stand-alone program (no Python, no device call).  Every segment
// lies in a heap block of exactly its own bytes, so a marker walk, a packet-header reader or an
// MQ decoder that reads past a cut-short stream is caught.  The streams are built here: SOC, SIZ,
// COD, QCD, COM, SOT, SOD and then either one zero byte per packet (every packet empty: all
// coefficients zero, every sample 2^(P-1)) or pseudo-random bytes, which decode to garbage or are
// refused, and must do either without touching a byte outside the planner's geometry.
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
static void put32(Bytes& b, uint32_t v) { put(b, {(int)(v >> 24), (int)(v >> 16) & 255, (int)(v >> 8) & 255, (int)v & 255}); }

// A w x h codestream of `ncomp` components of `prec` bits, `levels` decomposition levels, code
// blocks of 2^xcb x 2^ycb, optionally declared precincts of 2^15; the header's length in *hdr.
static Bytes stream(int w, int h, int ncomp, int prec, int levels, int xcb, int ycb, int prog, bool precincts, int mct,
                    const Bytes& packets, size_t* hdr = nullptr) {
    Bytes s;
    put(s, {0xFF, 0x4F, 0xFF, 0x51, 0, 38 + 3 * ncomp, 0, 0});
    put32(s, w); put32(s, h); put32(s, 0); put32(s, 0); put32(s, w); put32(s, h); put32(s, 0); put32(s, 0);
    put(s, {0, ncomp});
    for (int c = 0; c < ncomp; c++) put(s, {prec - 1, 1, 1});
    put(s, {0xFF, 0x52, 0, 12 + (precincts ? levels + 1 : 0), precincts ? 1 : 0, prog, 0, 1, mct, levels, xcb - 2, ycb - 2, 0, 1});
    for (int r = 0; precincts && r <= levels; r++) put(s, {0xFF});
    put(s, {0xFF, 0x5C, 0, 4 + 3 * levels, 2 << 5});
    for (int b = 0; b < 3 * levels + 1; b++) put(s, {(prec + (b ? 1 + (b % 3 == 0) : 0)) << 3});
    put(s, {0xFF, 0x64, 0, 6, 0, 1, 'h', 'i'});
    put(s, {0xFF, 0x90, 0, 10, 0, 0});
    put32(s, 0);  // Psot 0: to the end of the stream
    put(s, {0, 1, 0xFF, 0x93});
    if (hdr) *hdr = s.size();
    s.insert(s.end(), packets.begin(), packets.end());
    put(s, {0xFF, 0xD9});
    return s;
}

// The segments in one heap block of exactly their bytes.
struct Case {
    uint8_t* data;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    Case(int32_t seg_w, int32_t seg_h, int32_t tiled, const std::vector<Bytes>& segs) {
        offsets.push_back(0);
        for (const Bytes& b : segs) offsets.push_back(offsets.back() + b.size());
        data = new uint8_t[offsets.back() ? offsets.back() : 1];
        for (size_t k = 0; k < segs.size(); k++)
            if (!segs[k].empty()) memcpy(data + offsets[k], segs[k].data(), segs[k].size());
        s = pbx_tiff_segments{seg_w, seg_h, tiled, PBX_TIFF_J2K, 1, 0, data, offsets.data()};
    }
    ~Case() { delete[] data; }
    Case(const Case&) = delete;
};

static void expect(const char* what, int rc, int want_rc, const char* want_msg) {
    const char* err = pbx_last_error();
    const bool ok = rc == want_rc && (!want_msg || strstr(err, want_msg));
    printf("%-66s rc %3d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED: ", ok ? "" : err);
    if (!ok) failures++;
}

int main() {
    uint64_t out[4];
    {
        // a 40 x 30 plane in 16 x 16 tiles (3 x 2), gray 8-bit, 2 levels: 3 packets a tile, all empty
        std::vector<Bytes> segs(6, stream(16, 16, 1, 8, 2, 4, 4, 0, false, 0, Bytes(3, 0)));
        Case c(16, 16, 1, segs);
        expect("tiles, gray, every packet empty", pbx_test_tiff_j2k_plan(&c.s, 40, 30, PBX_UINT8, 1, 0, 0, out), 0, nullptr);
        // per tile: LL 4 x 4 (1 block), three bands of 4 x 4 (3), three of 8 x 8 (3); two planes of 1024 bytes
        if (out[0] != 6 || out[1] != 6 * 7 || out[2] != 6 * 3 || out[3] != 6 * 2048) { printf("counts\n"); failures++; }
        std::vector<uint8_t> px(40 * 30, 7);
        expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&c.s, 40, 30, PBX_UINT8, 1, px.data(), px.size()), 0, nullptr);
        for (uint8_t v : px) if (v != 128) { printf("sample %u\n", v); failures++; break; }
        Case b(16, 16, 1, std::vector<Bytes>(3, segs[0]));
        expect("tiles, rows 16 .. 29 (one tile row)", pbx_test_tiff_j2k_plan(&b.s, 40, 30, PBX_UINT8, 1, 16, 14, out), 0, nullptr);
        if (out[0] != 3) failures++;
        // strips of 16 rows on a 33 x 40 plane: 16, 16 and 8 rows; RGB through the RCT, 4 x 4 blocks, CPRL
        Case s(33, 16, 0, {stream(33, 16, 3, 8, 3, 2, 2, 4, true, 1, Bytes(12, 0)), stream(33, 16, 3, 8, 3, 2, 2, 4, true, 1, Bytes(12, 0)),
                           stream(33, 8, 3, 8, 1, 2, 2, 4, true, 1, Bytes(6, 0))});
        expect("strips, RGB, declared precincts, 4 x 4 blocks", pbx_test_tiff_j2k_plan(&s.s, 33, 40, PBX_UINT8, 3, 0, 0, out), 0, nullptr);
        if (out[0] != 3 || out[2] != 12 + 12 + 6) failures++;
        std::vector<uint8_t> rgb(33 * 40 * 3, 7);
        expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&s.s, 33, 40, PBX_UINT8, 3, rgb.data(), rgb.size()), 0, nullptr);
        for (uint8_t v : rgb) if (v != 128) { printf("sample %u\n", v); failures++; break; }
        // uint16, 32 levels on a 5 x 3 tile, a 1024 x 4 block
        Case d(5, 3, 0, {stream(5, 3, 1, 16, 32, 10, 2, 3, false, 0, Bytes(33, 0))});
        std::vector<uint16_t> p16(15, 7);
        expect("uint16, 32 levels on 5 x 3", pbx_test_tiff_j2k_decode(&d.s, 5, 3, PBX_UINT16, 1, p16.data(), 30), 0, nullptr);
        for (uint16_t v : p16) if (v != 32768) { printf("sample %u\n", v); failures++; break; }
    }
    // every prefix of two headers
    int before = failures;
    for (int k = 0; k < 2; k++) {
        size_t hdr = 0;
        const Bytes good = k ? stream(16, 16, 3, 8, 3, 6, 6, 2, true, 1, Bytes(12, 0), &hdr)
                             : stream(16, 16, 1, 16, 2, 4, 4, 0, false, 0, Bytes(3, 0), &hdr);
        for (size_t cut = 0; cut < hdr; cut++) {
            Case c(16, 16, 1, {Bytes(good.begin(), good.begin() + cut)});
            const int rc = pbx_test_tiff_j2k_plan(&c.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, 0, 0, out);
            if (rc != 400) { printf("header prefix of %zu bytes: rc %d\n", cut, rc); failures++; }
        }
        Case whole(16, 16, 1, {Bytes(good.begin(), good.begin() + hdr)});
        expect("a header with no packet after it: the plan stands",
               pbx_test_tiff_j2k_plan(&whole.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, 0, 0, out), 0, nullptr);
        std::vector<uint8_t> px(16 * 16 * 6);
        expect("... and the decoder says what is missing",
               pbx_test_tiff_j2k_decode(&whole.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, px.data(), k ? 768 : 512), 400,
               "corrupt segment stream 0 (j2k, decoder code 1)");
    }
    printf("%-66s %s\n", "every prefix of two headers is refused", failures != before ? "FAILED" : "ok");
    // pseudo-random packet bytes: decoded to garbage or refused, never a byte out of place
    before = failures;
    uint32_t lcg = 12345, n_ok = 0, n_refused = 0;
    for (int k = 0; k < 400; k++) {
        Bytes junk(16 + k % 200);
        for (uint8_t& v : junk) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
        if (k & 1) junk[0] |= 0xC0;  // a non-empty first packet whose first block is included
        const bool rgb = k % 3 == 0;
        const int xcb = 2 + k % 5, ycb = 2 + (k / 5) % 5;
        Case c(64, 48, 0, {stream(64, 48, rgb ? 3 : 1, rgb ? 8 : 16, k % 4, xcb, ycb, k % 5, false, rgb, junk)});
        std::vector<uint8_t> px(64 * 48 * (rgb ? 3 : 2));
        const int rc = pbx_test_tiff_j2k_decode(&c.s, 64, 48, rgb ? PBX_UINT8 : PBX_UINT16, rgb ? 3 : 1, px.data(), px.size());
        if (rc == 0) n_ok++;
        else if (rc == 400 && strstr(pbx_last_error(), "corrupt segment stream 0 (j2k, decoder code")) n_refused++;
        else { printf("junk %d: rc %d %s\n", k, rc, pbx_last_error()); failures++; }
    }
    printf("%-66s %s (%u decoded, %u refused)\n", "400 streams of pseudo-random packet bytes", failures != before ? "FAILED" : "ok",
           n_ok, n_refused);
    {
        size_t hdr;
        Bytes g = stream(16, 16, 1, 8, 2, 4, 4, 0, false, 0, Bytes(3, 0), &hdr);
        Bytes irr = g; irr[2 + 43 + 4 + 9] = 0;  // COD's transformation byte
        Case a(16, 16, 1, {irr});
        expect("the 9/7 wavelet", pbx_test_tiff_j2k_plan(&a.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "irreversible wavelet");
        Bytes lay = g; lay[2 + 43 + 4 + 3] = 2;
        Case b(16, 16, 1, {lay});
        expect("two layers", pbx_test_tiff_j2k_plan(&b.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "2 quality layers");
        Case c(16, 16, 1, {g});
        expect("the stream as it is", pbx_test_tiff_j2k_plan(&c.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 0, nullptr);
        Case d(32, 32, 1, {g});
        expect("SIZ size != segment size", pbx_test_tiff_j2k_plan(&d.s, 32, 32, PBX_UINT8, 1, 0, 0, out), 400,
               "SIZ size 16 x 16 != segment size 32 x 32");
        c.s.compression = PBX_TIFF_DEFLATE;
        expect("compression 8 in a JPEG 2000 call", pbx_test_tiff_j2k_plan(&c.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "bad compression 8");
        c.s.compression = PBX_TIFF_J2K;
        uint64_t o4[4];
        expect("compression 34712 in a plain TIFF call", pbx_test_tiff_plan(&c.s, 16, 16, 1, o4), 400, "bad compression 34712");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
