// The irreversible (9/7) JPEG 2000 path on the host under AddressSanitizer / UBSan: the header
// parser's QCD styles 1 and 2 and the planner's step table (pbx_test_tiff_j2k_plan), and through
// pbx_test_tiff_j2k_decode the device's own code: tier 1 with its half bit (j2k_block<true>), the
// dequantising store, the float lifting, the ICT and the rounding of tiff_j2k_dev.h.  A
// stand-alone program (no Python, no device call) in the manner of tiff_j2k_plan_san.cpp: every
// segment lies in a heap block of exactly its own bytes, the streams are built here, their packets
// either empty (every coefficient zero: every sample exactly 2^(P-1), whatever the steps) or
// pseudo-random bytes, which decode to garbage magnitudes of up to 30 bit-planes or are refused.
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

// A w x h 9/7 codestream (transformation `trans`, 0 for 9/7) with a QCD of style `style`: style 2
// one 16-bit entry per sub-band (exponent `eps` + the band's gain, mantissa 100 b), style 1 the
// LL entry alone (exponent eps), style 0 one byte per sub-band.  The header's length in *hdr.
static Bytes stream(int w, int h, int ncomp, int prec, int levels, int xcb, int ycb, int prog, int mct, int trans, int style,
                    int guard, int eps, const Bytes& packets, size_t* hdr = nullptr) {
    Bytes s;
    put(s, {0xFF, 0x4F, 0xFF, 0x51, 0, 38 + 3 * ncomp, 0, 0});
    put32(s, w); put32(s, h); put32(s, 0); put32(s, 0); put32(s, w); put32(s, h); put32(s, 0); put32(s, 0);
    put(s, {0, ncomp});
    for (int c = 0; c < ncomp; c++) put(s, {prec - 1, 1, 1});
    put(s, {0xFF, 0x52, 0, 12, 0, prog, 0, 1, mct, levels, xcb - 2, ycb - 2, 0, trans});
    const int nb = 3 * levels + 1, bytes = style == 0 ? nb : style == 1 ? 2 : 2 * nb;
    put(s, {0xFF, 0x5C, (3 + bytes) >> 8, (3 + bytes) & 255, guard << 5 | style});
    for (int b = 0; b < (style == 1 ? 1 : nb); b++) {
        const int e = eps + (style == 2 && b ? 1 + (b % 3 == 0) : 0);
        if (style == 0) put(s, {e << 3});
        else put(s, {(e << 11 | (100 * b) % 2048) >> 8, (e << 11 | (100 * b) % 2048) & 255});
    }
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
        std::vector<Bytes> segs(6, stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 0, 2, 2, 8, Bytes(3, 0)));
        Case c(16, 16, 1, segs);
        expect("9/7 tiles, gray, style 2, every packet empty", pbx_test_tiff_j2k_plan(&c.s, 40, 30, PBX_UINT8, 1, 0, 0, out), 0, nullptr);
        if (out[0] != 6 || out[1] != 6 * 7 || out[2] != 6 * 3 || out[3] != 6 * 2048) { printf("counts\n"); failures++; }
        std::vector<uint8_t> px(40 * 30, 7);
        expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&c.s, 40, 30, PBX_UINT8, 1, px.data(), px.size()), 0, nullptr);
        for (uint8_t v : px) if (v != 128) { printf("sample %u\n", v); failures++; break; }
        // strips of 16 rows on a 33 x 40 plane: RGB through the ICT, style 1, 4 x 4 blocks, CPRL
        Case s(33, 16, 0, {stream(33, 16, 3, 8, 3, 2, 2, 4, 1, 0, 1, 2, 9, Bytes(12, 0)), stream(33, 16, 3, 8, 3, 2, 2, 4, 1, 0, 1, 2, 9, Bytes(12, 0)),
                           stream(33, 8, 3, 8, 1, 2, 2, 4, 1, 0, 1, 2, 9, Bytes(6, 0))});
        expect("9/7 strips, RGB with ICT, style 1, 4 x 4 blocks", pbx_test_tiff_j2k_plan(&s.s, 33, 40, PBX_UINT8, 3, 0, 0, out), 0, nullptr);
        if (out[0] != 3 || out[2] != 12 + 12 + 6) failures++;
        std::vector<uint8_t> rgb(33 * 40 * 3, 7);
        expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&s.s, 33, 40, PBX_UINT8, 3, rgb.data(), rgb.size()), 0, nullptr);
        for (uint8_t v : rgb) if (v != 128) { printf("sample %u\n", v); failures++; break; }
        // uint16, 32 levels on a 5 x 3 tile, a 1024 x 4 block, 30 bit-planes on every band
        Case d(5, 3, 0, {stream(5, 3, 1, 16, 32, 10, 2, 3, 0, 0, 2, 7, 22, Bytes(33, 0))});
        std::vector<uint16_t> p16(15, 7);
        expect("9/7 uint16, 32 levels on 5 x 3, 30 bit-planes", pbx_test_tiff_j2k_decode(&d.s, 5, 3, PBX_UINT16, 1, p16.data(), 30), 0, nullptr);
        for (uint16_t v : p16) if (v != 32768) { printf("sample %u\n", v); failures++; break; }
        // a reversible and an irreversible strip in one plan
        Case m(16, 16, 0, {stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 1, 0, 2, 8, Bytes(3, 0)), stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 0, 2, 2, 8, Bytes(3, 0))});
        std::vector<uint8_t> p2(16 * 32, 7);
        expect("a 5/3 and a 9/7 strip in one plane", pbx_test_tiff_j2k_decode(&m.s, 16, 32, PBX_UINT8, 1, p2.data(), p2.size()), 0, nullptr);
        for (uint8_t v : p2) if (v != 128) { printf("sample %u\n", v); failures++; break; }
    }
    // every prefix of two headers
    int before = failures;
    for (int k = 0; k < 2; k++) {
        size_t hdr = 0;
        const Bytes good = k ? stream(16, 16, 3, 8, 3, 6, 6, 2, 1, 0, 1, 2, 9, Bytes(12, 0), &hdr)
                             : stream(16, 16, 1, 16, 2, 4, 4, 0, 0, 0, 2, 2, 16, Bytes(3, 0), &hdr);
        for (size_t cut = 0; cut < hdr; cut++) {
            Case c(16, 16, 1, {Bytes(good.begin(), good.begin() + cut)});
            const int rc = pbx_test_tiff_j2k_plan(&c.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, 0, 0, out);
            if (rc != 400) { printf("header prefix of %zu bytes: rc %d\n", cut, rc); failures++; }
        }
        Case whole(16, 16, 1, {Bytes(good.begin(), good.begin() + hdr)});
        expect("a 9/7 header with no packet after it: the plan stands",
               pbx_test_tiff_j2k_plan(&whole.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, 0, 0, out), 0, nullptr);
        std::vector<uint8_t> px(16 * 16 * 6);
        expect("... and the decoder says what is missing",
               pbx_test_tiff_j2k_decode(&whole.s, 16, 16, k ? PBX_UINT8 : PBX_UINT16, k ? 3 : 1, px.data(), k ? 768 : 512), 400,
               "corrupt segment stream 0 (j2k, decoder code 1)");
    }
    printf("%-66s %s\n", "every prefix of two 9/7 headers is refused", failures != before ? "FAILED" : "ok");
    // pseudo-random packet bytes: decoded to garbage or refused, never a byte out of place
    before = failures;
    uint32_t lcg = 97531, n_ok = 0, n_refused = 0;
    for (int k = 0; k < 400; k++) {
        Bytes junk(16 + k % 200);
        for (uint8_t& v : junk) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
        if (k & 1) junk[0] |= 0xC0;  // a non-empty first packet whose first block is included
        const bool rgb = k % 3 == 0;
        const int xcb = 2 + k % 5, ycb = 2 + (k / 5) % 5;
        // exponents from few bit-planes up to the 30 the path allows, both styles
        const int style = 1 + k % 2, guard = 1 + k % 7, eps = (style == 1 ? 4 : 0) + k % (style == 1 ? 20 : 22);
        Case c(64, 48, 0, {stream(64, 48, rgb ? 3 : 1, rgb ? 8 : 16, k % 4, xcb, ycb, k % 5, rgb, 0, style, guard, eps, junk)});
        std::vector<uint8_t> px(64 * 48 * (rgb ? 3 : 2));
        const int rc = pbx_test_tiff_j2k_decode(&c.s, 64, 48, rgb ? PBX_UINT8 : PBX_UINT16, rgb ? 3 : 1, px.data(), px.size());
        if (rc == 0) n_ok++;
        else if (rc == 400 && strstr(pbx_last_error(), "corrupt segment stream 0 (j2k, decoder code")) n_refused++;
        else { printf("junk %d: rc %d %s\n", k, rc, pbx_last_error()); failures++; }
    }
    printf("%-66s %s (%u decoded, %u refused)\n", "400 9/7 streams of pseudo-random packet bytes", failures != before ? "FAILED" : "ok",
           n_ok, n_refused);
    {
        Case a(16, 16, 1, {stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 0, 0, 2, 8, Bytes(3, 0))});
        expect("9/7 with QCD style 0", pbx_test_tiff_j2k_plan(&a.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400,
               "irreversible wavelet (9/7) with quantisation style 0");
        Case b(16, 16, 1, {stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 1, 2, 2, 8, Bytes(3, 0))});
        expect("5/3 with QCD style 2", pbx_test_tiff_j2k_plan(&b.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "quantisation style 2");
        Case c(16, 16, 1, {stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 1, 1, 2, 8, Bytes(3, 0))});
        expect("5/3 with QCD style 1", pbx_test_tiff_j2k_plan(&c.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "quantisation style 1");
        Case d(16, 16, 1, {stream(16, 16, 1, 8, 2, 4, 4, 0, 0, 0, 2, 7, 24, Bytes(3, 0))});
        expect("31 bit-planes on a 9/7 band", pbx_test_tiff_j2k_plan(&d.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400, "(at most 30)");
        Case e(16, 16, 1, {stream(16, 16, 1, 8, 5, 4, 4, 0, 0, 0, 1, 2, 3, Bytes(6, 0))});
        expect("style 1 deriving a negative exponent", pbx_test_tiff_j2k_plan(&e.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400,
               "quantisation style 1 derives exponent -1");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
