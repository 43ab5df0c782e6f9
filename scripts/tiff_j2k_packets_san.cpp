// The JPEG 2000 packet structure behind PBX_TIFF_F_J2K_PACKETS -- quality layers, precincts, SOP
// and EPH markers -- under AddressSanitizer / UBSan: the planner's packet list
// (pbx_test_tiff_j2k_plan) and the device's own walker and gather arithmetic run on the host
// (pbx_test_tiff_j2k_decode: j2k_packets and j2k_gather_span of csrc/tiff_j2k_dev.h, the tables
// and every stream's gather area in heap blocks of exactly their planned sizes).  A stand-alone
// program: no Python, no device call, nothing preloaded.  Every segment lies in a heap block of
// exactly its own bytes.  The streams are built here: headers with layers and declared precincts
// over packets that are all empty, a one-block stream whose block gets bytes in two and three
// layers (with Lblock growing), the same with SOP and EPH markers, and pseudo-random packet bytes
// under a three-layer, multi-precinct header, which decode to garbage or are refused.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/.
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

// A w x h codestream: `layers`, Scod bits `scod` (2 SOP, 4 EPH), precinct exponents pp (PPx = PPy,
// one per resolution; empty: none declared), code blocks of 2^cb x 2^cb.
static Bytes stream(int w, int h, int ncomp, int prec, int levels, int cb, int prog, int layers, int scod, const std::vector<int>& pp,
                    const Bytes& packets, size_t* hdr = nullptr) {
    Bytes s;
    put(s, {0xFF, 0x4F, 0xFF, 0x51, 0, 38 + 3 * ncomp, 0, 0});
    put32(s, w); put32(s, h); put32(s, 0); put32(s, 0); put32(s, w); put32(s, h); put32(s, 0); put32(s, 0);
    put(s, {0, ncomp});
    for (int c = 0; c < ncomp; c++) put(s, {prec - 1, 1, 1});
    put(s, {0xFF, 0x52, 0, 12 + (int)pp.size(), scod | (pp.empty() ? 0 : 1), prog, layers >> 8, layers & 255, ncomp == 3, levels,
            cb - 2, cb - 2, 0, 1});
    for (int e : pp) put(s, {e | e << 4});
    put(s, {0xFF, 0x5C, 0, 4 + 3 * levels, 2 << 5});
    for (int b = 0; b < 3 * levels + 1; b++) put(s, {(prec + (b ? 1 + (b % 3 == 0) : 0)) << 3});
    put(s, {0xFF, 0x90, 0, 10, 0, 0});
    put32(s, 0);  // Psot 0: to the end of the stream
    put(s, {0, 1, 0xFF, 0x93});
    if (hdr) *hdr = s.size();
    s.insert(s.end(), packets.begin(), packets.end());
    put(s, {0xFF, 0xD9});
    return s;
}

// n empty packets, each optionally between an SOP marker segment and an EPH marker
static Bytes empties(int n, bool sop, bool eph) {
    Bytes p;
    for (int k = 0; k < n; k++) {
        if (sop) put(p, {0xFF, 0x91, 0, 4, k >> 8, k & 255});
        put(p, {0});
        if (eph) put(p, {0xFF, 0x92});
    }
    return p;
}

struct Case {
    uint8_t* data;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    Case(int32_t seg_w, int32_t seg_h, int32_t tiled, const std::vector<Bytes>& segs, int32_t flags = PBX_TIFF_F_J2K_PACKETS) {
        offsets.push_back(0);
        for (const Bytes& b : segs) offsets.push_back(offsets.back() + b.size());
        data = new uint8_t[offsets.back() ? offsets.back() : 1];
        for (size_t k = 0; k < segs.size(); k++)
            if (!segs[k].empty()) memcpy(data + offsets[k], segs[k].data(), segs[k].size());
        s = pbx_tiff_segments{seg_w, seg_h, tiled, PBX_TIFF_J2K, 1, flags, data, offsets.data()};
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
        // 40 x 24 gray uint16, 3 levels, 8 x 8 blocks, precincts 2, 4, 8, 16 a side (what an encoder
        // makes of "16 x 16 precincts"), 3 layers.  Resolutions 5 x 3, 10 x 6, 20 x 12, 40 x 24 hold
        // 3 x 2 precincts each: 24 precincts, 72 packets.
        for (int prog = 0; prog < 5; prog++)
            for (int mk = 0; mk < 4; mk++) {
                Case c(40, 24, 0, {stream(40, 24, 1, 16, 3, 3, prog, 3, mk * 2, {1, 2, 3, 4}, empties(72, mk & 1, mk & 2))});
                char what[80];
                snprintf(what, sizeof what, "3 layers, 24 precincts, progression %d, Scod 0x%02x, all empty", prog, mk * 2 | 1);
                expect(what, pbx_test_tiff_j2k_plan(&c.s, 40, 24, PBX_UINT16, 1, 0, 0, out), 0, nullptr);
                if (out[0] != 1 || out[2] != 72) { printf("counts: %llu packets\n", (unsigned long long)out[2]); failures++; }
                std::vector<uint16_t> px(40 * 24, 7);
                expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&c.s, 40, 24, PBX_UINT16, 1, px.data(), 2 * px.size()), 0, nullptr);
                for (uint16_t v : px) if (v != 32768) { printf("sample %u\n", v); failures++; break; }
            }
        // without the flag the same stream is refused by name, as ever
        Case plain(40, 24, 0, {stream(40, 24, 1, 16, 3, 3, 0, 3, 0, {1, 2, 3, 4}, empties(72, false, false))}, 0);
        expect("the flag clear: layers", pbx_test_tiff_j2k_plan(&plain.s, 40, 24, PBX_UINT16, 1, 0, 0, out), 400, "3 quality layers (1)");
        Case prec(40, 24, 0, {stream(40, 24, 1, 16, 3, 3, 0, 1, 0, {1, 2, 3, 4}, empties(24, false, false))}, 0);
        expect("the flag clear: precincts", pbx_test_tiff_j2k_plan(&prec.s, 40, 24, PBX_UINT16, 1, 0, 0, out), 400,
               "more than one precinct in resolution 0");
        Case bits(40, 24, 0, {stream(40, 24, 1, 16, 3, 3, 0, 1, 0, {}, empties(4, false, false))}, 2);
        expect("another flag bit", pbx_test_tiff_j2k_plan(&bits.s, 40, 24, PBX_UINT16, 1, 0, 0, out), 400, "bad flags 0x2");
        // RGB, 64 layers, PPx = PPy = 0 at resolution 0: 1 x 1 precincts of 1 x 1 blocks there
        Case deep(9, 7, 0, {stream(9, 7, 3, 8, 1, 2, 4, 64, 0, {0, 1}, empties(3 * 64 * (5 * 4 + 5 * 4), false, false))});
        expect("64 layers, exponent 0 at resolution 0, CPRL", pbx_test_tiff_j2k_plan(&deep.s, 9, 7, PBX_UINT8, 3, 0, 0, out), 0, nullptr);
        if (out[2] != 3 * 64 * 40) { printf("counts: %llu packets\n", (unsigned long long)out[2]); failures++; }
        std::vector<uint8_t> rgb(9 * 7 * 3, 7);
        expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&deep.s, 9, 7, PBX_UINT8, 3, rgb.data(), rgb.size()), 0, nullptr);
        for (uint8_t v : rgb) if (v != 128) { printf("sample %u\n", v); failures++; break; }
        Case l65(9, 7, 0, {stream(9, 7, 3, 8, 1, 2, 4, 65, 0, {0, 1}, Bytes(8, 0))});
        expect("65 layers", pbx_test_tiff_j2k_plan(&l65.s, 9, 7, PBX_UINT8, 3, 0, 0, out), 400, "65 quality layers (1 .. 64)");
        Case l0(9, 7, 0, {stream(9, 7, 3, 8, 1, 2, 4, 0, 0, {0, 1}, Bytes(8, 0))});
        expect("0 layers", pbx_test_tiff_j2k_plan(&l0.s, 9, 7, PBX_UINT8, 3, 0, 0, out), 400, "0 quality layers (1 .. 64)");
        Case z1(9, 7, 0, {stream(9, 7, 3, 8, 1, 2, 4, 2, 0, {1, 0}, Bytes(8, 0))});
        expect("exponent 0 above resolution 0", pbx_test_tiff_j2k_plan(&z1.s, 9, 7, PBX_UINT8, 3, 0, 0, out), 400,
               "precinct exponent 0 at resolution 1");
    }
    {
        // One 8 x 8 block (no levels, gray 8-bit: Mb = 9), its bytes in several layers.
        // Layer 0: non-empty 1, inclusion 1, zero bit-planes 1 (none), passes 0 (one), Lblock 0 (3),
        // length 010 (2): 1110 0010, then 2 bytes.  Layer 1: non-empty 1, included 1, passes 0,
        // Lblock 0, length 011 (3) and a pad bit: 1100 0110, then 3 bytes.  Layer 2: non-empty 1,
        // included 1, passes 0, Lblock 110 (5), length 10010 (18): 1101 1010 010 + 5 pad bits.
        const Bytes two = {0xE2, 0x12, 0x34, 0xC6, 0x56, 0x78, 0x1A};
        Bytes three = two;
        put(three, {0xDA, 0x40});
        for (int k = 0; k < 18; k++) three.push_back((uint8_t)(0x21 + 7 * k));
        std::vector<uint8_t> px(64);
        Case a(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 0, 2, 0, {}, two)});
        expect("one block, bytes in two layers", pbx_test_tiff_j2k_decode(&a.s, 8, 8, PBX_UINT8, 1, px.data(), 64), 0, nullptr);
        expect("... its plan", pbx_test_tiff_j2k_plan(&a.s, 8, 8, PBX_UINT8, 1, 0, 0, out), 0, nullptr);
        if (out[1] != 1 || out[2] != 2 || out[3] != 2 * 256 + 256) { printf("counts\n"); failures++; }
        Case b(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 1, 3, 0, {}, three)});
        expect("three layers, Lblock grows in the third", pbx_test_tiff_j2k_decode(&b.s, 8, 8, PBX_UINT8, 1, px.data(), 64), 0, nullptr);
        // the same with SOP before the first and third packets only, and EPH after every header
        Bytes marked = {0xFF, 0x91, 0, 4, 0, 0, 0xE2, 0xFF, 0x92, 0x12, 0x34, 0xC6, 0xFF, 0x92, 0x56, 0x78, 0x1A,
                        0xFF, 0x91, 0, 4, 0, 2, 0xDA, 0x40, 0xFF, 0x92};
        marked.insert(marked.end(), three.begin() + 9, three.end());
        std::vector<uint8_t> px2(64);
        Case m(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 1, 3, 6, {}, marked)});
        expect("... with SOP (optional per packet) and EPH", pbx_test_tiff_j2k_decode(&m.s, 8, 8, PBX_UINT8, 1, px2.data(), 64), 0, nullptr);
        if (memcmp(px.data(), px2.data(), 64)) { printf("the markers change the pixels\n"); failures++; }
        Bytes noeph = marked;
        noeph[12] = 0x00;  // the second header's FF92
        Case n(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 1, 3, 6, {}, noeph)});
        expect("a missing EPH", pbx_test_tiff_j2k_decode(&n.s, 8, 8, PBX_UINT8, 1, px2.data(), 64), 400, "decoder code 2");
        // cut inside the third packet's data: the gathered run would pass the stream's end
        Bytes cut(three.begin(), three.end() - 5);
        Case c(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 1, 3, 0, {}, cut)});
        expect("cut inside a later layer's data", pbx_test_tiff_j2k_decode(&c.s, 8, 8, PBX_UINT8, 1, px2.data(), 64), 400, "decoder code 1");
        // passes that overflow only in the sum: 25 passes allowed (Mb = 9), 3 layers x 9 (1111 00011)
        // layer 0: 1 1 1 | 1111 00011 | 0 | 000000 (3 + 3 bits: length 0) ; later: 1 1 | 1111 00011 | 0 | 000000
        const Bytes sum = {0xFE, 0x30, 0x00, 0xFC, 0x60, 0x00, 0xFC, 0x60, 0x00};
        Case s(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 0, 3, 0, {}, sum)});
        expect("passes that overflow only in the sum across layers", pbx_test_tiff_j2k_decode(&s.s, 8, 8, PBX_UINT8, 1, px2.data(), 64), 400,
               "decoder code 3");
        const Bytes fits(sum.begin(), sum.begin() + 6);
        Case f(8, 8, 0, {stream(8, 8, 1, 8, 0, 3, 0, 2, 0, {}, fits)});
        expect("... two of them fit", pbx_test_tiff_j2k_decode(&f.s, 8, 8, PBX_UINT8, 1, px2.data(), 64), 0, nullptr);
    }
    // every prefix of two headers
    int before = failures;
    for (int k = 0; k < 2; k++) {
        size_t hdr = 0;
        const Bytes good = k ? stream(16, 16, 3, 8, 3, 3, 2, 5, 6, {1, 2, 2, 3}, Bytes(12, 0), &hdr)
                             : stream(16, 16, 1, 16, 2, 2, 3, 2, 0, {2, 2, 3}, Bytes(3, 0), &hdr);
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
    // pseudo-random packet bytes under a 3-layer, multi-precinct header
    before = failures;
    uint32_t lcg = 54321, n_ok = 0, n_refused = 0;
    for (int k = 0; k < 400; k++) {
        Bytes junk(16 + k % 300);
        for (uint8_t& v : junk) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
        if (k & 1) junk[0] |= 0xC0;  // a non-empty first packet whose first block is included
        if (k % 7 == 0) for (size_t i = 0; i < junk.size(); i += 3) junk[i] |= 0x80;  // many non-empty packets
        const bool rgb = k % 3 == 0;
        const int levels = k % 4;
        std::vector<int> pp;
        for (int r = 0; r <= levels; r++) pp.push_back(1 + (k / 4 + r) % 5);
        Case c(64, 48, 0, {stream(64, 48, rgb ? 3 : 1, rgb ? 8 : 16, levels, 2 + k % 5, k % 5, 3, (k % 4) * 2, pp, junk)});
        std::vector<uint8_t> px(64 * 48 * (rgb ? 3 : 2));
        const int rc = pbx_test_tiff_j2k_decode(&c.s, 64, 48, rgb ? PBX_UINT8 : PBX_UINT16, rgb ? 3 : 1, px.data(), px.size());
        if (rc == 0) n_ok++;
        else if (rc == 400 && strstr(pbx_last_error(), "corrupt segment stream 0 (j2k, decoder code")) n_refused++;
        else { printf("junk %d: rc %d %s\n", k, rc, pbx_last_error()); failures++; }
    }
    printf("%-66s %s (%u decoded, %u refused)\n", "400 streams of pseudo-random packet bytes, 3 layers, precincts",
           failures != before ? "FAILED" : "ok", n_ok, n_refused);
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
