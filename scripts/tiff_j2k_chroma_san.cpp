// Subsampled chroma and YCbCr components of JPEG 2000 segments (PBX_TIFF_F_J2K_SUBSAMPLED,
// PBX_TIFF_F_J2K_YCBCR) under AddressSanitizer / UBSan: the planner's per-component sizes and
// packet list (pbx_test_tiff_j2k_plan) and the CPU decode hook (pbx_test_tiff_j2k_decode), which
// runs the device's walker, tier 1, the inverse wavelets on each component's own planes and the
// placement's replication and conversion (j2k_chroma_at and j2k_ycc_rgb of csrc/tiff_j2k_dev.h), every
// table and plane in a heap block of exactly its planned size.  A stand-alone program: no Python,
// no device call, nothing preloaded.  Every segment lies in a heap block of exactly its own bytes.
// The streams are built here: hand-built subsampled headers over packets that are all empty, the
// refusals, every prefix of one header, and pseudo-random packet bytes under a 4:2:0
// multi-precinct header, which decode to garbage or are refused.
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

struct Comp {
    int xr, yr;
};

// A w x h codestream of 8-bit components with the sampling factors `comps`: `layers`, Scod bits
// `scod` (2 SOP, 4 EPH), precinct exponents pp (PPx = PPy, one per resolution; empty: none
// declared), code blocks of 2^cb x 2^cb, 5/3 (style-0 QCD) or 9/7 (style-2 QCD).
static Bytes stream(int w, int h, const std::vector<Comp>& comps, int levels, int cb, int prog, int layers, int scod, int mct,
                    bool irrev, const std::vector<int>& pp, const Bytes& packets, size_t* hdr = nullptr) {
    Bytes s;
    const int nc = (int)comps.size();
    put(s, {0xFF, 0x4F, 0xFF, 0x51, 0, 38 + 3 * nc, 0, 0});
    put32(s, w); put32(s, h); put32(s, 0); put32(s, 0); put32(s, w); put32(s, h); put32(s, 0); put32(s, 0);
    put(s, {0, nc});
    for (const Comp& c : comps) put(s, {7, c.xr, c.yr});
    put(s, {0xFF, 0x52, 0, 12 + (int)pp.size(), scod | (pp.empty() ? 0 : 1), prog, layers >> 8, layers & 255, mct, levels,
            cb - 2, cb - 2, 0, irrev ? 0 : 1});
    for (int e : pp) put(s, {e | e << 4});
    const int nb = 3 * levels + 1;
    if (irrev) {
        put(s, {0xFF, 0x5C, 0, 3 + 2 * nb, 2 << 5 | 2});
        for (int b = 0; b < nb; b++) put(s, {(8 + (b ? 1 + (b % 3 == 0) : 0)) << 3 | 1, 0x23});
    } else {
        put(s, {0xFF, 0x5C, 0, 3 + nb, 2 << 5});
        for (int b = 0; b < nb; b++) put(s, {(8 + (b ? 1 + (b % 3 == 0) : 0)) << 3});
    }
    put(s, {0xFF, 0x90, 0, 10, 0, 0});
    put32(s, 0);  // Psot 0: to the end of the stream
    put(s, {0, 1, 0xFF, 0x93});
    if (hdr) *hdr = s.size();
    s.insert(s.end(), packets.begin(), packets.end());
    put(s, {0xFF, 0xD9});
    return s;
}

static const std::vector<Comp> C420 = {{1, 1}, {2, 2}, {2, 2}}, C422 = {{1, 1}, {2, 1}, {2, 1}}, C440 = {{1, 1}, {1, 2}, {1, 2}};

struct Case {
    uint8_t* data;
    std::vector<uint64_t> offsets;
    pbx_tiff_segments s;
    Case(int32_t seg_w, int32_t seg_h, int32_t tiled, const std::vector<Bytes>& segs, int32_t flags) {
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
    printf("%-72s rc %3d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED: ", ok ? "" : err);
    if (!ok) failures++;
}

static int cdiv(int a, int b) { return (a + b - 1) / b; }

// the packets of a w x h stream of three components: per component and resolution the precinct grid
static int packets_of(int w, int h, const std::vector<Comp>& comps, int levels, const std::vector<int>& pp, int layers) {
    int n = 0;
    for (const Comp& c : comps)
        for (int r = 0; r <= levels; r++) {
            const int rw = cdiv(cdiv(w, c.xr), 1 << (levels - r)), rh = cdiv(cdiv(h, c.yr), 1 << (levels - r));
            const int e = pp.empty() ? 15 : pp[r];
            n += cdiv(rw, 1 << e) * cdiv(rh, 1 << e);
        }
    return n * layers;
}

int main() {
    const int SUB = PBX_TIFF_F_J2K_SUBSAMPLED, YCC = PBX_TIFF_F_J2K_YCBCR, PK = PBX_TIFF_F_J2K_PACKETS;
    uint64_t out[4];
    {
        // 37 x 23 (odd: the chroma rounds up to 19 and 12), all packets empty: every sample decodes
        // to the level shift, 128, and with the conversion to RGB (128, 128, 128)
        const std::vector<Comp>* all[3] = {&C422, &C440, &C420};
        for (int k = 0; k < 3; k++)
            for (int prog = 0; prog < 5; prog++)
                for (int irr = 0; irr < 2; irr++) {
                    const std::vector<int> pp = {1, 2, 3, 4};
                    const int npk = packets_of(37, 23, *all[k], 3, pp, 2);
                    Case c(37, 23, 0, {stream(37, 23, *all[k], 3, 3, prog, 2, 0, 0, irr, pp, Bytes(npk, 0))}, PK | SUB | YCC);
                    char what[96];
                    snprintf(what, sizeof what, "37 x 23, factors %d x %d, progression %d, %s, %d empty packets", (*all[k])[1].xr,
                             (*all[k])[1].yr, prog, irr ? "9/7" : "5/3", npk);
                    expect(what, pbx_test_tiff_j2k_plan(&c.s, 37, 23, PBX_UINT8, 3, 0, 0, out), 0, nullptr);
                    if (out[0] != 1 || out[2] != (uint64_t)npk) { printf("counts: %llu packets\n", (unsigned long long)out[2]); failures++; }
                    std::vector<uint8_t> px(37 * 23 * 3, 7);
                    expect("... decoded on the CPU", pbx_test_tiff_j2k_decode(&c.s, 37, 23, PBX_UINT8, 3, px.data(), px.size()), 0, nullptr);
                    for (uint8_t v : px) if (v != 128) { printf("sample %u\n", v); failures++; break; }
                }
        // scratch: two dword planes per component of the component's own size, each rounded up to 256
        Case one(37, 23, 0, {stream(37, 23, C420, 0, 4, 0, 1, 0, 0, false, {}, Bytes(3, 0))}, SUB);
        expect("4:2:0 without levels: the plan", pbx_test_tiff_j2k_plan(&one.s, 37, 23, PBX_UINT8, 3, 0, 0, out), 0, nullptr);
        const uint64_t luma = (37 * 23 * 4 + 255) & ~255, chroma = (19 * 12 * 4 + 255) & ~255;
        if (out[3] != 2 * luma + 4 * chroma) { printf("scratch %llu\n", (unsigned long long)out[3]); failures++; }
        // the refusals, by name
        struct {
            const char* what;
            std::vector<Comp> comps;
            int mct, flags;
            const char* text;
        } bad[] = {
            {"the flag clear", C420, 0, 0, "subsampled components (component 1: 2 x 2)"},
            {"the flag clear, packets", C420, 0, PK, "subsampled components (component 1: 2 x 2)"},
            {"the flag clear, YCbCr", C420, 0, YCC, "subsampled components (component 1: 2 x 2)"},
            {"4 x 1", {{1, 1}, {4, 1}, {4, 1}}, 0, SUB, "sampling factors 4 x 1 on component 1 (2 x 1, 1 x 2 or 2 x 2)"},
            {"2 x 3", {{1, 1}, {2, 3}, {2, 3}}, 0, SUB, "sampling factors 2 x 3 on component 1 (2 x 1, 1 x 2 or 2 x 2)"},
            {"0 x 1", {{1, 1}, {0, 1}, {0, 1}}, 0, SUB, "sampling factors 0 x 1 on component 1"},
            {"a subsampled first component", {{2, 2}, {2, 2}, {2, 2}}, 0, SUB, "subsampled first component (2 x 2)"},
            {"chroma components that differ", {{1, 1}, {2, 1}, {2, 2}}, 0, SUB, "chroma components of different sampling factors (2 x 1 and 2 x 2)"},
            {"the third component alone", {{1, 1}, {1, 1}, {2, 2}}, 0, SUB, "chroma components of different sampling factors (1 x 1 and 2 x 2)"},
            {"subsampling with MCT 1", C420, 1, SUB, "subsampled components (2 x 2) with the multiple-component transform"},
            {"YCbCr with MCT 1", {{1, 1}, {1, 1}, {1, 1}}, 1, YCC, "YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on a stream with the multiple-component transform"},
            {"another flag bit", C420, 0, SUB | 2, "bad flags 0x6"},
        };
        for (auto& b : bad) {
            Case c(16, 16, 1, {stream(16, 16, b.comps, 1, 3, 0, 1, 0, b.mct, false, {}, Bytes(6, 0))}, b.flags);
            expect(b.what, pbx_test_tiff_j2k_plan(&c.s, 16, 16, PBX_UINT8, 3, 0, 0, out), 400, b.text);
        }
        Case mono(16, 16, 1, {stream(16, 16, {{2, 1}}, 1, 3, 0, 1, 0, 0, false, {}, Bytes(2, 0))}, SUB);
        expect("subsampling on a one-component stream", pbx_test_tiff_j2k_plan(&mono.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400,
               "subsampling on a stream of one component (2 x 1)");
        Case mono8(16, 16, 1, {stream(16, 16, {{1, 1}}, 1, 3, 0, 1, 0, 0, false, {}, Bytes(2, 0))}, YCC);
        expect("YCbCr on one sample per pixel", pbx_test_tiff_j2k_plan(&mono8.s, 16, 16, PBX_UINT8, 1, 0, 0, out), 400,
               "YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on JPEG 2000 segments of 1 sample(s) per pixel");
    }
    // every prefix of one header
    int before = failures;
    {
        size_t hdr = 0;
        const Bytes good = stream(16, 16, C420, 3, 3, 2, 5, 6, 0, true, {1, 2, 2, 3}, Bytes(12, 0), &hdr);
        for (size_t cut = 0; cut < hdr; cut++) {
            Case c(16, 16, 1, {Bytes(good.begin(), good.begin() + cut)}, PK | SUB | YCC);
            const int rc = pbx_test_tiff_j2k_plan(&c.s, 16, 16, PBX_UINT8, 3, 0, 0, out);
            if (rc != 400) { printf("header prefix of %zu bytes: rc %d\n", cut, rc); failures++; }
        }
        Case whole(16, 16, 1, {Bytes(good.begin(), good.begin() + hdr)}, PK | SUB | YCC);
        expect("a header with no packet after it: the plan stands", pbx_test_tiff_j2k_plan(&whole.s, 16, 16, PBX_UINT8, 3, 0, 0, out), 0,
               nullptr);
        std::vector<uint8_t> px(16 * 16 * 3);
        expect("... and the decoder says what is missing", pbx_test_tiff_j2k_decode(&whole.s, 16, 16, PBX_UINT8, 3, px.data(), px.size()),
               400, "corrupt segment stream 0 (j2k, decoder code 1)");
    }
    printf("%-72s %s\n", "every prefix of a subsampled header is refused", failures != before ? "FAILED" : "ok");
    // pseudo-random packet bytes under a 4:2:0 (every third: 4:2:2, 4:4:0), multi-precinct header
    before = failures;
    uint32_t lcg = 97531, n_ok = 0, n_refused = 0;
    for (int k = 0; k < 400; k++) {
        Bytes junk(16 + k % 300);
        for (uint8_t& v : junk) { lcg = lcg * 1664525u + 1013904223u; v = (uint8_t)(lcg >> 24); }
        if (k & 1) junk[0] |= 0xC0;  // a non-empty first packet whose first block is included
        if (k % 7 == 0) for (size_t i = 0; i < junk.size(); i += 3) junk[i] |= 0x80;  // many non-empty packets
        const int levels = k % 4;
        std::vector<int> pp;
        for (int r = 0; r <= levels; r++) pp.push_back(1 + (k / 4 + r) % 5);
        const std::vector<Comp>& f = k % 3 == 0 ? C420 : k % 3 == 1 ? C422 : C440;
        const int w = 61 + k % 4, h = 45 + k % 3;
        Case c(w, h, 0, {stream(w, h, f, levels, 2 + k % 5, k % 5, 1 + k % 3, (k % 4) * 2, 0, k % 2, pp, junk)},
               PK | SUB | (k % 5 < 3 ? YCC : 0));
        std::vector<uint8_t> px((size_t)w * h * 3);
        const int rc = pbx_test_tiff_j2k_decode(&c.s, w, h, PBX_UINT8, 3, px.data(), px.size());
        if (rc == 0) n_ok++;
        else if (rc == 400 && strstr(pbx_last_error(), "corrupt segment stream 0 (j2k, decoder code")) n_refused++;
        else { printf("junk %d: rc %d %s\n", k, rc, pbx_last_error()); failures++; }
    }
    printf("%-72s %s (%u decoded, %u refused)\n", "400 streams of pseudo-random packet bytes, subsampled, precincts",
           failures != before ? "FAILED" : "ok", n_ok, n_refused);
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
