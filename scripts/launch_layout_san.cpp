// The host half of a decode launch -- LaunchLayout, launch_errors and tiff_codec_check of
// csrc/source_plan.cpp -- under AddressSanitizer / UBSan: a stand-alone program (no Python, no
// device call) linked with source_plan.cpp alone.  Every expected number below is written out by
// hand from the layout source_plan.h states: streams kind by kind in the order of enum ZS_*; checks
// polynomial by polynomial, within one the ranges shorter than the split length before the others,
// each group in the plan's order; JPEG 2000 segments with J2_SEG_CHROMA after the others; err[] =
// streams, checks, JPEG streams, JPEG 2000 streams.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/ (this file and csrc/source_plan.cpp
// compiled with the sanitizers by g++ alone); tests/test_launch_layout_host.py builds it plain.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../omero-ms-pixel-buffer_amd/csrc/source_plan.h"

using namespace pbx;

static int failures = 0;

static void check(const char* what, bool ok) {
    printf("%-66s %s\n", what, ok ? "ok" : "UNEXPECTED");
    if (!ok) failures++;
}

// rc and the whole message
static void expect(const char* what, int rc, int want_rc, const char* want_msg) {
    const char* err = pbx_last_error();
    const bool ok = rc == want_rc && (!want_msg || !strcmp(err, want_msg));
    printf("%-66s rc %3d %s%s\n", what, rc, ok ? "ok" : "UNEXPECTED: ", ok ? "" : err);
    if (!ok) failures++;
}

template <size_t N>
static bool same(const uint32_t (&got)[N], std::initializer_list<uint32_t> want) {
    return want.size() == N && std::equal(want.begin(), want.end(), got);
}

int main() {
    // ---------------------------------------------------------------- the layout
    ZarrPlan P;
    // 2 zlib, 1 zstd, 3 gzip streams; dst_off names them
    P.kind[ZS_GZIP] = {ZStream{0, 103, 1, 1, ZS_GZIP, 0}, ZStream{0, 104, 1, 1, ZS_GZIP, 0}, ZStream{0, 105, 1, 1, ZS_GZIP, 0}};
    P.kind[ZS_ZLIB] = {ZStream{0, 100, 1, 1, ZS_ZLIB, 0}, ZStream{0, 101, 1, 1, ZS_ZLIB, 0}};
    P.kind[ZS_ZSTD] = {ZStream{0, 102, 1, 1, ZS_ZSTD, 0}};
    // CRC-32 ranges either side of a split length of 1000 (1000 itself is long), one CRC-32C range
    P.checks[ZK_CRC32] = {ZCheck{0, 2000, 0xA0, ZK_SCRATCH, ZK_CRC32}, ZCheck{0, 10, 0xA1, ZK_SCRATCH, ZK_CRC32},
                          ZCheck{0, 1000, 0xA2, ZK_SCRATCH, ZK_CRC32}, ZCheck{0, 999, 0xA3, ZK_SCRATCH, ZK_CRC32}};
    P.checks[ZK_CRC32C] = {ZCheck{0, 5, 0xC0, ZK_INPUT, ZK_CRC32C}};
    P.jstreams.resize(2);
    P.jsegs.resize(2);
    P.j2streams.resize(3);
    P.j2segs.resize(3);
    for (uint32_t k = 0; k < 3; k++) {
        memset(&P.j2segs[k], 0, sizeof(TJ2Seg));
        P.j2segs[k].x0 = (int32_t)k;  // names it
        P.j2segs[k].rct = 1;
    }
    P.j2segs[1].rct |= J2_SEG_XS2;  // the middle one: k_tiff_j2k_place_chroma's
    P.j2blocks.resize(5);
    P.j2cons = 7;
    P.j2nodes = 11;
    const LaunchLayout L(P, 1000);
    check("counts by kind", same(L.counts, {0, 2, 0, 0, 1, 3, 0, 0}));
    bool order = L.streams.size() == 6;
    for (size_t k = 0; order && k < 6; k++) order = L.streams[k].dst_off == 100 + k;
    check("streams: zlib, zstd, gzip, each kind in the plan's order", order);
    bool cks = L.checks.size() == 5;
    const uint32_t want_expect[5] = {0xA1, 0xA3, 0xA0, 0xA2, 0xC0};
    for (size_t k = 0; cks && k < 5; k++) cks = L.checks[k].expect == want_expect[k];
    check("checks: CRC-32 short, CRC-32 long, CRC-32C", cks);
    check("ck_first", same(L.ck_first, {0, 4}));
    check("ck_wave", same(L.ck_wave, {2, 1}));
    check("ck_n", same(L.ck_n, {4, 1}));
    check("J2K segments: 0, 2, then the chroma one",
          L.j2segs.size() == 3 && L.j2segs[0].x0 == 0 && L.j2segs[1].x0 == 2 && L.j2segs[2].x0 == 1);
    check("one chroma segment", L.j2chroma == 1);
    check("the plan's own segment order is untouched", P.j2segs[1].x0 == 1);
    check("j2meta = 24 * 5 + 16 * 7 + 4 * 11", L.j2meta == 276);
    check("nstreams, nchecks, njpeg, nj2", L.nstreams == 6 && L.nchecks == 5 && L.njpeg == 2 && L.nj2 == 3);
    check("err[] bases 0, 6, 11, 13 and nerr 16",
          L.err_streams == 0 && L.err_checks == 6 && L.err_jpeg == 11 && L.err_j2k == 13 && L.nerr == 16);
    {
        const LaunchLayout E(ZarrPlan(), 1000);
        check("an empty plan", E.nerr == 0 && E.streams.empty() && E.checks.empty() && E.j2chroma == 0 && E.j2meta == 0 &&
                                   same(E.ck_n, {0, 0}));
    }

    // ---------------------------------------------------------------- launch_errors
    std::vector<uint32_t> err(17, 0);
    expect("nothing reported", launch_errors(L, err.data()), 0, nullptr);
    auto one = [&](const char* what, uint32_t at, uint32_t code, const char* msg) {
        err.assign(17, 0);
        err[at] = code;
        expect(what, launch_errors(L, err.data()), 400, msg);
    };
    one("stream 1: the second zlib", 1, 7, "corrupt chunk stream 1 (zlib, decoder code 7)");
    one("stream 2: the zstd", 2, 37, "corrupt chunk stream 2 (zstd, decoder code 37)");
    one("stream 4: the second gzip", 4, 9, "corrupt chunk stream 4 (gzip, decoder code 9)");
    one("check 3: the CRC-32 range of 1000 bytes", 6 + 3, 40,
        "chunk checksum mismatch: the gzip CRC-32 of 1000 bytes is not 0x000000a2");
    one("check 1: the CRC-32 range of 999 bytes", 6 + 1, 40,
        "chunk checksum mismatch: the gzip CRC-32 of 999 bytes is not 0x000000a3");
    one("check 4: the CRC-32C range", 6 + 4, 40, "chunk checksum mismatch: the crc32c of 5 bytes is not 0x000000c0");
    one("JPEG stream 1, code 1", 11 + 1, 1,
        "corrupt segment stream 1 (jpeg, decoder code 1: entropy data ends before the last MCU)");
    one("JPEG stream 1, code 2", 11 + 1, 2, "corrupt segment stream 1 (jpeg, decoder code 2: a code that is in no table)");
    one("JPEG stream 1, code 3", 11 + 1, 3,
        "corrupt segment stream 1 (jpeg, decoder code 3: a run that passes coefficient 63)");
    one("JPEG stream 1, code 4", 11 + 1, 4,
        "corrupt segment stream 1 (jpeg, decoder code 4: a DC size > 11 or an AC size > 10)");
    one("JPEG stream 1, code 5", 11 + 1, 5,
        "corrupt segment stream 1 (jpeg, decoder code 5: a restart marker missing, out of sequence or misplaced)");
    one("JPEG stream 1, a code without a reason", 11 + 1, 6, "corrupt segment stream 1 (jpeg, decoder code 6: ?)");
    one("J2K stream 2", 13 + 2, 3, "corrupt segment stream 2 (j2k, decoder code 3)");
    err.assign(17, 0);
    err[4] = 9;
    err[11 + 1] = 1;
    expect("a stream and a JPEG stream: the stream", launch_errors(L, err.data()), 400,
           "corrupt chunk stream 4 (gzip, decoder code 9)");
    err.assign(17, 0);
    err[13 + 1] = 2;
    err[6 + 4] = 40;
    expect("a check and a J2K stream: the check", launch_errors(L, err.data()), 400,
           "chunk checksum mismatch: the crc32c of 5 bytes is not 0x000000c0");
    err.assign(17, 0);
    err[13 + 1] = 2;
    err[11] = 5;
    expect("a JPEG and a J2K stream: the JPEG one", launch_errors(L, err.data()), 400,
           "corrupt segment stream 0 (jpeg, decoder code 5: a restart marker missing, out of sequence or misplaced)");
    err.assign(17, 0);
    err[16] = 1;  // the dword past nerr is not a report
    expect("the spare dword", launch_errors(L, err.data()), 0, nullptr);

    // ---------------------------------------------------------------- tiff_codec_check
    const uint8_t data[1] = {0};
    const uint64_t offsets[2] = {0, 1};
    const pbx_tiff_segments lzw{16, 16, 1, PBX_TIFF_LZW, 1, 0, data, offsets};
    const pbx_tiff_segments jps{16, 16, 1, PBX_TIFF_JPEG, 1, 0, data, offsets};
    const pbx_tiff_segments j2s{16, 16, 1, PBX_TIFF_J2K, 1, 0, data, offsets};
    const pbx_tiff_jpeg tabs{nullptr, 0, 1, 0};
    expect("LZW tiles on uint16", tiff_codec_check(TiffCodec{&lzw, nullptr, false}, PBX_UINT16, 1, 0, 7), 0, nullptr);
    expect("YCbCr JPEG tiles, sample 2 of 3", tiff_codec_check(TiffCodec{&jps, &tabs, false}, PBX_UINT8, 3, 2, 7), 0, nullptr);
    expect("JPEG 2000 tiles on uint16", tiff_codec_check(TiffCodec{&j2s, nullptr, true}, PBX_UINT16, 1, 0, 7), 0, nullptr);
    {
        pbx_tiff_segments s = lzw;
        s.seg_w = 0;
        expect("a segment 0 wide", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_UINT16, 1, 0, 7), 400,
               "bad segment shape 0 x 16");
        s = lzw;
        s.predictor = 2;
        expect("predictor 2 on float", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_FLOAT, 1, 0, 7), 400,
               "plane 7: predictor 2 on floating-point samples");
        expect("predictor 2 on uint16", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_UINT16, 1, 0, 7), 0, nullptr);
        s.predictor = 3;
        expect("predictor 3 on int32", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_INT32, 1, 0, 7), 400,
               "bad predictor 3 (the floating-point predictor) on a plane of integer samples");
        expect("predictor 3 on float", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_FLOAT, 1, 0, 7), 0, nullptr);
        expect("sample 3 of 3", tiff_codec_check(TiffCodec{&lzw, nullptr, false}, PBX_UINT16, 3, 3, 7), 400,
               "sample 3 outside segments of 3 samples per pixel");
    }
    expect("JPEG tiles on uint16", tiff_codec_check(TiffCodec{&jps, &tabs, false}, PBX_UINT16, 3, 0, 7), 400,
           "JPEG segments on a plane that is not uint8");
    expect("JPEG 2000 tiles on int32", tiff_codec_check(TiffCodec{&j2s, nullptr, true}, PBX_INT32, 1, 0, 7), 400,
           "JPEG 2000 segments on a plane that is neither uint8 nor uint16");
    expect("LZW tiles through the JPEG 2000 calls", tiff_codec_check(TiffCodec{&lzw, nullptr, true}, PBX_UINT16, 1, 0, 7), 400,
           "bad compression 5 (the JPEG 2000 calls take 34712)");
    // two defects at once: the codec's own check, then the predictor, then the sample
    {
        pbx_tiff_segments s = lzw;
        s.predictor = 2;
        expect("predictor 2 on float and sample 3 of 3", tiff_codec_check(TiffCodec{&s, nullptr, false}, PBX_FLOAT, 3, 3, 9), 400,
               "plane 9: predictor 2 on floating-point samples");
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
