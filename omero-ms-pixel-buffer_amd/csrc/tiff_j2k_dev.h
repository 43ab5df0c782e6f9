// tiff_j2k_dev.h — the serial halves of the JPEG 2000 decoder (kernels_tiff_j2k.hip; DESIGN.md
// §10b "JPEG 2000 segments"): the packet-header parser of tier 2 and the bit-plane decoder of
// tier 1, each run by one lane.  Plain C++ over pointers, so that the very same text also runs
// on the host: pbx_test_tiff_j2k_decode (source_plan.cpp, built by the host compiler without HIP)
// decodes with it on the CPU, each block's state in heap blocks of exactly the kernel's LDS sizes,
// which is how the tests without a GPU and the sanitizer run of scripts/tiff_j2k_plan_san.cpp
// reach this code.
//
// Safety.  Every index below comes from the planner's geometry (J2Packet, J2Band, J2Block), never
// from the stream: code-block bytes steer decisions and values, not addresses.  The exceptions are
// checked where they are read: a run-length position is two bits inside a full stripe of four
// rows, and a code block's offsets and lengths (in the packets, and in the gather area of a stream
// of several layers) are compared with the stream's length before they are stored (j2k_packets)
// and again before they are used (j2k_gather_span, j2k_code_bytes).
#pragma once
#include <stdint.h>

#include "pbx_decode_types.h"

#define PBX_J2K_FN PBX_HD

namespace pbx {

// T.800 table C.2, packed: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
#define PBX_MQ(qe, nm, nl, sw) ((uint32_t)(qe) | (uint32_t)(nm) << 16 | (uint32_t)(nl) << 22 | (uint32_t)(sw) << 28)
constexpr uint32_t J2_MQ_STATES = 47;
#define PBX_MQ_TABLE                                                                                                  \
    PBX_MQ(0x5601, 1, 1, 1), PBX_MQ(0x3401, 2, 6, 0), PBX_MQ(0x1801, 3, 9, 0), PBX_MQ(0x0AC1, 4, 12, 0),             \
    PBX_MQ(0x0521, 5, 29, 0), PBX_MQ(0x0221, 38, 33, 0), PBX_MQ(0x5601, 7, 6, 1), PBX_MQ(0x5401, 8, 14, 0),          \
    PBX_MQ(0x4801, 9, 14, 0), PBX_MQ(0x3801, 10, 14, 0), PBX_MQ(0x3001, 11, 17, 0), PBX_MQ(0x2401, 12, 18, 0),       \
    PBX_MQ(0x1C01, 13, 20, 0), PBX_MQ(0x1601, 29, 21, 0), PBX_MQ(0x5601, 15, 14, 1), PBX_MQ(0x5401, 16, 14, 0),      \
    PBX_MQ(0x5101, 17, 15, 0), PBX_MQ(0x4801, 18, 16, 0), PBX_MQ(0x3801, 19, 17, 0), PBX_MQ(0x3401, 20, 18, 0),      \
    PBX_MQ(0x3001, 21, 19, 0), PBX_MQ(0x2801, 22, 19, 0), PBX_MQ(0x2401, 23, 20, 0), PBX_MQ(0x2201, 24, 21, 0),      \
    PBX_MQ(0x1C01, 25, 22, 0), PBX_MQ(0x1801, 26, 23, 0), PBX_MQ(0x1601, 27, 24, 0), PBX_MQ(0x1401, 28, 25, 0),      \
    PBX_MQ(0x1201, 29, 26, 0), PBX_MQ(0x1101, 30, 27, 0), PBX_MQ(0x0AC1, 31, 28, 0), PBX_MQ(0x09C1, 32, 29, 0),      \
    PBX_MQ(0x08A1, 33, 30, 0), PBX_MQ(0x0521, 34, 31, 0), PBX_MQ(0x0441, 35, 32, 0), PBX_MQ(0x02A1, 36, 33, 0),      \
    PBX_MQ(0x0221, 37, 34, 0), PBX_MQ(0x0141, 38, 35, 0), PBX_MQ(0x0111, 39, 36, 0), PBX_MQ(0x0085, 40, 37, 0),      \
    PBX_MQ(0x0049, 41, 38, 0), PBX_MQ(0x0025, 42, 39, 0), PBX_MQ(0x0015, 43, 40, 0), PBX_MQ(0x0009, 44, 41, 0),      \
    PBX_MQ(0x0005, 45, 42, 0), PBX_MQ(0x0001, 45, 43, 0), PBX_MQ(0x5601, 46, 46, 0)

// ------------------------------------------------------------------------------ tier 2
// Packet-header bits (T.800 B.10.1): after an FF byte the next byte gives 7 bits.  Past the
// stream's end the reader answers zeros and sets err, which ends every loop below.
struct J2Bits {
    const uint8_t* d;
    uint32_t pos, end, buf, ct, err;
};

PBX_J2K_FN uint32_t j2bit(J2Bits& s) {
    if (s.ct == 0) {
        if (s.pos >= s.end) {
            s.err = J2E_END;
            return 0;
        }
        s.ct = s.buf == 0xFF ? 7 : 8;
        s.buf = s.d[s.pos++];
    }
    s.ct--;
    return (s.buf >> s.ct) & 1u;
}

// Tag-tree decoding (B.10.2) of leaf (bx, by) of a precinct's window against `threshold`: is its
// value below it?  A node is one dword, its lower bound | (its value + 1, 0 while unknown) << 16,
// zero before the first packet.  Level l holds ceil(nx / 2^l) x ceil(ny / 2^l) nodes, the leaves
// first.
PBX_J2K_FN bool j2tag(J2Bits& s, uint32_t* tree, const J2Window& W, uint32_t bx, uint32_t by, uint32_t threshold) {
    uint32_t low = 0, off = W.nodes, val = 0;
    for (uint32_t l = W.tlevels; l-- > 0;) {
        const uint32_t wl = (W.nx + (1u << l) - 1) >> l, hl = (W.ny + (1u << l) - 1) >> l;
        off -= wl * hl;
        const uint32_t i = off + (by >> l) * wl + (bx >> l);
        const uint32_t node = tree[i];
        const uint32_t nlow = node & 0xffffu;
        val = node >> 16;
        if (low < nlow) low = nlow;
        while (low < threshold && (val == 0 || low < val - 1)) {
            if (j2bit(s)) val = low + 1; else low++;
        }
        tree[i] = val << 16 | low;
    }
    return val != 0 && val - 1 < threshold;
}

// The packets of one stream, in the order of its packet list: code[] of its included blocks (the
// others stay zero: never included, coefficients zero), their passes and bytes summed over the
// layers.  walk[] (zero at the start) keeps a block's Lblock and its count of contributions from
// layer to layer.  In a stream of several layers every contribution of at least one byte is also
// written down in con[] (S.ncon entries from S.con0, zero at the start); at the end a block with
// more than one gets its run in the stream's gather area (J2C_GATHERED, a prefix over the stream's
// blocks), and the entries of the others are cleared: those blocks are read where they lie.
// Returns 0 or the device error code.
PBX_J2K_FN uint32_t j2k_packets(const J2Stream& S, const J2Packet* packets, const J2Band* bands, const uint8_t* src,
                                uint32_t* tt, J2Code* code, J2Walk* walk, J2Contrib* con) {
    J2Bits s{src + S.src_off, 0, S.len, 0, 0, 0};
    uint32_t ncon = 0;
    for (uint32_t p = 0; p < S.npk; p++) {
        const J2Packet& K = packets[S.pk0 + p];
        const uint32_t nbn = K.nbands <= 3 ? K.nbands : 3, layer = K.layer;
        // B.10.1 with Scod bit 1: FF91, Lsop = 4, Nsop (not verified) may stand before the header
        if ((S.mode & J2S_SOP) && s.end - s.pos >= 6 && s.d[s.pos] == 0xFF && s.d[s.pos + 1] == 0x91) s.pos += 6;
        s.ct = 0;
        s.buf = 0;
        const uint32_t nonempty = j2bit(s);
        if (s.err) return s.err;
        for (uint32_t k = 0; k < nbn && nonempty; k++) {
            const J2Band B = bands[K.band + k];
            const J2Window W = K.win[k];
            for (uint32_t by = 0; by < W.ny; by++)
                for (uint32_t bx = 0; bx < W.nx; bx++) {
                    const uint32_t bi = B.blk0 + (W.y0 + by) * B.nbx + W.x0 + bx;
                    J2Code C = code[bi];
                    if (!C.passes) {  // not yet included: the inclusion tree, then the zero bit-planes
                        const bool incl = j2tag(s, tt + W.tt, W, bx, by, layer + 1);
                        if (s.err) return s.err;
                        if (!incl) continue;
                        uint32_t z = 1;
                        while (!j2tag(s, tt + W.tt + W.nodes, W, bx, by, z)) {
                            if (s.err) return s.err;
                            if (++z > B.mb + 1) return J2E_PLANES;
                        }
                        C.zbp = z - 1;
                    } else {
                        const uint32_t incl = j2bit(s);
                        if (s.err) return s.err;
                        if (!incl) continue;
                    }
                    uint32_t n;
                    if (!j2bit(s)) n = 1;
                    else if (!j2bit(s)) n = 2;
                    else {
                        n = j2bit(s) << 1;
                        n |= j2bit(s);
                        if (n < 3) n += 3;
                        else {
                            n = 0;
                            for (int i = 0; i < 5; i++) n = n << 1 | j2bit(s);
                            if (n < 31) n += 6;
                            else {
                                n = 0;
                                for (int i = 0; i < 7; i++) n = n << 1 | j2bit(s);
                                n += 37;
                            }
                        }
                    }
                    if (s.err) return s.err;
                    C.passes += n;  // (at most 164 a packet, 64 packets: no overflow)
                    if ((int32_t)C.passes > 3 * ((int32_t)B.mb - (int32_t)C.zbp) - 2) return J2E_PLANES;
                    // one codeword segment (code-block style 0): Lblock + floor(log2(passes added)) bits
                    J2Walk& K2 = walk[bi];
                    uint32_t lb = K2.lblock & 0xffu;
                    uint32_t nbits = 3 + lb + (31u - (uint32_t)__builtin_clz(n));
                    while (j2bit(s)) {
                        lb++;
                        if (++nbits > 32) return J2E_HEADER;
                    }
                    if (nbits > 32) return J2E_HEADER;
                    uint32_t len = 0;
                    for (uint32_t i = 0; i < nbits; i++) len = len << 1 | j2bit(s);
                    if (s.err) return s.err;
                    if (len > S.len) return J2E_END;
                    K2.lblock = (K2.lblock & ~0xffu) | lb;
                    K2.pend = len + 1;
                    code[bi] = C;
                }
        }
        if (s.buf == 0xFF) s.pos++;  // the stuffed byte after a header that ends in FF
        if (s.pos > s.end) return J2E_END;
        if (S.mode & J2S_EPH) {
            if (s.end - s.pos < 2 || s.d[s.pos] != 0xFF || s.d[s.pos + 1] != 0x92) return J2E_HEADER;  // no EPH
            s.pos += 2;
        }
        for (uint32_t k = 0; k < nbn && nonempty; k++) {
            const J2Band B = bands[K.band + k];
            const J2Window W = K.win[k];
            for (uint32_t by = 0; by < W.ny; by++)
                for (uint32_t bx = 0; bx < W.nx; bx++) {
                    const uint32_t bi = B.blk0 + (W.y0 + by) * B.nbx + W.x0 + bx;
                    J2Walk& K2 = walk[bi];
                    if (!K2.pend) continue;
                    const uint32_t len = K2.pend - 1;
                    K2.pend = 0;
                    if (!len) continue;
                    if (len > s.end - s.pos) return J2E_END;
                    J2Code& C = code[bi];
                    if (C.len > S.len - len) return J2E_END;  // (packets do not overlap: cannot be)
                    if (!C.len) C.off = s.pos;
                    if (S.layers > 1) {
                        if (ncon >= S.ncon) return J2E_HEADER;  // (one a block and layer: cannot be)
                        con[S.con0 + ncon++] = J2Contrib{bi, s.pos, len, C.len};
                    }
                    K2.lblock += 1u << 8;
                    C.len += len;
                    s.pos += len;
                }
        }
    }
    if (S.layers > 1) {
        uint32_t run = 0;
        for (uint32_t bi = S.blk0; bi < S.blk0 + S.nblk; bi++)
            if ((walk[bi].lblock >> 8) > 1) {
                J2Code& C = code[bi];
                if (C.len > S.len - run) return J2E_END;  // (the runs are disjoint parts of the stream)
                C.off = run | J2C_GATHERED;
                run += C.len;
            }
        for (uint32_t i = 0; i < ncon; i++) {
            J2Contrib& G = con[S.con0 + i];
            if ((walk[G.block].lblock >> 8) <= 1) G.len = 0;
        }
    }
    return 0;
}

// k_tiff_j2k_gather's arithmetic for one contribution: where its bytes lie in the stream (*from,
// from S.src_off) and where they go in the gather area (*to, from S.gather), both checked against
// the stream's length, which is the gather area's too.  False: nothing to copy.
PBX_J2K_FN bool j2k_gather_span(const J2Stream& S, const J2Code& C, const J2Contrib& G, uint32_t* from, uint32_t* to) {
    if (!G.len || !(C.off & J2C_GATHERED)) return false;
    const uint32_t run = C.off & ~J2C_GATHERED;
    if (G.off > S.len || G.len > S.len - G.off) return false;
    if (G.at > C.len || G.len > C.len - G.at) return false;
    if (run > S.len || C.len > S.len - run) return false;
    *from = G.off;
    *to = run + G.at;
    return true;
}

// Where tier 1 reads a block's bytes: base[0] the stream's packets, base[1] its gather area.
// Null: the run does not lie inside the stream's length.
PBX_J2K_FN const uint8_t* j2k_code_bytes(const J2Stream& S, const J2Code& C, const uint8_t* packets, const uint8_t* gather) {
    const uint32_t off = C.off & ~J2C_GATHERED;
    if (off > S.len || C.len > S.len - off) return nullptr;
    return (C.off & J2C_GATHERED ? gather : packets) + off;
}

// ------------------------------------------------------------------------------ tier 1
// LDS of one code block: int32 magnitudes (pitch w), one flag byte per coefficient with a border
// of one (pitch w + 2), the 19 context states (index << 1 | MPS), the MQ table.
constexpr uint32_t J2F_SIG = 1, J2F_VIS = 2, J2F_REF = 4, J2F_NEG = 8;
constexpr uint32_t J2_CTX_BYTES = 32, J2_TAB_BYTES = 192;

struct J2MQ {
    const uint8_t* d;
    uint32_t len, bp, c, a, ct;
    uint8_t* ctx;
    const uint32_t* tab;
};

// bytes past the block's last are FF: FF FF reads as a marker, which feeds 1-bits for ever
PBX_J2K_FN uint32_t j2mq_byte(const J2MQ& m, uint32_t i) { return i < m.len ? m.d[i] : 0xFFu; }

PBX_J2K_FN void j2mq_bytein(J2MQ& m) {
    if (j2mq_byte(m, m.bp) == 0xFF) {
        const uint32_t b1 = j2mq_byte(m, m.bp + 1);
        if (b1 > 0x8F) {
            m.c += 0xFF00;
            m.ct = 8;
        } else {
            m.bp++;
            m.c += b1 << 9;
            m.ct = 7;
        }
    } else {
        m.bp++;
        m.c += j2mq_byte(m, m.bp) << 8;
        m.ct = 8;
    }
}

PBX_J2K_FN void j2mq_init(J2MQ& m) {
    m.bp = 0;
    m.c = j2mq_byte(m, 0) << 16;
    j2mq_bytein(m);
    m.c <<= 7;
    m.ct -= 7;
    m.a = 0x8000;
}

PBX_J2K_FN uint32_t j2mq_decode(J2MQ& m, uint32_t cx) {
    const uint32_t st = m.ctx[cx], mps = st & 1u;
    const uint32_t e = m.tab[st >> 1], qe = e & 0xffffu;
    const uint32_t nmps = (e >> 16) & 63u, nlps = (e >> 22) & 63u, sw = e >> 28;
    uint32_t d;
    m.a -= qe;
    if ((m.c >> 16) < qe) {
        if (m.a < qe) {
            d = mps;
            m.ctx[cx] = (uint8_t)(nmps << 1 | mps);
        } else {
            d = mps ^ 1u;
            m.ctx[cx] = (uint8_t)(nlps << 1 | (mps ^ sw));
        }
        m.a = qe;
    } else {
        m.c -= qe << 16;
        if (m.a & 0x8000u) return mps;
        if (m.a < qe) {
            d = mps ^ 1u;
            m.ctx[cx] = (uint8_t)(nlps << 1 | (mps ^ sw));
        } else {
            d = mps;
            m.ctx[cx] = (uint8_t)(nmps << 1 | mps);
        }
    }
    do {
        if (m.ct == 0) j2mq_bytein(m);
        m.a <<= 1;
        m.c <<= 1;
        m.ct--;
    } while (!(m.a & 0x8000u));
    return d;
}

// zero-coding context (table D.1) from the significant neighbours: hh horizontal, vv vertical,
// dd diagonal; orient 0 LL, 1 HL, 2 LH, 3 HH
PBX_J2K_FN uint32_t j2zc(uint32_t orient, uint32_t hh, uint32_t vv, uint32_t dd) {
    if (orient == 3) {
        const uint32_t hv = hh + vv;
        if (dd >= 3) return 8;
        if (dd == 2) return hv >= 1 ? 7 : 6;
        if (dd == 1) return hv >= 2 ? 5 : hv == 1 ? 4 : 3;
        return hv >= 2 ? 2 : hv;
    }
    if (orient == 1) {
        const uint32_t t = hh;
        hh = vv;
        vv = t;
    }
    if (hh == 2) return 8;
    if (hh == 1) return vv >= 1 ? 7 : dd >= 1 ? 6 : 5;
    if (vv == 2) return 4;
    if (vv == 1) return 3;
    return dd >= 2 ? 2 : dd;
}

struct J2Nbr {
    uint32_t hh, vv, dd;
};

PBX_J2K_FN J2Nbr j2nbr(const uint8_t* f, uint32_t fp) {
    J2Nbr n;
    n.hh = (f[-1] & 1u) + (f[1] & 1u);
    n.vv = (*(f - fp) & 1u) + (f[fp] & 1u);
    n.dd = (*(f - fp - 1) & 1u) + (*(f - fp + 1) & 1u) + (f[fp - 1] & 1u) + (f[fp + 1] & 1u);
    return n;
}

PBX_J2K_FN int32_t j2contrib(uint32_t f) { return (f & J2F_SIG) ? ((f & J2F_NEG) ? -1 : 1) : 0; }

// the coefficient at *f becomes significant in bit-plane p: its sign (table D.3), flag and bit.
// IRR (the irreversible path): every magnitude carries one more bit below bit-plane 0 and is at
// all times twice the midpoint of what the passes so far leave open: 3 * 2^p here (|q| = 2^p, the
// planes below p unknown: 2 (2^p + 2^(p-1))), and +- 2^p at a refinement bit in bit-plane p.
template <bool IRR>
PBX_J2K_FN void j2sign(J2MQ& m, uint8_t* f, uint32_t fp, int32_t* mag, uint32_t p) {
    int32_t hc = j2contrib(f[-1]) + j2contrib(f[1]), vc = j2contrib(*(f - fp)) + j2contrib(f[fp]);
    hc = hc < -1 ? -1 : hc > 1 ? 1 : hc;
    vc = vc < -1 ? -1 : vc > 1 ? 1 : vc;
    uint32_t flip = 0;
    if (hc < 0 || (hc == 0 && vc < 0)) {
        flip = 1;
        hc = -hc;
        vc = -vc;
    }
    const uint32_t cx = hc == 1 ? (uint32_t)(12 + vc) : vc == 0 ? 9u : 10u;
    const uint32_t s = j2mq_decode(m, cx) ^ flip;
    *f = (uint8_t)(*f | J2F_SIG | (s ? J2F_NEG : 0));
    if (IRR) *mag = (int32_t)(3u << p);
    else *mag |= (int32_t)(1u << p);
}

// One code block of w x h coefficients (w * h <= the magnitudes' room, (w + 2) * (h + 2) <= the
// flags': the caller checks), magnitudes and flags zero, contexts at their initial states:
// `passes` coding passes from bit-plane planes - 1 down (1 <= planes <= 31, passes <= 3 * planes
// - 2: the caller checks), the first a cleanup pass.  IRR: planes <= 30 (3 * 2^29 fits).
template <bool IRR>
PBX_J2K_FN void j2k_block(int32_t* mag, uint8_t* flg, uint8_t* ctx, const uint32_t* tab, const uint8_t* codebytes,
                          uint32_t len, uint32_t w, uint32_t h, uint32_t orient, uint32_t planes, uint32_t passes) {
    J2MQ m;
    m.d = codebytes;
    m.len = len;
    m.ctx = ctx;
    m.tab = tab;
    j2mq_init(m);
    const uint32_t fp = w + 2;
    uint32_t p = planes - 1, kind = 2;
    for (uint32_t pass = 0; pass < passes; pass++) {
        for (uint32_t y0 = 0; y0 < h; y0 += 4) {
            const uint32_t y1 = y0 + 4 < h ? y0 + 4 : h;
            for (uint32_t x = 0; x < w; x++) {
                uint8_t* f0 = flg + (y0 + 1) * fp + x + 1;
                int32_t* m0 = mag + y0 * w + x;
                if (kind == 0) {  // significance propagation
                    for (uint32_t y = y0; y < y1; y++) {
                        uint8_t* f = f0 + (y - y0) * fp;
                        if (*f & J2F_SIG) continue;
                        const J2Nbr n = j2nbr(f, fp);
                        if (n.hh + n.vv + n.dd == 0) continue;
                        if (j2mq_decode(m, j2zc(orient, n.hh, n.vv, n.dd))) j2sign<IRR>(m, f, fp, m0 + (y - y0) * w, p);
                        *f |= J2F_VIS;
                    }
                } else if (kind == 1) {  // magnitude refinement
                    for (uint32_t y = y0; y < y1; y++) {
                        uint8_t* f = f0 + (y - y0) * fp;
                        if ((*f & (J2F_SIG | J2F_VIS)) != J2F_SIG) continue;
                        uint32_t cx = 16;
                        if (!(*f & J2F_REF)) {
                            const J2Nbr n = j2nbr(f, fp);
                            cx = n.hh + n.vv + n.dd ? 15 : 14;
                        }
                        const uint32_t bit = j2mq_decode(m, cx);
                        if (IRR) m0[(y - y0) * w] += bit ? (int32_t)(1u << p) : -(int32_t)(1u << p);
                        else m0[(y - y0) * w] |= (int32_t)(bit << p);
                        *f |= J2F_REF;
                    }
                } else {  // cleanup
                    uint32_t first = y0;
                    if (y1 - y0 == 4) {
                        bool run = true;
                        for (uint32_t y = y0; y < y1 && run; y++) {
                            const uint8_t* f = f0 + (y - y0) * fp;
                            const J2Nbr n = j2nbr(f, fp);
                            run = !(*f & (J2F_SIG | J2F_VIS)) && n.hh + n.vv + n.dd == 0;
                        }
                        if (run) {
                            if (!j2mq_decode(m, 17)) continue;
                            uint32_t k = j2mq_decode(m, 18) << 1;
                            k |= j2mq_decode(m, 18);  // 0 .. 3: inside the stripe
                            j2sign<IRR>(m, f0 + k * fp, fp, m0 + k * w, p);
                            first = y0 + k + 1;
                        }
                    }
                    for (uint32_t y = first; y < y1; y++) {
                        uint8_t* f = f0 + (y - y0) * fp;
                        if (*f & J2F_VIS) {  // coded in this bit-plane's first pass: the flag goes here
                            *f &= (uint8_t)~J2F_VIS;
                            continue;
                        }
                        if (*f & J2F_SIG) continue;
                        const J2Nbr n = j2nbr(f, fp);
                        if (j2mq_decode(m, j2zc(orient, n.hh, n.vv, n.dd))) j2sign<IRR>(m, f, fp, m0 + (y - y0) * w, p);
                    }
                }
            }
        }
        if (kind == 2) {  // the bit-plane is done
            if (p == 0) break;
            p--;
        }
        kind = kind == 2 ? 0 : kind + 1;
    }
}

// ------------------------------------------------------------------- irreversible arithmetic
// The per-sample float32 arithmetic of the 9/7 path (T.800 E.1, F.3.8, G.3), shared by the
// kernels and the CPU hook.  Every operation is rounded to float32 on its own (no contraction
// into fused multiply-adds), in one fixed order, so the two agree bit for bit.
constexpr float J2F_K = 1.230174105f, J2F_INVK = (float)(1.0 / 1.230174105);
constexpr float J2F_DELTA = 0.443506852f, J2F_GAMMA = 0.882911075f, J2F_BETA = -0.052980118f,
                J2F_ALPHA = -1.586134342f;

// tier 1's store: m2 is twice the midpoint magnitude, hstep half the band's step
PBX_J2K_FN float j2f_dequant(int32_t m2, bool neg, float hstep) {
#pragma clang fp contract(off)
    const float v = (float)m2 * hstep;
    return neg ? -v : v;
}

PBX_J2K_FN float j2f_scale(float x, float k) {
#pragma clang fp contract(off)
    return x * k;
}

// one lifting update: the neighbours' sum, times the constant, subtracted
PBX_J2K_FN float j2f_lift(float x, float a, float b, float c) {
#pragma clang fp contract(off)
    const float s = a + b;
    const float t = c * s;
    return x - t;
}

// inverse irreversible colour transform (G.3): v = Y, Cb, Cr -> R, G, B
PBX_J2K_FN void j2f_ict(float v[3]) {
#pragma clang fp contract(off)
    const float y = v[0], cb = v[1], cr = v[2];
    const float r = y + 1.402f * cr;
    const float g0 = y - 0.34413f * cb;
    const float g = g0 - 0.71414f * cr;
    const float b = y + 1.772f * cb;
    v[0] = r;
    v[1] = g;
    v[2] = b;
}

// level shift, round half to even, clamp to [0, 2^prec - 1]; NaN and -inf give 0, +inf the top
PBX_J2K_FN uint32_t j2f_sample(float v, uint32_t prec) {
#pragma clang fp contract(off)
    const float hi = (float)((1u << prec) - 1u);
    const float t = v + (float)(1u << (prec - 1));
    if (!(t > 0.0f)) return 0;
    if (t >= hi) return (uint32_t)hi;
    return (uint32_t)__builtin_rintf(t);
}

// One dimension of the inverse 9/7 in place over x[0 .. n) with stride `st`, the low-pass samples
// already at the even places: the CPU hook's form; k_tiff_j2k_idwt97 runs the same five steps
// with a barrier between them.  A signal of one sample passes through.
PBX_J2K_FN float j2f_at(const float* x, int64_t n, int64_t st, int64_t i) {
    return x[(i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i) * st];
}
inline void j2f_sr97(float* x, int64_t n, int64_t st) {
    if (n < 2) return;
    for (int64_t i = 0; i < n; i++) x[i * st] = j2f_scale(x[i * st], i & 1 ? J2F_INVK : J2F_K);
    const float c[4] = {J2F_DELTA, J2F_GAMMA, J2F_BETA, J2F_ALPHA};
    for (int k = 0; k < 4; k++)
        for (int64_t i = k & 1; i < n; i += 2) x[i * st] = j2f_lift(x[i * st], j2f_at(x, n, st, i - 1), j2f_at(x, n, st, i + 1), c[k]);
}

// ------------------------------------------------------- subsampled and YCbCr components
// The placement of a segment with J2_SEG_CHROMA bits (k_tiff_j2k_place_chroma and the CPU hook).
// Upsampling is replication: plane sample (x, y) of component 1 or 2 is component sample
// (x / XRsiz, y / YRsiz) -- T.800 puts a component sample on the reference grid at multiples of
// XRsiz and YRsiz and defines no chroma siting.  Where component c's sample of pixel (x, y) of a
// segment w pixels wide lies in its plane, in samples:
PBX_J2K_FN uint64_t j2k_chroma_at(uint32_t c, uint32_t x, uint32_t y, uint32_t w, uint32_t rct) {
    const uint32_t xs = c && (rct & J2_SEG_XS2) ? 1u : 0u, ys = c && (rct & J2_SEG_YS2) ? 1u : 0u;
    const uint32_t pitch = (w + xs) >> xs;
    return (uint64_t)(y >> ys) * pitch + (x >> xs);
}

// YCbCr -> RGB on clamped 8-bit samples, in place: libjpeg's jdcolor.c 16-bit fixed point, the
// arithmetic of k_tiff_jpeg_place
PBX_J2K_FN void j2k_ycc_rgb(uint32_t v[3]) {
    const int32_t y = (int32_t)v[0], u = (int32_t)v[1] - 128, w = (int32_t)v[2] - 128;
    const int32_t r = y + ((91881 * w + 32768) >> 16);
    const int32_t g = y + ((-22554 * u - 46802 * w + 32768) >> 16);
    const int32_t b = y + ((116130 * u + 32768) >> 16);
    v[0] = (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r);
    v[1] = (uint32_t)(g < 0 ? 0 : g > 255 ? 255 : g);
    v[2] = (uint32_t)(b < 0 ? 0 : b > 255 ? 255 : b);
}

}  // namespace pbx
