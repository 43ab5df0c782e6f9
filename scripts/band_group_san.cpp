// The band state machine of a write that spans planes -- the device-free admission, failure and
// completion functions of csrc/band_state.h -- under AddressSanitizer / UBSan: a stand-alone
// program (no Python, no device call, nothing preloaded) that drives Band records through the
// sequences the runtime's band_group_load_rows runs them through: a load in pieces that
// publishes, a failed writer, a void writer, a stale reset, a sibling dropped at allocation, a
// primary that is kept out.  The bands' HBM is heap memory here, so a block returned twice or
// never shows as a sanitizer report.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/ (its log: profiles/band_group/san.log).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../omero-ms-pixel-buffer_amd/csrc/band_state.h"

using namespace pbx;

static int failures = 0;

static void check(const char* what, bool ok) {
    printf("%-74s %s\n", what, ok ? "ok" : "UNEXPECTED");
    if (!ok) failures++;
}

constexpr int32_t ROWS = 8;            // rows of a band
constexpr int64_t STALE = 1000;        // the stale limit, in the clock's units
constexpr size_t BYTES = 64;

// What band_group_load_rows does with the decisions, on members that are Band records alone.
struct Group {
    std::vector<Band*> b;
    int primary = 0;
    bool joined[4] = {false, false, false, false}, alloc[4] = {false, false, false, false};
    int status[4] = {-1, -1, -1, -1};
    BandBlocks freed;

    // admission; returns the primary's decision
    int admit(int64_t now, bool first_row) {
        BandView v[4];
        int a[4];
        const int n = (int)b.size();
        for (int i = 0; i < n; i++) v[i] = band_view(*b[i], now, STALE);
        band_group_admit(v, n, primary, first_row, a);
        if (!band_admitted(a[primary])) {
            band_reap(*b[primary], v[primary], freed);
            status[primary] = band_admit_status(a[primary]);
            return a[primary];
        }
        for (int i = 0; i < n; i++) {
            status[i] = band_admit_status(a[i]);
            if (!band_admitted(a[i])) continue;
            band_join(*b[i], v[i], a[i], ROWS, now, freed);
            joined[i] = true;
            alloc[i] = a[i] == BA_ALLOC;
        }
        return a[primary];
    }
    // allocation, primary first; `no_room` names a member whose allocation answers 507
    int allocate(int64_t now, int no_room = -1) {
        const int n = (int)b.size();
        for (int j = 0; j < n; j++) {
            const int i = j == 0 ? primary : j <= primary ? j - 1 : j;
            if (!joined[i] || !alloc[i]) continue;
            if (i == no_room) {
                if (i == primary) return fail_all(now, PBX_E_NO_SPACE);
                band_leave_failed(*b[i], now, freed);
                joined[i] = false;
                status[i] = PBX_E_NO_SPACE;
                continue;
            }
            b[i]->dev = (uint8_t*)malloc(BYTES);
            b[i]->bytes = BYTES;
        }
        return PBX_OK;
    }
    int fail_all(int64_t now, int rc) {
        for (size_t i = 0; i < b.size(); i++)
            if (joined[i]) {
                band_leave_failed(*b[i], now, freed);
                joined[i] = false;
                status[i] = rc;
            }
        return rc;
    }
    // the fill wrote rows [r0, r0 + rows) of every joined member
    int complete(int64_t now, int32_t r0, int32_t rows) {
        for (size_t i = 0; i < b.size(); i++) {
            if (!joined[i]) continue;
            for (int32_t r = r0; r < r0 + rows; r++) b[i]->dev[r] = (uint8_t)(r + 1);  // the band's HBM is there
            const int d = band_complete(*b[i], ROWS, r0, rows, now, freed);
            status[i] = d == BD_VOID ? (int)PBX_E_INTERNAL : (int)PBX_OK;
            joined[i] = false;
        }
        return status[primary];
    }
    void give_back() {
        for (auto& f : freed) free(f.first);
        freed.clear();
    }
};

static void release(Band& b) {
    free(b.dev);
    b = Band();
}

int main() {
    // ---------------------------------------------------------------- success in pieces
    {
        Band p[3];
        Group g1{{&p[0], &p[1], &p[2]}, 1}, g2{{&p[0], &p[1], &p[2]}, 1};
        check("three absent bands: all join and allocate", g1.admit(10, false) == BA_ALLOC && g1.alloc[0] && g1.alloc[1] && g1.alloc[2]);
        check("allocation", g1.allocate(11) == PBX_OK && p[0].dev && p[1].dev && p[2].dev);
        check("first piece written, nothing published", g1.complete(12, 3, 5) == PBX_OK && p[0].state == BS_LOADING &&
                                                            p[2].rows_left == 3 && p[1].writers == 0);
        check("second piece joins as one more writer", g2.admit(13, true) == BA_JOIN && !g2.alloc[0] && p[0].writers == 1);
        check("no allocation for it", g2.allocate(14) == PBX_OK);
        check("the last write publishes every band", g2.complete(15, 0, 3) == PBX_OK && p[0].state == BS_READY &&
                                                         p[1].state == BS_READY && p[2].state == BS_READY && p[0].rows_done.empty());
        Group g3{{&p[0], &p[1], &p[2]}, 0};
        check("a write of resident bands: 409, nothing joined", g3.admit(16, true) == BA_RESIDENT && g3.status[0] == PBX_E_EXISTS &&
                                                                    g3.status[1] == -1 && p[1].writers == 0);
        check("nothing was freed", g1.freed.empty() && g2.freed.empty() && g3.freed.empty());
        for (Band& b : p) release(b);
    }
    // ---------------------------------------------------------------- a failed writer, alone
    {
        Band p[2];
        Group g{{&p[0], &p[1]}, 0};
        g.admit(10, true);
        g.allocate(11);
        check("the fill fails: every joined member is failed with its status", g.fail_all(12, PBX_E_BADARG) == PBX_E_BADARG &&
                                                                                   g.status[0] == 400 && g.status[1] == 400);
        check("the last writer out reset the bands: absent, HBM returned", p[0].state == BS_ABSENT && !p[0].dev && !p[1].dev &&
                                                                               g.freed.size() == 2 && !p[0].failed && !p[0].stale_reset);
        g.give_back();
        Group again{{&p[0], &p[1]}, 0};
        check("the same call again: join and allocate, from any row", again.admit(13, false) == BA_ALLOC);
        again.allocate(14);
        check("and it publishes", again.complete(15, 0, ROWS) == PBX_OK && p[0].state == BS_READY && p[1].state == BS_READY);
        for (Band& b : p) release(b);
    }
    // ---------------------------------------------------------------- a failed writer and a void one
    {
        Band p[2];
        Group a{{&p[0], &p[1]}, 0}, b{{&p[0], &p[1]}, 1};
        a.admit(10, true);
        a.allocate(11);
        check("a second writer joins both loads", b.admit(12, false) == BA_JOIN && p[0].writers == 2 && p[1].writers == 2);
        check("the first fails: the bands stay, under the other's upload", a.fail_all(13, PBX_E_INTERNAL) == 500 && p[0].dev && p[1].dev &&
                                                                              p[0].failed && p[0].state == BS_LOADING && a.freed.empty());
        Group c{{&p[0], &p[1]}, 0};
        check("a third caller meanwhile: 409, being reset", c.admit(14, true) == BA_BUSY && c.status[0] == PBX_E_EXISTS && p[0].writers == 1);
        check("the second completes: void, 500 for both members", b.complete(15, 4, 4) == PBX_E_INTERNAL && b.status[0] == 500 &&
                                                                      b.status[1] == 500);
        check("and, the last out, resets the bands", p[0].state == BS_ABSENT && p[1].state == BS_ABSENT && b.freed.size() == 2 && !p[0].failed);
        b.give_back();
    }
    // ---------------------------------------------------------------- one member void, the other published
    {
        Band p[2];
        Group a{{&p[0], &p[1]}, 0};
        a.admit(10, true);
        a.allocate(11);
        // a single-plane writer of member 1 alone joins and fails
        Group s{{&p[1]}, 0};
        check("a single write joins member 1", s.admit(12, false) == BA_JOIN);
        s.fail_all(13, PBX_E_INTERNAL);
        check("the group completes: member 0 published, member 1 void", a.complete(14, 0, ROWS) == PBX_OK && a.status[1] == 500 &&
                                                                            p[0].state == BS_READY && p[1].state == BS_ABSENT);
        check("member 1's HBM alone went back", a.freed.size() == 1 && !p[1].dev && p[0].dev);
        a.give_back();
        release(p[0]);
    }
    // ---------------------------------------------------------------- a stale reset
    {
        Band p[2];
        Group a{{&p[0], &p[1]}, 0};
        a.admit(10, true);
        a.allocate(11);
        a.complete(12, 0, 4);  // half the band, then the loader goes away
        Group late{{&p[0], &p[1]}, 0};
        check("a late piece, not at the first row: 500, the primary reset as stale", late.admit(12 + STALE + 1, false) == BA_STALE &&
                                                                                         late.status[0] == 500 && p[0].state == BS_ABSENT &&
                                                                                         p[0].stale_reset && late.freed.size() == 1);
        check("the sibling was not touched", p[1].state == BS_LOADING && p[1].dev && late.status[1] == -1);
        late.give_back();
        Group mid{{&p[0], &p[1]}, 0};
        check("still 500 away from the first row", mid.admit(13 + STALE, false) == BA_STALE && mid.freed.empty());
        Group fresh{{&p[0], &p[1]}, 0};
        check("from the first row: both start over", fresh.admit(14 + STALE, true) == BA_ALLOC && fresh.alloc[1] && !p[0].stale_reset &&
                                                         !p[1].stale_reset && fresh.freed.size() == 1 && p[1].rows_left == ROWS);
        fresh.give_back();
        fresh.allocate(15 + STALE);
        check("and publish", fresh.complete(16 + STALE, 0, ROWS) == PBX_OK && p[0].state == BS_READY && p[1].state == BS_READY);
        // a sibling whose load went stale, under a primary that is absent: a piece away from the first row
        Band q[2];
        Group h{{&q[0], &q[1]}, 1};
        h.admit(10, true);
        h.allocate(11);
        h.complete(12, 0, 4);
        band_reap(q[1], band_view(q[1], 13 + STALE, STALE), h.freed);  // member 1's dead load is reclaimed (pbx_plane_band_info) ...
        h.give_back();
        q[1].stale_reset = false;                                      // ... and, loaded and evicted since, is plainly absent
        Group k{{&q[0], &q[1]}, 1};
        check("a stale sibling is dropped (500), the primary is written", k.admit(14 + STALE, false) == BA_ALLOC && k.status[0] == 500 &&
                                                                              !k.joined[0] && q[0].state == BS_LOADING && q[0].dev);
        k.allocate(15 + STALE);
        check("the primary's piece", k.complete(16 + STALE, 4, 4) == PBX_OK && q[1].state == BS_LOADING && q[1].rows_left == 4);
        for (Band& b : p) release(b);
        for (Band& b : q) release(b);
    }
    // ---------------------------------------------------------------- a sibling dropped at allocation
    {
        Band p[3];
        Group g{{&p[0], &p[1], &p[2]}, 0};
        g.admit(10, true);
        check("the last sibling does not fit: 507 for it alone", g.allocate(11, 2) == PBX_OK && g.status[2] == PBX_E_NO_SPACE && !g.joined[2] &&
                                                                     p[2].state == BS_ABSENT && !p[2].dev && g.freed.empty());
        check("the others are written and published", g.complete(12, 0, ROWS) == PBX_OK && g.status[1] == PBX_OK && p[0].state == BS_READY &&
                                                          p[1].state == BS_READY && g.status[2] == PBX_E_NO_SPACE);
        for (Band& b : p) release(b);
        Band q[3];
        Group f{{&q[0], &q[1], &q[2]}, 1};
        f.admit(10, true);
        check("the primary does not fit: the call fails, every sibling leaves failed", f.allocate(11, 1) == PBX_E_NO_SPACE &&
                                                                                          f.status[0] == 507 && f.status[1] == 507 && f.status[2] == 507);
        check("all absent again, no HBM held", q[0].state == BS_ABSENT && q[1].state == BS_ABSENT && q[2].state == BS_ABSENT && !q[0].dev &&
                                                   !q[2].dev && f.freed.empty());
    }
    // ---------------------------------------------------------------- mixed states at admission
    {
        Band p[4];
        p[1].state = BS_READY;                      // resident
        p[1].dev = (uint8_t*)malloc(BYTES);
        p[1].bytes = BYTES;
        p[2].state = BS_LOADING;                    // being allocated by another caller
        p[2].writers = 1;
        p[2].rows_done.assign(ROWS, 0);
        p[2].rows_left = ROWS;
        p[2].touched = 9;
        Group g{{&p[0], &p[1], &p[2], &p[3]}, 3};
        check("resident and busy siblings are kept out with 409, the rest joins", g.admit(10, true) == BA_ALLOC && g.status[1] == 409 &&
                                                                                      g.status[2] == 409 && g.joined[0] && g.joined[3] &&
                                                                                      p[2].writers == 1 && p[1].writers == 0);
        g.allocate(11);
        check("and is written", g.complete(12, 0, ROWS) == PBX_OK && p[0].state == BS_READY && p[3].state == BS_READY && p[1].state == BS_READY &&
                                    p[2].state == BS_LOADING);
        for (Band& b : p) release(b);
    }
    printf("%s\n", failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
