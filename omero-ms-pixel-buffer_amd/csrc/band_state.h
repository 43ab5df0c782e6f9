// band_state.h — the band record of a sparse plane and the decisions of its load state machine:
// admission of a write (alone or as a group that spans planes), its failure and its completion.
// Device-free: plain functions over Band records, no context, no HIP call, no clock (the caller
// passes the time and holds the registry lock).  runtime.cpp runs them under pbx_ctx::reg_mu;
// scripts/band_group_san.cpp and pbx_test_band_group_admit run them with no device at all.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/pbx.h"

namespace pbx {

// One row band of a sparse plane (pbx_plane_create_sparse): rows [k*B, (k+1)*B) of the plane
// (clipped to the plane and to the context's owned rows), loaded on demand, pinned by the
// batches that read it and evicted on its own (region-proportional residency: a request
// loads only the bands its rows cover, as getTileDirect reads only the requested region,
// TileRequestHandler.java:102-109).
enum BandState : int { BS_ABSENT = 0, BS_LOADING = 1, BS_READY = 2 };

struct Band {
    uint8_t* dev = nullptr;      // the band's rows at the plane's pitch + 256 B slack
    size_t bytes = 0;
    int state = BS_ABSENT;
    int64_t pins = 0;            // planned batches that read it
    uint64_t last_use = 0;
    int64_t fresh_until = 0;     // loaded, not served yet: not evicted before this (fresh_now)
    uint32_t rows_left = 0;      // BS_LOADING: rows not written yet
    int32_t writers = 0;         // pbx_band_write calls in flight
    bool failed = false;         // BS_LOADING: a write failed; the last writer out resets the band
    int64_t touched = 0;         // BS_LOADING: mono_ns of the last write activity
    // the last load went idle past stale_ns and was reset: the next load must start at the
    // band's first row, so a late piece of the reset load fails instead of starting a load
    // that could never complete
    bool stale_reset = false;
    std::vector<uint8_t> rows_done;
};

typedef std::vector<std::pair<void*, size_t>> BandBlocks;  // HBM blocks to give back

// A loading band back to absent; its HBM goes to `to_free`.
inline void band_reset(Band& b, BandBlocks& to_free) {
    if (b.dev) to_free.emplace_back(b.dev, b.bytes);
    b.dev = nullptr;
    b.state = BS_ABSENT;
    b.rows_done.clear();
    b.rows_left = 0;
    b.failed = false;
}

// What the admission of a write looks at.
struct BandView {
    int state;
    bool has_dev;      // the band's HBM is there
    int32_t writers;
    bool failed, stale_reset;
    bool idle_stale;   // its last write activity lies further back than the stale limit
};

inline BandView band_view(const Band& b, int64_t now, int64_t stale_ns) {
    return BandView{b.state, b.dev != nullptr, b.writers, b.failed, b.stale_reset, now - b.touched > stale_ns};
}

// The decision for one band.  BA_ALLOC and BA_JOIN admit the write; the others keep it out.
enum BandAdmit : int {
    BA_ALLOC = 1,     // absent (or a failed / stale load without writers, reset first): join and allocate
    BA_JOIN = 2,      // loading, its HBM there, not failed: one more writer
    BA_RESIDENT = 3,  // 409: the band is resident
    BA_BUSY = 4,      // 409: being allocated or reset by another caller
    BA_STALE = 5,     // 500: its load was reset as stale and this piece does not start the band
    BA_SKIPPED = 6    // a sibling of a primary that was not admitted: never attempted
};

inline bool band_admitted(int a) { return a == BA_ALLOC || a == BA_JOIN; }

// PBX_OK for an admitted write, else the status of the refusal (-1: never attempted).
inline int band_admit_status(int a) {
    return band_admitted(a) ? (int)PBX_OK : a == BA_STALE ? (int)PBX_E_INTERNAL : a == BA_SKIPPED ? -1 : (int)PBX_E_EXISTS;
}

// A load that failed part-way, or whose loader went away, starts over with the next writer.
inline bool band_load_dead(const BandView& v) {
    return v.state == BS_LOADING && v.writers == 0 && (v.failed || v.idle_stale);
}

// `first_row`: the piece starts at the band's first row.
inline int band_admit_one(const BandView& v, bool first_row) {
    if (v.state == BS_READY) return BA_RESIDENT;
    const bool dead = band_load_dead(v);
    const bool stale_reset = v.stale_reset || (dead && !v.failed);
    if (dead || v.state == BS_ABSENT) return stale_reset && !first_row ? BA_STALE : BA_ALLOC;
    return !v.has_dev || v.failed ? BA_BUSY : BA_JOIN;
}

// The decision for a group of n bands (one per plane) that one fill writes: every member by the
// rule above; if the primary is kept out, nobody joins.
inline void band_group_admit(const BandView* v, int n, int primary, bool first_row, int* out) {
    out[primary] = band_admit_one(v[primary], first_row);
    for (int i = 0; i < n; i++)
        if (i != primary) out[i] = band_admitted(out[primary]) ? band_admit_one(v[i], first_row) : (int)BA_SKIPPED;
}

// A dead load back to absent, as its next writer (or pbx_plane_band_info) finds it.
inline void band_reap(Band& b, const BandView& v, BandBlocks& to_free) {
    if (!band_load_dead(v)) return;
    if (!b.failed) b.stale_reset = true;
    band_reset(b, to_free);
}

// An admitted write (BA_ALLOC or BA_JOIN) enters band `b` of `band_rows` rows.
inline void band_join(Band& b, const BandView& v, int a, int32_t band_rows, int64_t now, BandBlocks& to_free) {
    band_reap(b, v, to_free);
    if (a == BA_ALLOC) {
        b.stale_reset = false;
        b.state = BS_LOADING;
        b.failed = false;
        b.rows_done.assign((size_t)band_rows, 0);
        b.rows_left = (uint32_t)band_rows;
    }
    b.writers++;
    b.touched = now;
}

// A writer leaves after its write failed: the whole load fails, and the band is reset (its HBM
// returned) by the last writer to leave, never under another writer's upload.
inline void band_leave_failed(Band& b, int64_t now, BandBlocks& to_free) {
    b.writers--;
    b.failed = true;
    b.touched = now;
    if (b.writers == 0) band_reset(b, to_free);
}

enum BandDone : int { BD_VOID = 0, BD_WRITTEN = 1, BD_PUBLISHED = 2 };

// A writer leaves after its rows [r0, r0 + rows) (relative to the band) are in place.  BD_VOID:
// another writer of this load failed meanwhile, the load is void and the last writer out resets
// it.  BD_PUBLISHED: this was the last write, the band is BS_READY (the caller stamps last_use and
// fresh_until).
inline int band_complete(Band& b, int32_t band_rows, int32_t r0, int32_t rows, int64_t now, BandBlocks& to_free) {
    if (b.failed || b.state != BS_LOADING || b.rows_done.size() != (size_t)band_rows) {
        b.writers--;
        if (b.writers == 0) band_reset(b, to_free);
        return BD_VOID;
    }
    b.writers--;
    b.touched = now;
    for (int32_t r = r0; r < r0 + rows; r++)
        if (!b.rows_done[(size_t)r]) {
            b.rows_done[(size_t)r] = 1;
            b.rows_left--;
        }
    if (b.rows_left != 0 || b.writers != 0) return BD_WRITTEN;
    b.rows_done.clear();
    b.rows_done.shrink_to_fit();
    b.state = BS_READY;
    return BD_PUBLISHED;
}

}  // namespace pbx
