// The source rows and bands of a reduced band write -- the device-free arithmetic of
// csrc/reduce_plan.h -- under AddressSanitizer / UBSan: a stand-alone program (no Python, no device
// call, nothing preloaded) that runs the sweep of tests/test_reduce_plan_host.py: k = 1 .. 4,
// source bands of {5, 8, 64} rows against destination bands of {3, 4, 64} rows, planes of
// {1, 7, 29, 777} rows and, for the shifts, of 2^31 - 1 rows.  Every piece's source rows are
// marked in a heap array of exactly the plane's rows, so a row outside the plane is a sanitizer
// report, and compared with the rows found by walking the 2x2 dependencies level by level.
//
// Build and run: `make san` in omero-ms-pixel-buffer_amd/.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../omero-ms-pixel-buffer_amd/csrc/reduce_plan.h"

using namespace pbx;

static int failures = 0;

static void check(const char* what, bool ok) {
    if (!ok) {
        printf("%-74s UNEXPECTED\n", what);
        failures++;
    }
}

// marks the rows of level 0 that rows [y0, y0 + rows) of level k depend on
static void walk(int32_t sy, int32_t k, int32_t y0, int32_t rows, std::vector<uint8_t>& need) {
    std::vector<int32_t> size(1, sy);
    for (int32_t j = 0; j < k; j++) size.push_back((size.back() + 1) / 2);
    std::vector<uint8_t> cur((size_t)size[(size_t)k], 0);
    for (int32_t y = y0; y < y0 + rows; y++) cur[(size_t)y] = 1;
    for (int32_t j = k; j > 0; j--) {
        std::vector<uint8_t> up((size_t)size[(size_t)j - 1], 0);
        for (int32_t y = 0; y < size[(size_t)j]; y++)
            if (cur[(size_t)y]) {
                up[(size_t)(2 * y)] = 1;
                up[(size_t)(2 * y + 1 < size[(size_t)j - 1] ? 2 * y + 1 : size[(size_t)j - 1] - 1)] = 1;
            }
        cur.swap(up);
    }
    need.swap(cur);
}

int main() {
    const int32_t heights[] = {1, 7, 29, 777}, sbs[] = {5, 8, 64}, dbs[] = {3, 4, 64};
    long pieces = 0;
    for (int32_t k = 1; k <= REDUCE_MAX_K; k++)
        for (int32_t sy : heights)
            for (int32_t sb : sbs)
                for (int32_t db : dbs) {
                    const int32_t dy = reduce_size(sy, k);
                    for (int32_t y0 = 0; y0 < dy; y0++)
                        for (int32_t rows = 1; y0 + rows <= dy; rows++) {
                            ReducePlan P{};
                            const int rc = reduce_plan(k, sy, sb, db, y0, rows, &P);
                            const bool one_band = y0 / db == (y0 + rows - 1) / db;
                            if (!one_band) {
                                check("rows that leave their band are refused", rc == RP_CROSS_BAND);
                                continue;
                            }
                            pieces++;
                            check("a piece inside one band is planned", rc == RP_OK && P.dst_sy == dy && P.dst_band == y0 / db);
                            std::vector<uint8_t> need, got((size_t)sy, 0);
                            walk(sy, k, y0, rows, need);
                            for (int32_t r = P.src_y0; r < P.src_y1; r++) got[(size_t)r] = 1;  // inside the plane, or a report
                            check("the source rows are the ones the levels depend on", need == got);
                            check("the bands hold them", P.band0 == P.src_y0 / sb && P.band1 == (P.src_y1 - 1) / sb &&
                                                             P.band0 * sb <= P.src_y0 && (int64_t)(P.band1 + 1) * sb >= P.src_y1);
                        }
                }
    ReducePlan P{};
    check("k = 0 is refused", reduce_plan(0, 777, 8, 4, 0, 1, &P) == RP_BAD_K);
    check("k = 5 is refused", reduce_plan(5, 777, 8, 4, 0, 1, &P) == RP_BAD_K);
    check("no rows are refused", reduce_plan(1, 777, 8, 4, 0, 0, &P) == RP_BAD_ROWS);
    check("a negative row is refused", reduce_plan(1, 777, 8, 4, -1, 1, &P) == RP_BAD_ROWS);
    check("rows past the level are refused", reduce_plan(2, 777, 8, 4, 194, 2, &P) == RP_BAD_ROWS);
    check("rows past the level are refused (overflowing sum)", reduce_plan(1, 777, 8, 4, 2147483647, 2147483647, &P) == RP_BAD_ROWS);
    check("band rows of 0 are refused", reduce_plan(1, 777, 0, 4, 0, 1, &P) == RP_BAD_BANDS &&
                                           reduce_plan(1, 777, 8, 0, 0, 1, &P) == RP_BAD_BANDS &&
                                           reduce_plan(1, 0, 8, 4, 0, 1, &P) == RP_BAD_BANDS);
    // the largest plane: the shifts stay inside 64 bits and the results inside the plane
    for (int32_t k = 1; k <= REDUCE_MAX_K; k++) {
        const int32_t sy = 2147483647, dy = reduce_size(sy, k);
        check("the last row of the largest plane", reduce_plan(k, sy, sy, 2147483647, dy - 1, 1, &P) == RP_OK &&
                                                       P.src_y0 == (int32_t)((int64_t)(dy - 1) << k) && P.src_y1 == sy &&
                                                       P.band0 == 0 && P.band1 == 0);
        check("its last band of 64 rows", reduce_plan(k, sy, 5, 64, (dy - 1) / 64 * 64, dy - (dy - 1) / 64 * 64, &P) == RP_OK &&
                                              P.src_y1 == sy && P.band1 == (sy - 1) / 5);
    }
    printf("%ld pieces planned\n%s\n", pieces, failures ? "FAILED" : "all as expected");
    return failures ? 1 : 0;
}
