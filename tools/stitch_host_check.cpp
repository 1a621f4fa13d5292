// Runs skoots_amd/csrc/stitch_host.cpp (sk_stitch_walk_host, plain C++) under AddressSanitizer + UBSan on the CPU, on the
// tables tests/test_flood_and_stitch_host.py::write_host_check_tables writes: every fixture case along every axis and
// 200 random tables, each with the lut a naive walk expects.  Every array gets an allocation of exactly its size, so one
// entry read or written outside offsets / rows / lut is a report.  Then malformed tables, which must be refused.
//
//   python -c "from tests.test_flood_and_stitch_host import write_host_check_tables as w; w('/tmp/stitch_tables.bin')"
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/stitch_host_check.cpp skoots_amd/csrc/stitch_host.cpp -o /tmp/stitch_host_check
//   /tmp/stitch_host_check /tmp/stitch_tables.bin
//
//   file: int32 n, then per case: int32 P, int64 R, (P + 1) int32 offsets, R x 3 int32 rows, (offsets[P] + 1) int32 lut
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/skoots_hip.h"

namespace sk {
static char g_err[512];
void set_error(const char* fmt, ...) {   // the library's lives in errors.cpp, next to the HIP runtime
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace sk

static int32_t* read_i32(FILE* f, size_t n) {
    int32_t* p = (int32_t*)malloc(n ? n * 4 : 1);
    if (n && fread(p, 4, n, f) != n) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return p;
}

static int expect_refused(const char* what, const int32_t* off, int P, const int32_t* rows, int64_t R, int T) {
    int32_t* lut = (int32_t*)malloc((size_t)(T + 1) * 4);
    int32_t mx = 0;
    const int rc = sk_stitch_walk_host(off, P, rows, R, lut, &mx);
    free(lut);
    if (rc != SK_ERR_ARG) {
        fprintf(stderr, "%s: returned %d, expected SK_ERR_ARG\n", what, rc);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s tables.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    int bad = 0;
    long long rows_total = 0, comps_total = 0;
    for (int32_t i = 0; i < n; ++i) {
        int32_t P;
        int64_t R;
        if (fread(&P, 4, 1, f) != 1 || fread(&R, 8, 1, f) != 1) return 2;
        int32_t* off = read_i32(f, (size_t)P + 1);
        int32_t* rows = read_i32(f, (size_t)R * 3);
        const int T = off[P];
        int32_t* want = read_i32(f, (size_t)T + 1);
        int32_t* lut = (int32_t*)malloc(((size_t)T + 1) * 4);
        int32_t mx = -1, want_mx = 0;
        const int rc = sk_stitch_walk_host(off, P, rows, R, lut, &mx);
        for (int c = 0; c <= T; ++c) want_mx = want[c] > want_mx ? want[c] : want_mx;
        if (rc != SK_OK || memcmp(lut, want, ((size_t)T + 1) * 4) != 0 || mx != want_mx) {
            fprintf(stderr, "case %d: rc %d (%s), max %d / %d\n", i, rc, sk::g_err, mx, want_mx);
            ++bad;
        }
        rows_total += R;
        comps_total += T;
        free(off);
        free(rows);
        free(want);
        free(lut);
    }
    fclose(f);
    const int32_t off[3] = {0, 2, 4};
    const int32_t unsorted[6] = {1, 4, 2, 1, 3, 1}, same_plane[3] = {1, 2, 1}, backwards[3] = {3, 1, 1}, past[3] = {1, 5, 1},
                  empty[3] = {1, 3, 0}, negative[3] = {-1, 3, 1};
    const int32_t bad_off[3] = {0, 3, 2};
    bad += expect_refused("unsorted rows", off, 2, unsorted, 2, 4);
    bad += expect_refused("rows inside one plane", off, 2, same_plane, 1, 4);
    bad += expect_refused("rows backwards", off, 2, backwards, 1, 4);
    bad += expect_refused("id past the total", off, 2, past, 1, 4);
    bad += expect_refused("empty overlap", off, 2, empty, 1, 4);
    bad += expect_refused("negative id", off, 2, negative, 1, 4);
    bad += expect_refused("decreasing offsets", bad_off, 2, nullptr, 0, 4);
    printf("%d tables (%lld components, %lld rows) + 7 malformed: %d failures\n", n, comps_total, rows_total, bad);
    return bad ? 1 : 0;
}
