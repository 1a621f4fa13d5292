// Runs the serial text of the dynamic Huffman blocks (skoots_amd/csrc/deflate_code.inc) on the CPU, linked against
// nothing else, so that AddressSanitizer and UBSan see every load and store it makes:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/deflate_code_check.cpp \
//       -o /tmp/deflate_code_check && /tmp/deflate_code_check
//
// The work structs and every input / output array are heap blocks of exactly their size, so one element read or written
// outside them is a report.  The cases are those of tests/test_deflate_code_cpu.py: seeded random histograms of 2..286
// symbols, Fibonacci counts over 17, 20 and 24 symbols (depth past 15) and over 19 and 12 under the limit 7, one and two
// used symbols, none, all 286 with equal counts, no and one distance symbol.  Every result is checked here as well:
// lengths within the limit, Kraft sum exactly 1 with two or more used symbols, canonical codes prefix-free, and the
// header written by dfc_header_emit has the bits dfc_header_plan counted and parses back to the lengths.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define SK_DFC_NS sk_dfc
#define SK_DFC_FN static
#include "../skoots_amd/csrc/deflate_code.inc"

using namespace sk_dfc;

static int g_fail = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            ++g_fail;                     \
        }                                 \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*: the cases are the same on every run
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// lengths of one alphabet; returns the number of used symbols
static int build(const uint32_t* freq_in, int n, int limit, uint8_t* len_out) {
    uint32_t* freq = (uint32_t*)malloc(sizeof(uint32_t) * n);
    uint8_t* len = (uint8_t*)malloc(n);
    uint16_t* code = (uint16_t*)malloc(sizeof(uint16_t) * n);
    DfcWork* w = (DfcWork*)malloc(sizeof(DfcWork));
    memcpy(freq, freq_in, sizeof(uint32_t) * n);
    const int m = dfc_sort(freq, n, w->order);
    for (int i = 1; i < m; ++i) {
        const int a = w->order[i - 1], b = w->order[i];
        CHECK(freq[a] < freq[b] || (freq[a] == freq[b] && a < b), "order broken at %d", i);
    }
    dfc_lengths(freq, n, m, limit, *w, len);
    dfc_codes(len, n, *w, code);
    uint64_t kraft = 0;
    for (int s = 0; s < n; ++s) {
        CHECK((len[s] != 0) == (freq[s] != 0), "symbol %d: length %d for count %u", s, len[s], freq[s]);
        CHECK(len[s] <= limit, "symbol %d: length %d above %d", s, len[s], limit);
        if (len[s]) kraft += 1ull << (limit - len[s]);
    }
    if (m >= 2) CHECK(kraft == (1ull << limit), "Kraft sum %llu / %llu with %d symbols", (unsigned long long)kraft,
                      1ull << limit, m);
    if (m == 1) CHECK(kraft == (1ull << (limit - 1)), "one used symbol must get length 1");
    for (int a = 0; a < n; ++a)       // prefix-free: no code is the head of another
        for (int b = 0; b < n; ++b)
            if (a != b && len[a] && len[b] && len[a] <= len[b])
                CHECK((code[b] >> (len[b] - len[a])) != code[a], "code of %d is a prefix of the code of %d", a, b);
    // rarer symbols never get shorter codes
    for (int i = 1; i < m; ++i) CHECK(len[w->order[i - 1]] >= len[w->order[i]], "lengths not monotone at %d", i);
    if (len_out) memcpy(len_out, len, n);
    free(freq);
    free(len);
    free(code);
    free(w);
    return m;
}

struct BitReader {
    const uint8_t* p;
    unsigned at, end;
    unsigned take(int n) {
        unsigned v = 0;
        for (int i = 0; i < n; ++i, ++at) {
            if (at >= end) {
                CHECK(false, "header read past its %u bits", end);
                return v;
            }
            v |= (unsigned)((p[at >> 3] >> (at & 7)) & 1) << i;
        }
        return v;
    }
};

static void header(const uint8_t* ll_in, const uint8_t* dl_in) {
    uint8_t* ll = (uint8_t*)malloc(kDfcLit);
    uint8_t* dl = (uint8_t*)malloc(kDfcDist);
    memcpy(ll, ll_in, kDfcLit);
    memcpy(dl, dl_in, kDfcDist);
    DfcWork* w = (DfcWork*)malloc(sizeof(DfcWork));
    DfcHdr* h = (DfcHdr*)malloc(sizeof(DfcHdr));
    const unsigned bits = dfc_header_plan(ll, dl, *w, *h);
    const unsigned nbytes = (bits + 7) / 8;
    uint8_t* out = (uint8_t*)calloc(nbytes ? nbytes : 1, 1);   // exactly the bytes the plan counted
    unsigned at = 0;
    dfc_header_emit(*h, 1, [&](unsigned val, int nb) {
        for (int b = 0; b < nb; ++b, ++at) out[at >> 3] |= (uint8_t)(((val >> b) & 1u) << (at & 7));
    });
    CHECK(at == bits, "header: %u bits written, %u counted", at, bits);
    // parse it back
    BitReader r{out, 0, bits};
    CHECK(r.take(3) == 5u, "BFINAL / BTYPE");
    const int hlit = (int)r.take(5) + 257, hdist = (int)r.take(5) + 1, hclen = (int)r.take(4) + 4;
    CHECK(hlit <= kDfcLit && hdist <= kDfcDist && hclen <= kDfcCl, "counts %d %d %d", hlit, hdist, hclen);
    uint8_t cl[kDfcCl] = {0};
    static const int place[kDfcCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int j = 0; j < kDfcCl; ++j) CHECK(dfc_cl_place(j) == place[j], "dfc_cl_place(%d)", j);
    for (int j = 0; j < hclen; ++j) cl[place[j]] = (uint8_t)r.take(3);
    uint16_t clcode[kDfcCl];
    dfc_codes(cl, kDfcCl, *w, clcode);
    unsigned kraft = 0;
    for (int s = 0; s < kDfcCl; ++s)
        if (cl[s]) kraft += 1u << (7 - cl[s]);
    CHECK(kraft == 128u, "code-length code: Kraft sum %u / 128", kraft);
    int seq[kDfcSeq + 138], n = 0;
    while (n < hlit + hdist && g_fail == 0) {
        unsigned code = 0;
        int sym = -1;
        for (int nb = 1; nb <= 7 && sym < 0; ++nb) {
            code = (code << 1) | r.take(1);
            for (int s = 0; s < kDfcCl; ++s)
                if (cl[s] == nb && clcode[s] == code) sym = s;
        }
        CHECK(sym >= 0, "no code-length symbol at bit %u", r.at);
        if (sym < 0) break;
        if (sym < 16) seq[n++] = sym;
        else if (sym == 16) {
            CHECK(n > 0, "16 with nothing before it");
            const int rep = 3 + (int)r.take(2), v = n > 0 ? seq[n - 1] : 0;
            for (int i = 0; i < rep; ++i) seq[n++] = v;
        } else {
            const int rep = sym == 17 ? 3 + (int)r.take(3) : 11 + (int)r.take(7);
            for (int i = 0; i < rep; ++i) seq[n++] = 0;
        }
    }
    CHECK(n == hlit + hdist && r.at == bits, "sequence of %d lengths for %d, %u of %u bits", n, hlit + hdist, r.at, bits);
    for (int s = 0; s < kDfcLit && g_fail == 0; ++s) CHECK((s < hlit ? seq[s] : 0) == ll[s], "literal length %d", s);
    for (int s = 0; s < kDfcDist && g_fail == 0; ++s) CHECK((s < hdist ? seq[hlit + s] : 0) == dl[s], "distance length %d", s);
    free(ll);
    free(dl);
    free(w);
    free(h);
    free(out);
}

int main() {
    uint32_t freq[kDfcLit];
    uint8_t ll[kDfcLit], dl[kDfcDist];
    int cases = 0;
    // seeded random histograms, four shapes; the literal / length ones also go through the header with a distance set
    for (int it = 0; it < 400; ++it, ++cases) {
        const int n = 2 + (int)(rnd() % 285);
        for (int s = 0; s < n; ++s) {
            switch (it & 3) {
                case 0: freq[s] = rnd() % 50; break;
                case 1: freq[s] = 1 + rnd() % (16384 / n + 1); break;
                case 2: freq[s] = (rnd() % 8 == 0) ? rnd() % 5000 : rnd() % 4; break;
                default: freq[s] = (rnd() % 3) * (1 + rnd() % 400); break;
            }
        }
        build(freq, n, 15, nullptr);
        if (n <= kDfcCl) build(freq, n, 7, nullptr);
        for (int s = n; s < kDfcLit; ++s) freq[s] = 0;
        freq[256] = 1;
        build(freq, kDfcLit, 15, ll);
        uint32_t df[kDfcDist];
        for (int s = 0; s < kDfcDist; ++s) df[s] = (rnd() % 3 == 0) ? 1 + rnd() % 100 : 0;
        if (it % 7 == 0) memset(df, 0, sizeof(df));
        if (it % 7 == 1) {
            memset(df, 0, sizeof(df));
            df[rnd() % kDfcDist] = 5;
        }
        build(df, kDfcDist, 15, dl);
        header(ll, dl);
    }
    // Fibonacci counts: the deepest optimal trees
    const int fib_cases[5][2] = {{17, 15}, {20, 15}, {24, 15}, {19, 7}, {12, 7}};
    for (const auto& fc : fib_cases) {
        freq[0] = freq[1] = 1;
        for (int s = 2; s < fc[0]; ++s) freq[s] = freq[s - 1] + freq[s - 2];
        build(freq, fc[0], fc[1], nullptr);
        for (int s = 0; s < fc[0] / 2; ++s) {   // and descending
            const uint32_t v = freq[s];
            freq[s] = freq[fc[0] - 1 - s];
            freq[fc[0] - 1 - s] = v;
        }
        build(freq, fc[0], fc[1], nullptr);
        ++cases;
    }
    // edges
    memset(freq, 0, sizeof(freq));
    CHECK(build(freq, kDfcDist, 15, dl) == 0, "no used symbol");
    freq[2] = 7;
    CHECK(build(freq, 4, 15, nullptr) == 1, "one used symbol");
    freq[0] = 5;
    CHECK(build(freq, 4, 15, nullptr) == 2, "two used symbols");
    for (int s = 0; s < kDfcLit; ++s) freq[s] = 3;
    build(freq, kDfcLit, 15, ll);
    header(ll, dl);                                  // everything used, no distance code
    memset(freq, 0, sizeof(freq));
    freq[0] = 9000;
    freq[128] = 7000;
    freq[256] = 1;
    build(freq, kDfcLit, 15, ll);
    header(ll, dl);                                  // two literals: about 280 zero lengths
    memset(dl, 0, sizeof(dl));
    dl[3] = 1;
    header(ll, dl);                                  // one distance symbol
    memset(ll, 0, sizeof(ll));
    memset(dl, 0, sizeof(dl));
    header(ll, dl);                                  // only zeros: one code-length symbol, completed by a second
    cases += 7;
    if (g_fail) {
        fprintf(stderr, "deflate_code_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("deflate_code_check: %d cases ok\n", cases);
    return 0;
}
