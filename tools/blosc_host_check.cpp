// Runs the Blosc / LZ4 decoder of skoots_amd/csrc/blosc.hip on the CPU: the file is compiled as host C++
// (-DSK_BLOSC_HOST: the decoder text of blosc_lz4.inc with a lane section = a loop over the 64 lanes, a barrier =
// nothing, LDS = a heap struct) so that AddressSanitizer and UBSan see every load and store it makes.  Every item gets a
// src and a dst allocation of exactly its sizes (the bytes in front of an unaligned start are poisoned), so one byte
// read or written outside them is a report.  Driven by tools/blosc_host_check.py, which writes the items and compares
// the results with the Python reference decoder.
//
//   corpus file:  int32 n, then per item: int32 mode, int32 src_misalign, int32 dst_misalign, int32 0, int64 row[5],
//                 int64 src_bytes, int64 dst_bytes, src bytes
//                 mode 0: one table row through lz4_stream (row offsets relative to the two buffers)
//                 mode 1: a whole frame through sk_blosc_decode_host
//   result file:  per item: int32 status, dst_bytes bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define SK_HAVE_ASAN 1
#endif
#endif
#if defined(__SANITIZE_ADDRESS__)
#define SK_HAVE_ASAN 1
#endif
#ifdef SK_HAVE_ASAN
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(a, n) ((void)(a), (void)(n))
#endif

#define SK_BLOSC_HOST 1
#include "../skoots_amd/csrc/blosc.hip"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s corpus results\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    sk_lz4_host::Lz4Lds* lds = new sk_lz4_host::Lz4Lds;
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 2;
    for (int32_t i = 0; i < n; ++i) {
        int32_t head[4];
        int64_t row[5], sl, dl;
        if (fread(head, 4, 4, in) != 4 || fread(row, 8, 5, in) != 5 || fread(&sl, 8, 1, in) != 1 || fread(&dl, 8, 1, in) != 1)
            return 2;
        const int mode = head[0], smis = head[1], dmis = head[2];
        // malloc returns 16-byte aligned blocks: the data start `mis` bytes in, the bytes before them are poisoned
        const size_t sn = (size_t)(sl + smis) ? (size_t)(sl + smis) : 1, dn = (size_t)(dl + dmis) ? (size_t)(dl + dmis) : 1;
        uint8_t* sbuf = (uint8_t*)malloc(sn);
        uint8_t* dbuf = (uint8_t*)malloc(dn);
        if (sl && fread(sbuf + smis, 1, (size_t)sl, in) != (size_t)sl) return 2;
        memset(dbuf, 0xA5, dn);
        if (smis) ASAN_POISON_MEMORY_REGION(sbuf, (size_t)smis);
        if (dmis) ASAN_POISON_MEMORY_REGION(dbuf, (size_t)dmis);
        if (sl + smis == 0) ASAN_POISON_MEMORY_REGION(sbuf, 1);
        if (dl + dmis == 0) ASAN_POISON_MEMORY_REGION(dbuf, 1);
        int32_t status = -1;
        if (mode == 0) {
            status = sk_lz4_host::lz4_stream(*lds, sbuf + smis, sl, row[0], row[1], row[2], row[3], row[4], dbuf + dmis, dl);
        } else if (sk_blosc_decode_host(sbuf + smis, sl, dbuf + dmis, dl, &status) != SK_OK) {
            return 3;
        }
        ASAN_UNPOISON_MEMORY_REGION(sbuf, sn);
        ASAN_UNPOISON_MEMORY_REGION(dbuf, dn);
        fwrite(&status, 4, 1, out);
        if (dl) fwrite(dbuf + dmis, 1, (size_t)dl, out);
        free(sbuf);
        free(dbuf);
    }
    delete lds;
    fclose(in);
    fclose(out);
    return 0;
}
