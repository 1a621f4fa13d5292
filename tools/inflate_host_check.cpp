// Runs skoots_amd/csrc/inflate.hip's decoder on the CPU: the kernel text is compiled as host C++ (-DSK_INFLATE_HOST: a
// lane section is a loop over the 64 lanes, a barrier is nothing, LDS is a static struct) so that AddressSanitizer and
// UBSan see every load and store it makes.  Every stream gets a src and a dst allocation of exactly its sizes (the
// bytes in front of an unaligned src are poisoned), so one byte read or written outside a stream's ranges is a report.
// Driven by tools/inflate_host_check.py, which writes the corpus and compares the results with zlib.
//
//   corpus file:  int32 n, then per stream: int32 wrapper, int32 misalign (0..7), int64 src_len, int64 dst_len, src bytes
//   result file:  per stream: int32 status, dst_len bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

#include "../include/skoots_hip.h"

#define __global__
#define __device__
#define __shared__ static
#define __launch_bounds__(x)
struct Dim3 {
    unsigned x;
};
static Dim3 blockIdx;

#define SK_INFLATE_HOST 1
#include "../skoots_amd/csrc/inflate.hip"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s corpus results\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 2;
    for (int32_t i = 0; i < n; ++i) {
        int32_t wrapper, mis;
        int64_t sl, dl;
        if (fread(&wrapper, 4, 1, in) != 1 || fread(&mis, 4, 1, in) != 1 || fread(&sl, 8, 1, in) != 1 ||
            fread(&dl, 8, 1, in) != 1)
            return 2;
        // malloc returns 16-byte aligned blocks: the stream starts `mis` bytes in, the bytes before it are poisoned
        uint8_t* sbuf = (uint8_t*)malloc((size_t)(sl + mis) ? (size_t)(sl + mis) : 1);
        uint8_t* dbuf = (uint8_t*)malloc((size_t)dl ? (size_t)dl : 1);
        if (sl && fread(sbuf + mis, 1, (size_t)sl, in) != (size_t)sl) return 2;
        memset(dbuf, 0xA5, (size_t)dl);
        if (mis) ASAN_POISON_MEMORY_REGION(sbuf, (size_t)mis);
        if (sl + mis == 0) ASAN_POISON_MEMORY_REGION(sbuf, 1);
        if (dl == 0) ASAN_POISON_MEMORY_REGION(dbuf, 1);
        const int64_t so[2] = {mis, mis + sl}, dofs[2] = {0, dl};
        int32_t status = -1;
        blockIdx.x = 0;
        sk::inflate_kernel(sbuf, so, dbuf, dofs, wrapper, &status);
        ASAN_UNPOISON_MEMORY_REGION(sbuf, (size_t)(sl + mis) ? (size_t)(sl + mis) : 1);
        ASAN_UNPOISON_MEMORY_REGION(dbuf, (size_t)dl ? (size_t)dl : 1);
        fwrite(&status, 4, 1, out);
        if (dl) fwrite(dbuf, 1, (size_t)dl, out);
        free(sbuf);
        free(dbuf);
    }
    fclose(in);
    fclose(out);
    return 0;
}
