#!/usr/bin/env python
"""Run skoots_amd/csrc/convert.hip on the CPU under AddressSanitizer + UBSan before it runs on a device.

The kernel's text is compiled as host C++ behind a small shim: a launch is a loop over blocks and threads, and the one
barrier splits a block into two passes (pass 0 returns at the barrier; pass 1 repeats the loads and LDS stores -- the
same values to the same places -- and goes on, by which time every thread's pass 0 has filled the tile).  Source and
destination are heap blocks of exactly the array's sizes, so any access past either end of either is a sanitizer
report.  Every case is compared with the torch route (``convert_trch_to_tif.pages_torch``) on the CPU, the two
every-fp16-value cases of tests/golden/convert.npz also with what the reference produced.

    python tools/convert_host_check.py            # builds into a temporary directory, prints one line per case

It checks the indexing, the masks, the LDS layout and the arithmetic as written; what only a device has (the wave's
real LDS banking, the hardware's fp16 instructions) it cannot see.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHIM = r"""
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "skoots_hip.h"
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx;
static int g_pass;
typedef void* hipStream_t;
#define __syncthreads() do { if (g_pass == 0) return; } while (0)
#define SK_CHECK_ARG(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return SK_ERR_ARG; } } while (0)
#define SK_CHECK_LAUNCH() do {} while (0)
#define LAUNCH(kernel, grid, block, ...) \
    for (unsigned b_ = 0; b_ < (grid).x; ++b_) for (g_pass = 0; g_pass < 2; ++g_pass) \
        for (unsigned t_ = 0; t_ < (block).x; ++t_) { blockIdx.x = b_; threadIdx.x = t_; kernel(__VA_ARGS__); }
"""

MAIN = r"""
int main(int argc, char** argv) {   // in.bin dtype mode C X Y Z want.bin
    if (argc != 9) return 2;
    const int dt = atoi(argv[2]), mode = atoi(argv[3]), C = atoi(argv[4]), X = atoi(argv[5]), Y = atoi(argv[6]), Z = atoi(argv[7]);
    const size_t n = (size_t)C * X * Y * Z, eb = dt == 0 ? 1 : dt == 1 ? 2 : 4;
    void* src = malloc(n * eb);
    uint8_t* want = (uint8_t*)malloc(n);
    uint8_t* dst = (uint8_t*)malloc(n);      // 16-byte aligned by malloc: Y * C decides between the two store paths
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(src, eb, n, f) != n) return 3;
    fclose(f);
    f = fopen(argv[8], "rb");
    if (!f || fread(want, 1, n, f) != n) return 3;
    fclose(f);
    memset(dst, 0xAB, n);
    if (sk_convert_pages_u8(src, dt, mode, C, X, Y, Z, dst, nullptr) != SK_OK) return 5;
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += dst[i] != want[i];
    printf("%zu mismatches", bad);
    free(src); free(want); free(dst);
    return bad ? 1 : 0;
}
"""

DTYPES = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}
SHAPES = ((3, 5, 7, 9), (1, 33, 70, 65), (4, 2, 129, 3), (3, 1, 1, 1), (2, 3, 5, 1), (3, 64, 64, 64), (3, 3, 80, 70),
          (4, 2, 64, 130), (2, 2, 65, 64))


def values(shape, dtype, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    if mode == 0:
        return (torch.rand(shape, generator=gen) * 255.99).to(dtype)
    x = (torch.rand(shape, generator=gen) * 2 - 1) * torch.where(torch.rand(shape, generator=gen) < 0.2, 3.0, 1.0)
    x[torch.rand(shape, generator=gen) < 0.15] = 0.0
    x[torch.rand(shape, generator=gen) < 0.1] = -0.0
    return x.to(dtype)


def build(workdir):
    with open(os.path.join(ROOT, "skoots_amd", "csrc", "convert.hip")) as f:
        text = f.read()
    text = text.replace('#include "common.h"', '#include "shim.h"')
    text, n = re.subn(r"(convert_pages_kernel<T, \d>)<<<grid, block, 0, stream>>>\(", r"LAUNCH((\1), grid, block, ", text)
    if n != 4:
        raise SystemExit(f"convert.hip: expected 4 launches, found {n}: the shim needs an update")
    with open(os.path.join(workdir, "shim.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(workdir, "convert_host.cpp"), "w") as f:
        f.write(text + MAIN)
    clang = os.environ.get("CXX_HOST", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(workdir, "convert_host")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(workdir, "convert_host.cpp")])
    return exe


def run(exe, workdir, x, mode, want, label):
    a, b = os.path.join(workdir, "in.bin"), os.path.join(workdir, "want.bin")
    x.numpy().tofile(a)
    want.numpy().tofile(b)
    r = subprocess.run([exe, a, str(DTYPES[x.dtype]), str(mode)] + [str(int(s)) for s in x.shape] + [b],
                       capture_output=True, text=True)
    print(f"{label}: {r.stdout.strip()} (exit {r.returncode})")
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(1)


def main():
    import numpy as np

    from skoots_amd.utils import convert_trch_to_tif as CV
    with tempfile.TemporaryDirectory() as workdir:
        exe = build(workdir)
        count = 0
        for shape in SHAPES:
            for dtype in DTYPES:
                for mode in (0, 1, 2):
                    x = values(shape, dtype, mode, seed=sum(shape) + mode)
                    run(exe, workdir, x, mode, CV.pages_torch(x, mode), f"{shape} {dtype} mode {mode}")
                    count += 1
        with np.load(os.path.join(ROOT, "tests", "golden", "convert.npz")) as z:
            x = torch.from_numpy(z["every_fp16_store_in"].copy())
            for mode, name in ((1, "every_fp16_store"), (2, "every_fp16_trch")):
                run(exe, workdir, x, mode, torch.from_numpy(z[name + "_out"]), f"{name} against the reference")
                count += 1
    print(f"{count} cases, no sanitizer report, no mismatch")


if __name__ == "__main__":
    main()
