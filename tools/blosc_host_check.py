"""The Blosc / LZ4 decoder on the CPU under AddressSanitizer + UBSan, before any malformed stream reaches a device.

Compiles tools/blosc_host_check.cpp (skoots_amd/csrc/blosc.hip as host C++: the decoder text of blosc_lz4.inc with a lane
section = a loop over 64 lanes, plus the frame walk and sk_blosc_decode_host) with ``-fsanitize=address,undefined`` and
feeds it, as a plain program, the whole corpus of tests/blosc_corpus.py (hand-assembled streams, every truncation, every
single-bit flip, the named errors, the out-of-range table rows) and the golden frames of tests/golden/blosc.npz, every
item in allocations of exactly its sizes and at source and destination misalignments 0 to 7.  Status and bytes are
compared with the Python reference decoder (streams) and with the expected bytes (frames); truncated and bit-flipped
golden frames run for the sanitizers alone.  A sanitizer report ends the run with a non-zero exit code.

    python tools/blosc_host_check.py [--cxx g++] [--keep DIR]
"""
from __future__ import annotations

import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import blosc_corpus as C  # noqa: E402


def run(exe: str, items, work: str):
    """items: (mode, src_misalign, dst_misalign, row, src bytes, dst_bytes) -> [(status, dst bytes)]"""
    corpus, results = os.path.join(work, "corpus.bin"), os.path.join(work, "results.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for mode, smis, dmis, row, src, dst_bytes in items:
            f.write(struct.pack("<iiii5qqq", mode, smis, dmis, 0, *row, len(src), dst_bytes))
            f.write(src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    subprocess.run([exe, corpus, results], check=True, env=env)
    out = []
    with open(results, "rb") as f:
        for item in items:
            (status,) = struct.unpack("<i", f.read(4))
            out.append((status, f.read(item[5])))
    return out


def golden_frames():
    """(name, frame, expected bytes) of every frame of tests/golden/blosc.npz that must decode."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "blosc.npz"))
    out = C.good_frames(d)
    refuse = [(f"d:{name}", d[f"d_frame_{name}"].tobytes(), int(d["d_bytes"])) for name in d["d_names"]]
    return out, refuse


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", default=None, help="directory for the binary and the corpus files (default: temporary)")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="blosc_host_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "blosc_host_check")
    subprocess.run([args.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tools", "blosc_host_check.cpp")], check=True)
    bad = 0

    def judge(name, status, data, want_status, want):
        nonlocal bad
        ok = (status == 0 and data == want) if want is not None else (status != 0 and (not want_status or status == want_status))
        if not ok:
            bad += 1
            print(f"MISMATCH {name}: status {status}, wanted {'the bytes' if want is not None else want_status or 'a refusal'}")

    groups = [("hand_assembled", C.hand_assembled(), True), ("named_errors", C.named_errors() + C.good_neighbours(), True),
              ("truncations", C.truncations(), False), ("bit_flips", C.bit_flips(), False)]
    for name, cases, every in groups:
        t0 = time.perf_counter()
        variants = [(m, (m * 3 + 1) % 8 if m else 0) for m in range(8)] + [(0, m) for m in range(1, 8)] if every else [None]
        for v in variants:
            items = []
            for k, c in enumerate(cases):
                smis, dmis = v if v is not None else (k % 8, (k // 8) % 8)
                items.append((0, smis, dmis, (0, len(c.stream), 0, c.size, c.kind), c.stream, c.size))
            for c, (status, data) in zip(cases, run(exe, items, work)):
                want_status, want = C.decode(c.stream, c.size, c.kind)
                assert want == c.expect and (want is not None or not c.code or want_status == c.code), c.name
                judge(c.name, status, data, want_status, want)
        print(f"{name}: {len(cases)} streams x {len(variants)} alignments, {time.perf_counter() - t0:.1f} s", flush=True)

    rows = C.range_rows(40, 48)
    for k, (status, _) in enumerate(run(exe, [(0, k % 8, k % 5, r, bytes(40), 48) for k, r in enumerate(rows)], work)):
        judge(f"range_row{k}", status, None, C.E_RANGE, None)
    print(f"range_rows: {len(rows)} rows", flush=True)

    # the corpus again, every stream as the one split of a frame, through sk_blosc_decode_host
    framed = [(c, C.frame_of(c.stream, c.size)) for c in C.all_cases() if c.kind == C.KIND_LZ4]
    framed = [(c, f) for c, f in framed if f is not None]
    items = [(1, k % 8, (k // 8) % 8, (0, 0, 0, 0, 0), f, c.size) for k, (c, f) in enumerate(framed)]
    for (c, _), (status, data) in zip(framed, run(exe, items, work)):
        judge("framed:" + c.name, status, data, c.code, c.expect)
    print(f"framed corpus: {len(framed)} frames", flush=True)

    good, refuse = golden_frames()
    for mis in range(8):
        items = [(1, mis, (mis * 5 + 2) % 8, (0, 0, 0, 0, 0), f, len(raw)) for _, f, raw in good]
        for (name, _, raw), (status, data) in zip(good, run(exe, items, work)):
            judge(name, status, data, 0, raw)
    for (name, _, _), (status, _) in zip(refuse, run(exe, [(1, 3, 5, (0, 0, 0, 0, 0), f, n) for _, f, n in refuse], work)):
        judge(name, status, None, C.E_CODEC, None)
    hurt = [(n, C.damaged(f), raw) for n, f, raw in good if n[0] in "ab"]      # the chunks of the two stores
    for (name, _, _), (status, _) in zip(hurt, run(exe, [(1, 1, 6, (0, 0, 0, 0, 0), f, len(raw)) for _, f, raw in hurt], work)):
        judge("damaged:" + name, status, None, C.E_OFFSET, None)
    print(f"golden frames: {len(good)} x 8 alignments, {len(refuse)} to refuse, {len(hurt)} damaged", flush=True)

    # truncations and bit flips of whole frames (header, block table, split prefixes): for the sanitizers alone, except
    # that a frame cut short must be refused (cbytes no longer fits)
    small = [(n, f, raw) for n, f, raw in good if len(f) <= 4000]
    items, cut = [], []
    for name, f, raw in small:
        for n in range(0, len(f), max(1, len(f) // 200)):
            items.append((1, n % 8, n % 7, (0, 0, 0, 0, 0), f[:n], len(raw)))
            cut.append(f"{name}[:{n}]")
    for name, (status, _) in zip(cut, run(exe, items, work)):
        judge(name, status, None, 0, None)
    items = []
    for name, f, raw in small:
        for bit in range(0, 8 * min(len(f), 160)):
            t = bytearray(f)
            t[bit >> 3] ^= 1 << (bit & 7)
            items.append((1, bit % 8, bit % 5, (0, 0, 0, 0, 0), bytes(t), len(raw)))
    run(exe, items, work)
    print(f"frame mutations: {len(cut)} truncations, {len(items)} bit flips in headers and tables", flush=True)
    print("mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
