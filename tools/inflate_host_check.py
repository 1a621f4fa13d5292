"""The inflate decoder on the CPU under AddressSanitizer + UBSan, before any malformed stream reaches a device.

Compiles tools/inflate_host_check.cpp (the text of skoots_amd/csrc/inflate.hip as host C++, a lane section = a loop over
64 lanes) with ``-fsanitize=address,undefined``, feeds it the whole corpus of tests/test_hip_inflate.py
(tests/inflate_corpus.py: payloads x encoders, hand-assembled streams, every truncation, every single-bit flip, the
named errors) with every stream in allocations of exactly its sizes, and compares status and bytes with the stdlib's
zlib.  A sanitizer report ends the run with a non-zero exit code.

    python tools/inflate_host_check.py [--cxx g++] [--keep DIR] [--no-big]
"""
from __future__ import annotations

import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import inflate_corpus as C  # noqa: E402


def run(exe: str, cases, work: str, misalign=None):
    corpus, results = os.path.join(work, "corpus.bin"), os.path.join(work, "results.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for k, c in enumerate(cases):
            mis = (k % 8) if misalign is None else misalign
            f.write(struct.pack("<iiqq", c.wrapper, mis, len(c.stream), c.size))
            f.write(c.stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    subprocess.run([exe, corpus, results], check=True, env=env)
    out = []
    with open(results, "rb") as f:
        for c in cases:
            (status,) = struct.unpack("<i", f.read(4))
            out.append((status, f.read(c.size)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", default=None, help="directory for the binary and the corpus files (default: temporary)")
    ap.add_argument("--no-big", action="store_true", help="leave out the 1 MiB payloads and the 8 MiB chunk")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="inflate_host_check_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "inflate_host_check")
    subprocess.run([args.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tools", "inflate_host_check.cpp")], check=True)
    groups = [(name, C.encoded(name, big=not args.no_big)) for name in C.ENCODERS]
    if not args.no_big:
        chunk = C.chunk_payload()
        groups.append(("chunk_8MiB", [C.Case(f"{n}:chunk", fn(chunk), w, len(chunk), chunk)
                                      for n, (w, fn) in C.ENCODERS.items() if n in ("level0", "level1", "level6", "raw")]))
    groups += [("hand_assembled", C.hand_assembled()), ("truncations", C.truncations()), ("bit_flips", C.bit_flips()),
               ("named_errors", C.named_errors() + C.good_neighbours())]
    bad = 0
    for name, cases in groups:
        t0 = time.perf_counter()
        variants = [None] if name not in ("hand_assembled", "named_errors") else list(range(8))
        for mis in variants:
            for c, (status, data) in zip(cases, run(exe, cases, work, mis)):
                want = C.oracle(c.stream, c.wrapper, c.size)
                assert want == c.expect or c.expect is None, c.name
                ok = (status == 0 and data == want) if want is not None else status != 0
                if ok and c.code and status != c.code:
                    ok = False
                if not ok:
                    bad += 1
                    print(f"MISMATCH {c.name}: status {status}, zlib {'accepts' if want is not None else 'refuses'}, "
                          f"code wanted {c.code}")
        print(f"{name}: {len(cases)} streams x {len(variants)} alignments, {time.perf_counter() - t0:.1f} s", flush=True)
    print("mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
