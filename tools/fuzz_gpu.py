#!/usr/bin/env python3
"""Differential campaign on the device: the product library against the real libzstd 1.5.7 (oracle) on structured random inputs
(tests/fuzz_cases.py) - many small/medium cases plus full 4 MiB chunks whose copies reach beyond the 2 MiB window.  Test
infrastructure (uses oracle/).   python tools/fuzz_gpu.py --cases 3000 --big 96 --seed 7 > gpurun_out/fuzz_gpu.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (one HIP runtime)
import tsxform  # noqa: E402
from tests import parity_cases as pc  # noqa: E402
from tests import keying_cases as kc  # noqa: E402
from tests import level_cases as lc  # noqa: E402
from tests.fuzz_cases import LEVEL_WINDOW, gen_case, level_case  # noqa: E402

nat = tsxform._native


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--big", type=int, default=64)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--level", type=int, choices=(1, 2, 3), default=3, help="1 and 2 (strategy fast): cases from all four generators of tests/fuzz_cases.py, "
                                                                            "the big ones sized from the level's window (512 KiB / 1 MiB) instead of 4 MiB")
    args = ap.parse_args()
    from oracle import oracle as o
    o.build()
    assert o.zstd_version().startswith("1.5.7"), o.zstd_version()
    N = tsxform.get()
    rng = np.random.default_rng(args.seed)
    t0 = time.time(); bad = 0; done = 0; nbytes = 0
    level = args.level

    def run(cases, label):
        nonlocal bad, done, nbytes
        outs, d = lc.run_transform(N, nat.COMPRESS, cases, level, mem="device")
        back, d2 = pc.run_detransform(N, nat.COMPRESS, outs, [int(c.size) for c in cases])
        for i, c in enumerate(cases):
            exp = o.zstd_compress_chunk(c.tobytes(), level)
            if d["status"][i] != 0 or outs[i] != exp:
                bad += 1; print("MISMATCH %s case %d size %d status %d" % (label, done + i, c.size, d["status"][i]), flush=True)
                c.tofile(os.path.join(ROOT, "gpurun_out", "fuzz_gpu_bad_%s_%d.bin" % (label, done + i)))
            if d2["status"][i] != 0 or back[i] != c.tobytes():
                bad += 1; print("DECODE MISMATCH %s case %d size %d status %d" % (label, done + i, c.size, d2["status"][i]), flush=True)
        done += len(cases); nbytes += sum(int(c.size) for c in cases)

    if level != 3:
        return fast_levels(args, o, N, rng, run, lambda: (bad, done, nbytes, time.time() - t0))
    for lo in range(0, args.cases, 256):
        run([gen_case(rng) for _ in range(min(256, args.cases - lo))], "small")
    print("[%5.0fs] %d cases, %.1f MB, %d bad" % (time.time() - t0, done, nbytes / 1e6, bad), flush=True)
    for lo in range(0, args.big, 32):
        run([gen_case(rng, 4194304 - int(rng.integers(0, 3)) * int(rng.integers(0, 70000))) for _ in range(min(32, args.big - lo))], "big")
    # the chain on a sample (CRC head + GCM tail in the compressor wave), under a key, AAD and segment drawn from the seed, and back
    sample = [gen_case(rng) for _ in range(96)] + [gen_case(rng, 4194304) for _ in range(4)]
    key, aad, seg = kc.draw(rng, int(rng.integers(0, 65)))
    try:
        kc.check_keyed(N, o, nat.COMPRESS | nat.ENCRYPT | nat.CRC, sample, key, aad, seg, "chain")
    except AssertionError as e:
        bad += 1; print("CHAIN MISMATCH:", e, flush=True)
    print("DONE seed %d: %d cases (%d of 4 MiB), %.1f MB, %d bad, %.0f s; libzstd %s" % (args.seed, done, args.big, nbytes / 1e6, bad, time.time() - t0, o.zstd_version()), flush=True)
    sys.exit(1 if bad else 0)


def fast_levels(args, o, N, rng, run, totals):
    """Levels 1 and 2: --cases inputs, one in four from each of gen_case / collision_case / accel_case / straddle_case, then --big structured
    inputs of W .. W + 300000 bytes and as many straddling ones (a mismatching input is written with the level in its name); frames against
    libzstd at the level, the device decoder, the chain on a sample."""
    level = args.level
    kinds = ("small", "collision", "accel", "straddle")
    for lo in range(0, args.cases, 128):
        run([level_case(rng, level, kinds[(lo + i) % 4]) for i in range(min(128, args.cases - lo))], "level%d_mixed" % level)
        if lo % 1024 == 0:
            bad, done, nbytes, secs = totals()
            print("[%5.0fs] %d cases, %.1f MB, %d bad" % (secs, done, nbytes / 1e6, bad), flush=True)
    for lo in range(0, args.big, 32):
        run([level_case(rng, level, "big") for _ in range(min(32, args.big - lo))], "level%d_big" % level)
        run([level_case(rng, level, "straddle") for _ in range(min(32, args.big - lo))], "level%d_straddle" % level)
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    sample = [gen_case(rng) for _ in range(92)] + [level_case(rng, level, k) for k in kinds]
    bad, done, nbytes, secs = totals()
    try:
        outs, _ = lc.check_vs_oracle(N, o, flags, sample, level)
        lc.check_roundtrip(N, flags, sample, outs)
    except AssertionError as e:
        bad += 1; print("CHAIN MISMATCH:", e, flush=True)
    print("DONE level %d seed %d: %d cases (%d + %d sized from the %d KiB window), %.1f MB, %d bad, %.0f s; libzstd %s"
          % (level, args.seed, done, args.big, args.big, LEVEL_WINDOW[level] >> 10, nbytes / 1e6, bad, totals()[3], o.zstd_version()), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
