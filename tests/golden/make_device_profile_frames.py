#!/usr/bin/env python3
"""Writes tests/golden/device_profile_frames.json: SHA-256 and size of the frame TSX_ZSTD_PROFILE_DEVICE makes of every case of
tests/device_profile_cases.py (every content at every size, the far-period case, one 4 MiB K and one 4 MiB B chunk), computed by the CPU
emulator.  A frame of this profile is a function of the chunk's bytes and the flags only, so the emulator (lanes are fibers) and the
device (lanes in lockstep) must agree on every digest: tests/test_emu_zstd_device_profile.py compares the cases up to 1 MiB,
tests/test_zzzzzzzzzzzzzz_gpu_device_profile.py all of them.  usage: python tests/golden/make_device_profile_frames.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tsxform  # noqa: E402
from tests import device_profile_cases as dc  # noqa: E402
from tests.emu import emu_native  # noqa: E402

nat = tsxform._native


def main():
    emu = emu_native.get()
    names = dc.names() + dc.BIG
    chunks = [dc.case(n) for n in names]
    frames, d = dc.run(emu, nat.COMPRESS, chunks)
    assert (d["status"] == 0).all()
    out = {"flags": "TSX_COMPRESS", "frames": {n: dict(dc.digest(f), chunk=int(c.size)) for n, f, c in zip(names, frames, chunks)}}
    with open(dc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dc.GOLDEN, len(names))


if __name__ == "__main__":
    main()
