#!/usr/bin/env python3
"""Writes tests/golden/device_profile_frames.json: SHA-256 and size of the frame TSX_ZSTD_PROFILE_DEVICE makes of every case of
tests/device_profile_cases.py (every content at every size, the far-period case, one 4 MiB K and one 4 MiB B chunk), computed by the CPU
emulator.  A frame of this profile is a function of the chunk's bytes and the flags only, so the emulator (lanes are fibers) and the
device (lanes in lockstep) must agree on every digest: tests/test_emu_zstd_device_profile.py compares the cases up to 1 MiB,
tests/test_zzzzzzzzzzzzzz_gpu_device_profile.py all of them.
Then tests/golden/device_profile_fuzz_frames.json, the same for the second family (96 seeded fuzz inputs, the window's edge, the aimed block
sequences, one 6 MiB and one 10 MiB chunk) together with its census - what the set reaches, printed as well (profiles/
device_profile_fuzz_census.txt is this printout): tests/test_emu_zstd_device_profile_fuzz.py and
tests/test_zzzzzzzzzzzzzzz_gpu_device_profile_fuzz.py.  usage: python tests/golden/make_device_profile_frames.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tsxform  # noqa: E402
from tests import device_profile_cases as dc  # noqa: E402
from tests.emu import emu_native  # noqa: E402

nat = tsxform._native


def write(path, names, chunks, frames, **more):
    out = dict({"flags": "TSX_COMPRESS", "frames": {n: dict(dc.digest(f), chunk=int(c.size)) for n, f, c in zip(names, frames, chunks)}}, **more)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%s: %d frames" % (os.path.relpath(path, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))), len(names)))


def print_census(title, c):
    b = c["blocks"]
    print("%-22s %3d frames  blocks: %d compressed, %d raw, %d RLE  raw->compressed %d, RLE->compressed %d (first sequence with literals: %d)" % (
        title, c["frames"], b["compressed"], b["raw"], b["rle"], c["raw_to_compressed"], c["rle_to_compressed"], c["raw_or_rle_to_compressed_first_ll_gt_0"]))
    print("%-22s largest literal length %d  largest offset %d  offsets in (2^21 - 4096, 2^21]: %d, at 2^21: %d  repeat code: %d of %d sequences (%.2f %%)" % (
        "", c["max_lit_length"], c["max_offset"], c["offsets_near_window"], c["offsets_at_window"], c["repeat_code_sequences"], c["sequences"],
        100.0 * c["repeat_code_sequences"] / max(c["sequences"], 1)))


def main():
    emu = emu_native.get()
    names = dc.names() + dc.BIG
    chunks = [dc.case(n) for n in names]
    frames, d = dc.run(emu, nat.COMPRESS, chunks)
    assert (d["status"] == 0).all()
    write(dc.GOLDEN, names, chunks, frames)

    names = dc.fuzz_names()
    chunks = [dc.fuzz_case(n) for n in names]
    frames, d = dc.run(emu, nat.COMPRESS, chunks)
    assert (d["status"] == 0).all()
    families = (("fuzz", dc.FUZZ), ("edge", dc.EDGE), ("aimed", dc.AIMED), ("big", dc.BIG_EMU + dc.BIG_DEVICE))
    for title, family in families:
        print_census(title, dc.census([frames[names.index(n)] for n in family]))
    for n in dc.EDGE + dc.AIMED + dc.BIG_EMU + dc.BIG_DEVICE:
        print_census(n, dc.census([frames[names.index(n)]]))
    whole = dc.census(frames)
    print_census("the whole family", whole)
    write(dc.FUZZ_GOLDEN, names, chunks, frames, census=whole)


if __name__ == "__main__":
    main()
