"""The record walk's bounds under AddressSanitizer: tests/emu/asan_records_frames.cpp, one stand-alone executable of the emulated sources
and a C++ driver (csrc/Makefile, emu-asan-records-frames), runs the damage matrix of tests/test_emu_records_frames.py - and lengths,
counts and header counts of 2^31 - 1 - with everything around the chunks out of bounds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiered-storage-for-apache-kafka_amd", "csrc")


def test_no_read_of_the_record_walk_leaves_the_chunks_on_damaged_batches():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan-records-frames"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tests", "emu", "_build", "asan_records_frames")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert " runs, 0 failed" in r.stdout and int(r.stdout.split("asan records frames: ")[1].split(" runs")[0]) >= 290, r.stdout[-2000:]
