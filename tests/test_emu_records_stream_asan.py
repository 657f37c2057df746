"""The record-batch validator's bounds on a stream given in several calls, under AddressSanitizer: tests/emu/asan_records_stream.cpp, one
stand-alone executable of the emulated sources and a C++ driver (csrc/Makefile, emu-asan-records-stream), runs the boundary and damage
matrices of tests/test_emu_records_stream.py with every call's source in a heap block that ends with the call's last byte and the state
in a block of exactly its 192 bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiered-storage-for-apache-kafka_amd", "csrc")


def test_no_read_of_the_validator_leaves_the_bytes_of_the_call_it_serves():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emu-asan-records-stream"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tests", "emu", "_build", "asan_records_stream")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert " runs, 0 failed" in r.stdout and int(r.stdout.split("asan records stream: ")[1].split(" runs")[0]) >= 150, r.stdout[-2000:]
