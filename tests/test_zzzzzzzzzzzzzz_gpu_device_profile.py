"""TSX_ZSTD_PROFILE_DEVICE on the device: every case of tests/golden/device_profile_frames.json in one batch - each chunk passes
(tests/device_profile_cases.py) and each frame's SHA-256 is the one the CPU emulator computed, so device and emulator agree lane for lane:
the device is the only place where a wave's lanes really run in lockstep.  Then the full chain in the three memory kinds with a round
trip, verify on upload, and the profile side by side with the exact level-3 parse from 8 threads.  A digest that differs is a finding
about a phase of the parse that is not separated as csrc/zstd_enc_devparse.h says - not about this test."""
import functools
import threading

import pytest

import tsxform
from tests import device_profile_cases as dc
from tests import level_cases as lc
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
FOUR = ["K_262145", "B_131079", "zeros_131072", "twin_1048589"]


@functools.lru_cache(maxsize=1)
def _cases():
    names = dc.names() + dc.BIG
    return names, [dc.case(n) for n in names]


@functools.lru_cache(maxsize=1)
def _batch(gpu):
    names, chunks = _cases()
    return dc.run(gpu, nat.COMPRESS, chunks)


def test_every_golden_case_passes_in_one_batch(gpu, oracle):
    names, chunks = _cases()
    frames, d = _batch(gpu)
    dc.check_pass(gpu, oracle, chunks, frames, d, names)


def test_every_frame_is_the_emulators(gpu):
    names, chunks = _cases()
    frames, d = _batch(gpu)
    want = dc.golden()
    assert sorted(want) == sorted(names)
    differ = [n for n, f in zip(names, frames) if dc.digest(f) != {k: want[n][k] for k in ("size", "sha256")}]
    assert not differ, "device and emulator disagree on %d of %d frames: %s" % (len(differ), len(names), differ[:8])


@pytest.mark.parametrize("mem", [None, "device", "packed"])
def test_full_chain_round_trips_in_every_memory_kind(gpu, oracle, mem):
    chunks = [dc.case(n) for n in FOUR]
    outs, d = dc.run(gpu, FULL, chunks, mem=mem)
    want = dc.golden()
    for i, (n, c) in enumerate(zip(FOUR, chunks)):
        assert d["status"][i] == 0, (n, int(d["status"][i]))
        assert int(d["crc32c"][i]) == oracle.crc32c(c.tobytes()), n
        frame = oracle.gcm_decrypt_chunk(synth.KEY, synth.AAD, outs[i])
        assert dc.digest(frame) == {k: want[n][k] for k in ("size", "sha256")}, n
    lc.check_roundtrip(gpu, FULL, chunks, outs)


def test_verify_on_upload_accepts_the_whole_batch(gpu):
    names, chunks = _cases()
    flags = FULL | nat.VERIFY | nat.VERIFY_GCM
    outs, d = dc.run(gpu, flags, chunks)
    assert (d["status"] == 0).all(), [(n, int(s)) for n, s in zip(names, d["status"]) if s]
    plain, _ = _batch(gpu)
    assert [len(o_) for o_ in outs] == [len(f) + 28 for f in plain]


def test_profile_and_exact_level_3_side_by_side_from_8_threads(gpu, oracle):
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")
    chunks = [synth.gen_chunk("K" if i % 2 else "B", 91, 0, i, 256 << 10) for i in range(16)]
    exact = [oracle.zstd_compress_chunk(c.tobytes(), 3) for c in chunks]
    mine, d0 = dc.run(gpu, nat.COMPRESS, chunks)
    assert (d0["status"] == 0).all()
    errors = []

    def worker(t):
        try:
            for k in range(2):
                if (t + k) % 2:
                    outs, d = lc.run_transform(gpu, nat.COMPRESS, chunks, 3)
                    assert (d["status"] == 0).all() and outs == exact, "exact frames differ from the oracle's"
                else:
                    outs, d = dc.run(gpu, nat.COMPRESS, chunks)
                    assert (d["status"] == 0).all() and outs == mine, "the profile's frames depend on what ran beside them"
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append((t, repr(e)))
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for c, f in zip(chunks, mine):
        assert oracle.zstd_decompress_chunk(f) == c.tobytes()
