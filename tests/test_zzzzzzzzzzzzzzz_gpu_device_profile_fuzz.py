"""TSX_ZSTD_PROFILE_DEVICE on the device, second family (tests/device_profile_cases.py): the 96 seeded fuzz inputs, the window-edge pairs
and the aimed block sequences in one batch - about a hundred waves parsing side by side - and the 6 MiB and 10 MiB chunks in a second one.
Every frame's SHA-256 is the one the CPU emulator computed (tests/golden/device_profile_fuzz_frames.json), and a frame with that digest is
the frame tests/test_emu_zstd_device_profile_fuzz.py validated: the Python inspector runs only on a frame whose digest differs, and what it
says goes into the failure message.  libzstd and both device decoder forms restore every chunk; the batch in reversed order and chunks
alone give the same frames; verify on upload accepts the batch.  A digest that differs is a finding about a phase of the parse that is
not separated as csrc/zstd_enc_devparse.h says - not about this test."""
import functools

import pytest

import tsxform
from tests import device_profile_cases as dc

nat = tsxform._native
pytestmark = pytest.mark.gpu
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
FIRST = dc.FUZZ + dc.EDGE + dc.AIMED
SECOND = dc.BIG_EMU + dc.BIG_DEVICE
ALONE = ["fuzz_037", "fuzz_064", "fuzz_080"]                          # small, collision, accel


@functools.lru_cache(maxsize=None)
def _chunks(which):
    return [dc.fuzz_case(n) for n in (FIRST if which == "first" else SECOND)]


@functools.lru_cache(maxsize=None)
def _batch(gpu, which):
    return dc.run(gpu, nat.COMPRESS, _chunks(which))


def _verdict(oracle, name, frame, chunk):
    """What tests/device_profile_cases.check_frame says about a frame the emulator did not make."""
    try:
        dc.check_frame(oracle, frame, chunk, dc.label(name))
    except Exception as e:                                              # noqa: BLE001 (part of the report)
        return "%s: %d bytes, INVALID: %r" % (dc.label(name), len(frame), e)
    return "%s: %d bytes, a valid frame of the chunk" % (dc.label(name), len(frame))


@pytest.mark.parametrize("which", ["first", "second"])
def test_every_frame_is_the_emulators(gpu, oracle, which):
    names, chunks = (FIRST if which == "first" else SECOND), _chunks(which)
    frames, d = _batch(gpu, which)
    assert (d["status"] == 0).all(), [(n, int(s)) for n, s in zip(names, d["status"]) if s]
    want = dc.fuzz_golden()["frames"]
    assert sorted(want) == sorted(FIRST + SECOND)
    differ = [i for i, (n, f, c) in enumerate(zip(names, frames, chunks)) if dict(dc.digest(f), chunk=int(c.size)) != want[n]]
    assert not differ, "device and emulator disagree on %d of %d frames:\n%s" % (
        len(differ), len(names), "\n".join(_verdict(oracle, names[i], frames[i], chunks[i]) for i in differ[:6]))


@pytest.mark.parametrize("which", ["first", "second"])
def test_libzstd_and_both_decoder_forms_restore_every_chunk(gpu, oracle, which):
    names, chunks = (FIRST if which == "first" else SECOND), _chunks(which)
    frames, d = _batch(gpu, which)
    for n, f, c in zip(names, frames, chunks):
        assert oracle.zstd_decompress_chunk(f) == c.tobytes(), "%s: libzstd does not restore the chunk" % dc.label(n)
    dc.check_decoders(gpu, chunks, frames)


def test_frames_do_not_depend_on_neighbours_or_slots(gpu):
    chunks = _chunks("first")
    frames, d = _batch(gpu, "first")
    back, db = dc.run(gpu, nat.COMPRESS, chunks[::-1])
    assert (db["status"] == 0).all()
    differ = [dc.label(n) for n, a, b in zip(FIRST, frames, back[::-1]) if a != b]
    assert not differ, "frames change with the batch's order: %s" % differ[:8]
    for n in ALONE:
        alone, da = dc.run(gpu, nat.COMPRESS, [chunks[FIRST.index(n)]])
        assert da["status"][0] == 0 and alone[0] == frames[FIRST.index(n)], "%s alone gives another frame" % dc.label(n)


def test_verify_on_upload_accepts_the_first_batch(gpu):
    chunks = _chunks("first")
    plain, _ = _batch(gpu, "first")
    outs, d = dc.run(gpu, FULL | nat.VERIFY | nat.VERIFY_GCM, chunks)
    assert (d["status"] == 0).all(), [(dc.label(n), int(s)) for n, s in zip(FIRST, d["status"]) if s]
    assert [len(o_) for o_ in outs] == [len(f) + 28 for f in plain]
