"""Zstandard content checksum under the CPU emulator: TSX_COMPRESS | TSX_ZSTD_CHECKSUM frames are the real libzstd 1.5.7's bytes with
ZSTD_c_checksumFlag (the last four pin the wave-level XXH64 on every length class), both decoder forms verify every frame that
declares a checksum and agree on the verdict, and the flag is validated.  Full-size chunks and the real lane exchange run on the
device (tests/test_zzzzzzz_gpu_zstd_checksum.py)."""
import ctypes
import threading
import time

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native


# ---- 1. byte identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3])
def test_checksummed_frames_are_byte_identical_to_libzstd(emu, oracle, level):
    """Every size of the matrix (no stripe loop, exact multiples of 32, tails that take the 8-byte, the 4-byte and the 1-byte steps),
    contents K / incompressible (raw blocks) / zeros (RLE blocks); profile 1.5.6 on the K cases whose frames the pre-splitter does not
    touch (the checksum does not depend on the splitter)."""
    cc.need157(oracle)
    for name in ("K", "R", "zero"):
        chunks = [cc.contents(n)[name] for n in cc.SIZES]
        outs, d, _ = cc.run_transform(emu, cc.CK, chunks, level)
        for i, c in enumerate(chunks):
            want = cc.frame(oracle, c, level)
            assert d["status"][i] == 0 and outs[i] == want, "%s, %d bytes, level %d: frame differs from libzstd's" % (name, c.size, level)
            assert want[4] & 4 and want[5:-4] == cc.frame(oracle, c, level, checksum=False)[5:]
    chunks = [cc.contents(n)["K"] for n in cc.SIZES]
    outs6, d6, _ = cc.run_transform(emu, cc.CK, chunks, level, profile=nat.ZSTD_PROFILE_1_5_6)
    for i, c in enumerate(chunks):
        want = cc.frame(oracle, c, level)
        assert d6["status"][i] == 0
        # libzstd's four bytes whatever the splitter did, and libzstd (which verifies them) restores the input; the pre-splitter works on
        # full blocks behind the first: below two full blocks the whole frame is libzstd 1.5.7's
        assert outs6[i][4] & 4 and outs6[i][-4:] == want[-4:], c.size
        assert oracle.zstd_decompress_chunk(outs6[i], c.size) == c.tobytes()
        if c.size < 262144:
            assert outs6[i] == want, c.size


def test_the_wave_hash_at_odd_and_8_byte_offsets(emu, oracle):
    """xxh64_wave itself (test hook tsx_debug_xxh64) on inputs that start at odd addresses and at multiples of 8: its low 32 bits
    are the last four bytes of libzstd's checksummed frame of the same bytes; the empty input's hash is the published constant."""
    cc.need157(oracle)
    assert cc.device_xxh64(emu, np.zeros(0, np.uint8), [0, 3]) == [0xEF46DB3751D8E999] * 2
    offsets = [0, 1, 3, 5, 7, 8, 24, 33]
    for n in cc.SIZES:
        for name in ("K", "R"):
            x = cc.contents(n)[name]
            want = int.from_bytes(cc.frame(oracle, x)[-4:], "little")
            got = cc.device_xxh64(emu, x, offsets if n <= 1000 else [1, 8])
            assert [g & 0xFFFFFFFF for g in got] == [want] * len(got), (n, name)
            assert len(set(got)) == 1


# ---- 2. full chain -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [None, "device", "packed"])
def test_full_chain_with_checksum_matches_libzstd_and_the_oracles_gcm(emu, oracle, mem):
    cc.need157(oracle)
    flags = cc.CK | nat.ENCRYPT | nat.CRC
    chunks = [synth.gen_chunk("K", 9, 2, 0, 150000), synth.gen_chunk("R", 9, 2, 1, 65537), synth.gen_chunk("K", 9, 2, 2, 17),
              np.zeros(0, np.uint8), np.zeros(140000, np.uint8)]
    outs, d, _ = cc.run_transform(emu, flags, chunks, 3, mem=mem)
    for i, c in enumerate(chunks):
        want = oracle.gcm_encrypt_chunk(synth.KEY, synth.iv_for(0, i), synth.AAD, cc.frame(oracle, c, 3))
        assert d["status"][i] == 0 and outs[i] == want, (mem, i)
        assert int(d["crc32c"][i]) == oracle.crc32c(c.tobytes())
    back, d2 = pc.run_detransform(emu, flags, outs, [int(c.size) for c in chunks])
    for i, c in enumerate(chunks):
        assert d2["status"][i] == 0 and back[i] == c.tobytes() and d2["crc32c"][i] == d["crc32c"][i], (mem, i)


def test_staged_path_emits_the_same_bytes(emu, oracle):
    """The stages as separate launches (test hook stages_separate): the frame waits in the staging buffer with its checksum on."""
    cc.need157(oracle)
    chunks = [synth.gen_chunk("K", 9, 4, 0, 70000), np.zeros(0, np.uint8), synth.gen_chunk("R", 9, 4, 1, 1000)]
    for flags in (cc.CK, cc.CK | nat.ENCRYPT | nat.CRC):
        fused, _, _ = cc.run_transform(emu, flags, chunks, 3)
        with emu.configured(stages_separate=1):
            staged, d, _ = cc.run_transform(emu, flags, chunks, 3)
        assert (d["status"] == 0).all() and staged == fused
    assert fused[0][12:-16] != b"" and cc.run_transform(emu, cc.CK, chunks, 3)[0] == [cc.frame(oracle, c, 3) for c in chunks]


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [None, "device"])
def test_a_slot_without_room_for_the_checksum_is_too_small(emu, oracle, mem):
    """dst_cap = frame size: fine.  One to four bytes less - room for the checksum-free frame at most - TSX_E_DST_TOO_SMALL, and the 32
    guard bytes behind the slot stay as they were."""
    cc.need157(oracle)
    x = synth.gen_chunk("K", 9, 5, 0, 50000)
    flen = len(cc.frame(oracle, x, 3))
    for flags, extra in ((cc.CK, 0), (cc.CK | nat.ENCRYPT | nat.CRC, 28)):
        shorts = [0, 1, 2, 3, 4]
        outs, d, guards = cc.run_transform(emu, flags, [x] * len(shorts), 3, mem=mem, dst_caps=[flen + extra - s for s in shorts], guard=32)
        assert d["status"][0] == 0 and d["dst_len"][0] == flen + extra
        assert list(d["status"][1:]) == [nat.E_DST_TOO_SMALL] * 4 and (d["dst_len"][1:] == 0).all(), (flags, list(d["status"]))
        assert all(g == b"\xEE" * 32 for g in guards), flags
    assert outs[0][12:-16] != b""


# ---- 4. decoding ---------------------------------------------------------------------------------------------------------
def _decode_inputs():
    K = synth.gen_chunk("K", 21, 0, 0, 300007)
    return [K[:1000], K[:200000], K]


@pytest.mark.parametrize("level", [1, 3, 19])
def test_libzstds_checksummed_frames_decode_in_both_forms(emu, oracle, level):
    cc.need157(oracle)
    inputs = _decode_inputs()
    blobs = [cc.frame(oracle, x, level) for x in inputs]
    res = cc.decode_both_forms(emu, nat.COMPRESS | nat.CRC, blobs, [int(x.size) for x in inputs])
    for form, (outs, d, kept) in res.items():
        assert (d["status"] == 0).all(), (form, level, list(d["status"]))
        assert outs == [x.tobytes() for x in inputs], (form, level)
        assert [int(c) for c in d["crc32c"]] == [oracle.crc32c(x.tobytes()) for x in inputs]
    assert res["block"][2] == len(blobs), "a checksummed frame left the block form"


# ---- 5. damage -----------------------------------------------------------------------------------------------------------
def test_damaged_checksummed_frames_are_bad_frames_in_both_forms(emu, oracle):
    """The four checksum bytes, a byte of a raw block's body, a byte of a raw literals section: libzstd rejects each one
    (cc.damage_cases asserts it), and so do both forms, with the treatment every corrupt frame gets.  The same body damage on the
    checksum-free frame of the same input is invisible, as it always was: TSX_OK and the bytes libzstd restores."""
    cc.need157(oracle)
    cases, controls = cc.damage_cases(oracle)
    assert len(cases) == 6
    res = cc.decode_both_forms(emu, nat.COMPRESS, [b for _, b, _ in cases], [s for _, _, s in cases])
    for form, (outs, d, kept) in res.items():
        assert list(d["status"]) == [nat.E_BAD_FRAME] * len(cases), (form, list(d["status"]))
        assert (d["dst_len"] == 0).all() and kept == (0 if form == "block" else -1), form
    res = cc.decode_both_forms(emu, nat.COMPRESS, [b for _, b, _, _ in controls], [s for _, _, s, _ in controls])
    for form, (outs, d, kept) in res.items():
        assert (d["status"] == 0).all() and outs == [w for _, _, _, w in controls], form


def test_only_the_damaged_chunk_of_a_mixed_batch_fails(emu, oracle):
    cc.need157(oracle)
    K = synth.gen_chunk("K", 21, 0, 0, 200000)
    rawlit = cc.rawlit_input(6000)
    f = cc.frame(oracle, rawlit, 3)
    at = cc.raw_sections(f)[1][0][0] + 7
    inputs = [K, K[:70000], rawlit, rawlit, K[:1000]]
    blobs = [cc.frame(oracle, K, 3), cc.frame(oracle, K[:70000], 3, checksum=False), cc.flip(f, at), f, cc.frame(oracle, K[:1000], 1)]
    assert cc.libzstd_rejects(oracle, blobs[2], rawlit.size) is not None
    res = cc.decode_both_forms(emu, nat.COMPRESS, blobs, [int(x.size) for x in inputs])
    for form, (outs, d, kept) in res.items():
        assert list(d["status"]) == [0, 0, nat.E_BAD_FRAME, 0, 0], (form, list(d["status"]))
        assert d["dst_len"][2] == 0
        for i in (0, 1, 3, 4):
            assert outs[i] == inputs[i].tobytes(), (form, i)
    assert res["block"][2] == 4


# ---- 6. validation -------------------------------------------------------------------------------------------------------
def test_the_flag_needs_compression_on_transform_and_is_ignored_on_detransform(emu, oracle):
    ck = nat.ZSTD_CHECKSUM
    assert ck == 8
    for flags in (ck, ck | nat.CRC, ck | nat.ENCRYPT, ck | nat.ENCRYPT | nat.CRC):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    for flags in (cc.CK, cc.CK | nat.CRC, cc.CK | nat.ENCRYPT | nat.CRC):
        assert cc.transform_rc(emu, flags) == 0, flags
    for flags in (16, 16 | cc.CK, 0x80000000 | nat.COMPRESS):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    x = synth.gen_chunk("K", 9, 6, 0, 30000)
    for blob in (cc.frame(oracle, x, 3), cc.frame(oracle, x, 3, checksum=False)):
        for flags in (cc.CK, nat.COMPRESS):                             # the frame decides, not the caller
            outs, d = pc.run_detransform(emu, flags, [blob], [x.size])
            assert d["status"][0] == 0 and outs[0] == x.tobytes()
    # the CRC-only entry point takes no flags at all
    d = pc.make_descs([x.size], [0], [0], [0])
    src = np.zeros(x.size + 16, np.uint8); src[:x.size] = x
    emu.crc32c_batch(d, src)
    assert int(d["crc32c"][0]) == oracle.crc32c(x.tobytes())


# ---- 7. hand-back --------------------------------------------------------------------------------------------------------
def test_a_chunk_handed_back_midway_still_gets_libzstds_checksum(emu, oracle):
    """A guest wave that gives its chunk up, and a wave the hardware moved onto a reserved CU: another wave starts the chunk again from
    its first byte and hashes it at its end - the frames are libzstd's, checksum included."""
    cc.need157(oracle)
    for f, t in (("hipemu_cu_key_shift", [ctypes.c_int]), ("hipemu_force_yield_after", [ctypes.c_int]), ("hipemu_relocate_after", [ctypes.c_int])):
        getattr(emu.lib, f).argtypes = t; getattr(emu.lib, f).restype = None
    flags = cc.CK | nat.ENCRYPT | nat.CRC
    sizes = [200000, 131072 + 5, 30001, 17]
    chunks = [synth.gen_chunk("K" if i % 3 else "B", 31, 1, i, s) for i, s in enumerate(sizes)]
    want = [oracle.gcm_encrypt_chunk(synth.KEY, synth.iv_for(0, i), synth.AAD, cc.frame(oracle, c, 3)) for i, c in enumerate(chunks)]
    with emu.configured(fetch_quiet_ms=1):
        time.sleep(0.01)
        emu.service_quiesce(0)
        s0 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(3)
        try:
            for after in (4, 3):
                time.sleep(0.01)
                emu.lib.hipemu_force_yield_after(after)
                got, d, _ = cc.run_transform(emu, flags, chunks, 3)
                assert got == want and (d["status"] == 0).all(), after
        finally:
            emu.lib.hipemu_cu_key_shift(0); emu.lib.hipemu_force_yield_after(0)
        emu.service_quiesce(0)
        s1 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(1)
        try:
            emu.lib.hipemu_relocate_after(4)
            got, d, _ = cc.run_transform(emu, flags, chunks, 3)
            assert got == want and (d["status"] == 0).all()
        finally:
            emu.lib.hipemu_relocate_after(0); emu.lib.hipemu_cu_key_shift(0)
    assert s1["returned_chunks"] - s0["returned_chunks"] >= 2, (s0, s1)


# ---- 8. concurrency ------------------------------------------------------------------------------------------------------
def test_members_with_and_without_the_flag_share_the_queue(emu, oracle):
    cc.need157(oracle)
    chunks = [synth.gen_chunk("K" if i % 2 else "B", 41, 0, i, 20000 + 9000 * i) for i in range(3)]
    want = {True: [cc.frame(oracle, c, 3) for c in chunks], False: [cc.frame(oracle, c, 3, checksum=False) for c in chunks]}
    errors = []

    def worker(on):
        try:
            outs, d, _ = cc.run_transform(emu, cc.CK if on else nat.COMPRESS, chunks, 3)
            assert (d["status"] == 0).all() and outs == want[on], on
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append((on, repr(e)))
    ts = [threading.Thread(target=worker, args=(on,)) for on in (True, False, True, False)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert all(a != b and a[5:-4] == b[5:] for a, b in zip(want[True], want[False]))
