"""Record framing and offset order (TSX_VALIDATE_FRAMES) under the CPU emulator: the flag's rules, clean segments on every path of the
front end, the damage matrix - every damage sealed with a valid CRC, on a batch inside a chunk, on a chunk's first byte, on the stream's
first and last batch, at 4099- and 65536-byte chunks - precedence, the cases in which the walkers' speculation loses, and a seeded fuzz:
all against tests/records_frames_cases.py::reference_walk_frames.  The same matrices run on the device in
tests/test_zzzzzzzzzzzzzzzzzz_gpu_records_frames.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import gcm_verify_cases as gv
from tests import parity_cases as pc
from tests import records_cases as rc
from tests import records_frames_cases as fc
from tsxform import synth

nat = tsxform._native
CE = nat.COMPRESS | nat.ENCRYPT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ctx(emu):
    h = emu.ctx_create(0, 0, 0)
    yield h
    emu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    s = rc.valid_segment(300000)
    counts = sum(int.from_bytes(s[p + 57:p + 61], "big") for p, l in rc.batches_of(s))
    assert len(s) == 290455 and fc.reference_walk_frames(s) == (19, 0, counts, rc.NONE, 0) and counts == 630
    return s


# ---- 1. the flag ------------------------------------------------------------------------------------------------------------
def test_the_flag_modifies_validate_records_and_the_streamed_form_refuses_it(emu, segment):
    f, r = getattr(nat, "VALIDATE_FRAMES", None), nat.VALIDATE_RECORDS
    assert f == 0x400
    header = open(os.path.join(ROOT, "include", "tsxform.h")).read()
    java = open(os.path.join(ROOT, "java", "io", "aiven", "kafka", "tieredstorage", "gpu", "TsxNative.java")).read()
    assert int(re.search(r"#define TSX_VALIDATE_FRAMES (0x[0-9a-fA-F]+)u", header).group(1), 16) == f
    assert int(re.search(r"int VALIDATE_FRAMES\s*=\s*(0x[0-9a-fA-F]+);", java).group(1), 16) == f
    assert "#define TSX_ABI_VERSION 4 " in header and nat.ABI_VERSION == 4
    ok = (0, nat.CRC, nat.ENCRYPT, nat.ENCRYPT | nat.CRC, nat.ENCRYPT | nat.VERIFY_GCM, nat.COMPRESS, nat.COMPRESS | nat.CRC, CE, CE | nat.CRC,
          CE | nat.ZSTD_CHECKSUM, CE | nat.VERIFY, CE | nat.VERIFY_GCM, CE | nat.CRC | nat.ZSTD_CHECKSUM | nat.VERIFY | nat.VERIFY_GCM)
    x = fc.batch(5, [fc.record(d, value=b"v" * 80) for d in range(9)])
    for flags in ok:
        assert cc.transform_rc(emu, flags | f) == nat.E_INVAL, flags         # without TSX_VALIDATE_RECORDS
        outs, d = rc.run(emu, flags | r | f, x, [len(x)])
        assert d["status"][0] == 0, flags
    assert cc.transform_rc(emu, f) == nat.E_INVAL
    for flags in (0x10 | CE | r | f, 0x40 | CE | r | f, 0x200 | CE | r | f, 0x800 | CE | r | f):     # the bits around it stay unassigned
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    y = synth.gen_chunk("K", 9, 6, 0, 30000)                            # no record batch: detransform does not look
    for flags in (nat.ENCRYPT, CE):
        outs, d = gv.run_transform(emu, flags, [y], "host")
        for more in (f, r | f):
            back, d2 = pc.run_detransform(emu, flags | more, outs, [y.size])
            assert d2["status"][0] == 0 and back[0] == y.tobytes(), flags
    # the streamed form: refused before anything is touched - the state stays bit for bit, the descriptors too
    st = emu.records_begin(len(x))
    before = bytes(st)
    sizes = [len(x)]
    soff, doff, caps, stt, dt = pc.layout(sizes, nat.CRC, emu)
    src = np.zeros(stt, np.uint8); src[soff[0]:soff[0] + len(x)] = np.frombuffer(x, np.uint8)
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps); d["status"][0] = 77
    p = nat.Native.make_params(nat.CRC | r | f, synth.KEY, synth.AAD)
    with pytest.raises(nat.TsxError) as e:
        emu.transform_batch(p, d, src, dst, dst.size, state=st)
    assert e.value.code == nat.E_UNSUPPORTED and bytes(st) == before and d["status"][0] == 77
    emu.transform_batch(nat.Native.make_params(nat.CRC | r, synth.KEY, synth.AAD), d, src, dst, dst.size, state=st)      # ... and goes on without it
    assert d["status"][0] == 0 and emu.records_result(st)[0] == 1


# ---- 2. clean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", rc.MEMS)
def test_a_clean_segment_passes_on_every_memory_kind_and_every_record_is_read(emu, ctx, segment, mem):
    sizes = rc.cut(segment, rc.CUT, (7,))
    want, d0 = rc.run(emu, nat.ENCRYPT | nat.CRC | rc.VR, segment, sizes, mem, ctx)
    rep0 = rc.info(emu, ctx)[4]
    outs, got, rep = fc.check(emu, nat.ENCRYPT | nat.CRC, segment, sizes, mem, ctx)
    assert got == (19, 0, 630, rc.NONE, 0) and rep == rep0 == 0 and outs == want and emu.ctx_records(ctx).ms > 0
    fc.check(emu, 0, segment, rc.cut(segment, 65536, (1,)), mem, None)      # a pooled context, the plain copy


def test_a_clean_segment_passes_behind_every_chain(emu, ctx, segment):
    for size in (rc.CUT, 65536, 1 << 20):
        outs, got, rep = fc.check(emu, nat.CRC, segment, rc.cut(segment, size, (2,)), "host", ctx)
        assert got == (19, 0, 630, rc.NONE, 0) and rep == 0
    fc.check(emu, nat.ENCRYPT, segment, rc.cut(segment, rc.CUT), "host", ctx, sub_bytes=40000)      # eight pieces
    small = segment[:rc.batches_of(segment)[3][0]]                       # (the emulated compressor is slow: three batches, 16 chunks)
    sizes = rc.cut(small, -(-len(small) // 16))
    want, got, rep = fc.check(emu, CE | nat.CRC, small, sizes, "zero_copy", ctx)
    assert got == fc.reference_walk_frames(small) and got[2] > 0 and rep == 0
    fc.check(emu, CE | nat.CRC, small, sizes, "packed", ctx, want=want)
    fc.check(emu, CE | nat.CRC | nat.VERIFY | nat.VERIFY_GCM, small, sizes, "zero_copy", None, want=want)


def test_the_built_stream_and_its_special_batches(emu, ctx):
    for name, s, exp in fc.special_streams():
        assert fc.reference_walk_frames(s)[3:] == exp, name
        for size in (rc.CUT, 65536):
            fc.check(emu, nat.CRC, s, fc.sizes_for(s, size), "host", ctx)


# ---- 3 + 4. damage: unseen by TSX_VALIDATE_RECORDS alone, found with the flag ----------------------------------------------------
@pytest.mark.parametrize("size", [rc.CUT, 65536])
def test_the_damage_matrix(emu, ctx, size):
    assert fc.damage_matrix(emu, ctx, size, nat.CRC) == len(fc.DAMAGE) * 4 == 124


# ---- speculation ----------------------------------------------------------------------------------------------------------------
def test_a_badly_framed_batch_inside_a_record_value_is_not_judged(emu, ctx):
    s = fc.nested_stream()
    ref = fc.reference_walk_frames(s)
    assert ref == (7, 0, 62, rc.NONE, 0)
    outs, got, rep = fc.check(emu, nat.CRC, s, rc.cut(s, rc.CUT), "host", ctx)
    assert rep >= 1                                                     # chunk 1's walker entered the inner batch; the resolver walked the chunk itself
    outs, got1, rep = fc.check(emu, nat.CRC, s, [len(s)], "host", ctx)
    assert got1 == got


def test_a_damaged_first_batch_of_a_chunk_is_repaired_with_the_uncut_result(emu, ctx, segment):
    first = {}
    for p, l in rc.batches_of(segment):
        first.setdefault(p // rc.CUT, (p, l))
    j, (p, l) = sorted(first.items())[3]
    assert j > 0 and p % rc.CUT
    for bad, why in ((rc.flip(segment, p + 20), rc.CRC), (fc.seal(rc.flip(segment[p:p + l], 57 + 3)), fc.RECORDS)):
        if why == fc.RECORDS:
            bad = segment[:p] + bad + segment[p + l:]
        outs, got, rep = fc.check(emu, nat.CRC, bad, rc.cut(bad, rc.CUT), "host", ctx)
        assert got[3:] == (p, why) and (rep >= 1 or why != rc.CRC)
        outs, uncut, rep = fc.check(emu, nat.CRC, bad, [len(bad)], "host", ctx)
        assert uncut == got


def test_the_seam_between_two_walkers_is_checked_by_the_resolver(emu, ctx):
    """Two batches whose offsets overlap, the second one beginning exactly on a chunk's first byte: its walker cannot know."""
    a = fc.batch(100, [fc.record(d, value=b"a" * 300) for d in range(10)])
    for base, why in ((109, fc.OFFSETS), (110, 0)):
        b = fc.batch(base, [fc.record(d, value=b"b" * 200) for d in range(10)], count=9 if base == 109 else None)      # (and a count that fails: the seam outranks it)
        s = a + b + fc.batch(500, [fc.record(0)])
        outs, got, rep = fc.check(emu, nat.CRC, s, [len(a), len(b), len(s) - len(a) - len(b)], "host", ctx)
        assert got == ((1, 0, 10, len(a), why) if why else (3, 0, 21, rc.NONE, 0)) and rep == 0


# ---- 5. fuzz --------------------------------------------------------------------------------------------------------------------
def test_seeded_fuzz_against_the_reference(emu, ctx, segment):
    """Seed 771, 300 single-byte mutations of the valid segment, every second one resealed (records_frames_cases.fuzz_cases)."""
    cases = fc.fuzz_cases(segment)
    assert len(cases) == 300 and (fc.FUZZ_SEED, fc.FUZZ_N) == (771, 300)
    want = {}
    sealed = caught = 0
    for s, size, resealed in cases:
        ref = fc.reference_walk_frames(s)
        sealed += resealed
        caught += resealed and ref[4] in (fc.RECORDS, fc.OFFSETS)
        sizes = rc.cut(s, size)
        outs, got, rep = fc.check(emu, 0, s, sizes, "host", ctx, want=[s[a:a + n] for a, n in zip(np.cumsum([0] + sizes), sizes)])
    assert sealed == 150 and 3 * caught >= sealed, (sealed, caught)
