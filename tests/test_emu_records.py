"""Record-batch validation (TSX_VALIDATE_RECORDS) under the CPU emulator: the flag's rules, a clean segment on every path of the front end,
headers split over chunks at every byte, one damaged byte at a time, hostile lengths and stream ends, and the cases in which the walkers'
speculation loses - all against tests/records_cases.py::reference_walk.  The same matrices run on the device in
tests/test_zzzzzzzzzzzz_gpu_records.py."""
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import gcm_verify_cases as gv
from tests import parity_cases as pc
from tests import records_cases as rc
from tsxform import synth

nat = tsxform._native
CE = nat.COMPRESS | nat.ENCRYPT


@pytest.fixture()
def ctx(emu):
    h = emu.ctx_create(0, 0, 0)
    yield h
    emu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    s = rc.valid_segment(300000)
    assert len(s) == 290455 and rc.reference_walk(s) == (19, 0, rc.NONE, 0)
    return s


# ---- 1. the flag ------------------------------------------------------------------------------------------------------------
def test_the_flag_goes_with_every_stage_combination_and_detransform_ignores_it(emu):
    r = nat.VALIDATE_RECORDS
    assert r == 0x100 and nat.E_RECORDS == -11 and "record batch" in emu.strerror(nat.E_RECORDS)
    ok = (0, nat.CRC, nat.ENCRYPT, nat.ENCRYPT | nat.CRC, nat.ENCRYPT | nat.VERIFY_GCM, nat.COMPRESS, nat.COMPRESS | nat.CRC, CE, CE | nat.CRC,
          CE | nat.ZSTD_CHECKSUM, CE | nat.VERIFY, CE | nat.VERIFY_GCM, CE | nat.CRC | nat.ZSTD_CHECKSUM | nat.VERIFY | nat.VERIFY_GCM)
    x = rc.make_batch(5, b"v" * 939)                                     # (transform_rc's one chunk has 1000 bytes; here the rule is what is asked)
    for flags in ok:
        assert cc.transform_rc(emu, flags) == 0, flags
        outs, d = rc.run(emu, flags | r, x, [len(x)])
        assert d["status"][0] == 0, flags
    for flags in (nat.VERIFY_GCM, nat.VERIFY, nat.ZSTD_CHECKSUM, nat.VERIFY | nat.ENCRYPT):    # what fails today fails with the flag too
        assert cc.transform_rc(emu, flags) == nat.E_INVAL and cc.transform_rc(emu, flags | r) == nat.E_INVAL, flags
    for flags in (0x10 | CE, 0x40 | CE, 0x10 | CE | r, 0x40 | CE | r, 0x200 | CE, 0x200 | CE | r):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    y = synth.gen_chunk("K", 9, 6, 0, 30000)                            # no record batch: detransform does not look
    for flags in (nat.ENCRYPT, CE):
        outs, d = gv.run_transform(emu, flags, [y], "host")
        back, d2 = pc.run_detransform(emu, flags | r, outs, [y.size])
        assert d2["status"][0] == 0 and back[0] == y.tobytes(), flags


def test_a_batch_without_chunks_or_without_bytes_is_a_clean_stream(emu, ctx):
    outs, got = rc.check(emu, nat.CRC, b"", [0, 0, 0], ctx=ctx, repaired=0)
    assert got == (0, 0, rc.NONE, 0, 0)


# ---- 2. a clean segment -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,empties", [(rc.CUT, ()), (rc.CUT, (0, 40)), (65536, ()), (65536, (2, 3)), (1 << 20, ())])
def test_a_clean_segment_passes_in_every_cut_and_keeps_its_bytes(emu, ctx, segment, size, empties):
    sizes = rc.cut(segment, size, empties)
    assert len(sizes) == -(-len(segment) // size) + len(empties)
    outs, got = rc.check(emu, nat.ENCRYPT | nat.CRC, segment, sizes, "host", ctx, repaired=0)
    assert got == (19, 0, rc.NONE, 0, 0) and emu.ctx_records(ctx).ms > 0


@pytest.mark.parametrize("mem", rc.MEMS)
def test_a_clean_segment_passes_on_every_memory_kind(emu, ctx, segment, mem):
    sizes = rc.cut(segment, rc.CUT, (7,))
    rc.check(emu, nat.ENCRYPT | nat.CRC, segment, sizes, mem, ctx, repaired=0)
    rc.check(emu, 0, segment, sizes, mem, None)                         # a pooled context, the plain copy


def test_a_clean_segment_passes_through_the_piece_pipeline_and_the_compressor(emu, ctx, segment):
    sizes = rc.cut(segment, rc.CUT)
    rc.check(emu, nat.ENCRYPT | nat.CRC, segment, sizes, "host", ctx, repaired=0, sub_bytes=40000)       # eight pieces
    rc.check(emu, nat.CRC, segment, sizes, "packed", ctx, repaired=0, sub_bytes=40000)
    small = segment[:rc.batches_of(segment)[3][0]]                       # (the emulated compressor is slow: three batches, 16 chunks, two members)
    sizes = rc.cut(small, -(-len(small) // 16))
    assert len(sizes) == 16
    want, got = rc.check(emu, CE | nat.CRC, small, sizes, "zero_copy", ctx, repaired=0)
    for mem, cfg in (("host", {}), ("packed", {}), ("device", {"stages_separate": 1})):
        rc.check(emu, CE | nat.CRC, small, sizes, mem, ctx, want=want, repaired=0, **cfg)
    rc.check(emu, CE | nat.CRC | nat.VERIFY | nat.VERIFY_GCM, small, sizes, "zero_copy", None, want=want)      # pooled, in front of both verifiers


# ---- 3. headers split over chunks ---------------------------------------------------------------------------------------------
def test_a_header_split_at_every_byte_and_a_batch_that_ends_on_a_chunk_end(emu, ctx):
    a, b = rc.make_batch(0, b"first" * 40), rc.make_batch(1, b"second" * 50, attributes=4)
    s = a + b
    want, d0 = rc.run(emu, nat.CRC, s, [len(s)], "device", ctx)
    for k in range(0, 61):                                               # k = 0: the first batch ends exactly on the chunk's end
        sizes = [len(a) + k, len(b) - k]
        outs, got = rc.check(emu, nat.CRC, s, sizes, "device", ctx)
        assert got[:4] == (2, 1, rc.NONE, 0) and b"".join(outs) == s, k
        bad = rc.flip(s, len(a) + 60)                                    # ... and the second batch's last header byte, behind the split
        outs, got = rc.check(emu, nat.CRC, bad, sizes, "device", ctx)
        assert got[:4] == (1, 0, len(a), rc.CRC), k
    outs, got = rc.check(emu, nat.CRC, s, [len(a), 0, 3, len(b) - 3], "device", ctx)         # a chunk that holds nothing but a piece of a header
    assert got[:4] == (2, 1, rc.NONE, 0)
    assert want[0] == s


# ---- 4. damage ----------------------------------------------------------------------------------------------------------------
def test_one_damaged_byte_hostile_lengths_and_bad_stream_ends(emu, ctx, segment):
    cases, (p, l, j) = rc.damage_cases(segment)
    assert j >= 2 and l >= 3 * rc.CUT and len(cases) == 22
    seen = set()
    for name, s, fails in cases:
        sizes = rc.cut(s, rc.CUT)
        ref = rc.reference_walk(s)
        assert (ref[3] != 0) == fails, (name, ref)
        outs, got = rc.check(emu, nat.CRC, s, sizes, "host", ctx)
        if fails and len(s) == len(segment):
            assert ref[2] == p and [int(x != 0) for x in rc.expected_statuses(sizes, ref[2])] == [0] * j + [1] * (len(sizes) - j), name
        seen.add(ref[3])
    assert seen == {0, rc.TRUNCATED, rc.LENGTH, rc.MAGIC, rc.CRC}
    by = {n: rc.reference_walk(s)[2:] for n, s, f in cases}
    assert by["len7FFFFFFF"] == (p, rc.TRUNCATED) and by["len80000000"] == (p, rc.LENGTH) and by["len48"] == (p, rc.LENGTH)
    assert by["cut1"][1] == rc.TRUNCATED and by["garbage60"] == (len(segment), rc.TRUNCATED) and by["zeros4096"] == (len(segment), rc.LENGTH)


def test_damage_is_found_on_the_other_paths_too(emu, ctx, segment):
    p, l, j = rc.long_batch(segment)
    bad = rc.flip(segment, p + 19)
    sizes = rc.cut(bad, rc.CUT)
    for flags, mem, cfg in ((nat.ENCRYPT, "zero_copy", {}), (0, "device", {}), (nat.CRC, "packed", {"sub_bytes": 40000}), (nat.ENCRYPT, "host", {"sub_bytes": 40000})):
        rc.check(emu, flags, bad, sizes, mem, ctx, **cfg)
    rc.check(emu, nat.CRC, bad, sizes, "host", None)                    # a pooled context
    small = segment[:rc.batches_of(segment)[3][0]]
    p = rc.batches_of(small)[1][0]
    bad = rc.flip(small, p + 19)
    sizes = rc.cut(bad, -(-len(bad) // 16))
    want = None
    for mem, cfg in (("zero_copy", {}), ("packed", {}), ("packed_zc", {}), ("host", {"stages_separate": 1})):
        outs, got = rc.check(emu, CE | nat.CRC, bad, sizes, mem, ctx, want=want, **cfg)
        want = want or rc.run(emu, CE | nat.CRC, bad, sizes, "zero_copy", ctx)[0]
        assert got[2] == p and outs[0] != b"" and outs[-1] == b""


def test_a_chunk_that_carries_another_error_keeps_it(emu, ctx, segment):
    import numpy as np
    p, l, j = rc.long_batch(segment)
    bad = rc.flip(segment, p + 17)
    sizes = rc.cut(bad, 65536)
    k = p // 65536
    assert k + 1 < len(sizes)
    soff, doff, caps, st, dt = pc.layout(sizes, nat.ENCRYPT, emu)
    src = np.zeros(st, np.uint8); at = 0
    for s_, o_ in zip(sizes, soff):
        src[o_:o_ + s_] = np.frombuffer(bad[at:at + s_], np.uint8); at += s_
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps); d["dst_cap"][k + 1] = 100; d["dst_cap"][0] = 100
    emu.transform_batch(nat.Native.make_params(nat.ENCRYPT | rc.VR, synth.KEY, synth.AAD), d, src, dst, dst.size, ctx=ctx)
    want = [nat.E_DST_TOO_SMALL if i in (0, k + 1) else rc.E_RECORDS if i >= k else 0 for i in range(len(sizes))]
    assert [int(x) for x in d["status"]] == want and (d["dst_len"][k:] == 0).all()


@pytest.mark.parametrize("mem,cfg", [("zero_copy", {}), ("host", {}), ("packed", {}), ("host", {"stages_separate": 1})])
def test_a_chunk_that_a_verifier_and_the_validator_fail_reports_the_verifier(emu, ctx, segment, mem, cfg):
    """All three checks on one compressing batch whose second record batch is damaged: the order in which their verdicts reach a chunk is
    what the caller sees as precedence - the Zstandard verifier, the GCM verifier, then the validator.  A chunk behind the bad record
    batch that a verifier fails as well is TSX_E_VERIFY, in front of it only the verifiers speak."""
    small = segment[:rc.batches_of(segment)[3][0]]
    bad = rc.flip(small, rc.batches_of(small)[1][0] + 19)
    sizes = rc.cut(bad, -(-len(bad) // 16))
    assert len(sizes) == 16 and sizes[0] == 3298
    k = rc.expected_statuses(sizes, rc.reference_walk(bad)[2]).index(rc.E_RECORDS)
    assert k == 3
    flags = CE | nat.CRC
    want, d0 = rc.run(emu, flags, bad, sizes, mem, ctx, **cfg)
    assert (d0["status"] == 0).all()
    V, R = gv.E_VERIFY, rc.E_RECORDS
    for src_hit, out_hit, exp in ((k - 1, k + 1, [0, 0, V, R, V] + [R] * 11), (k + 2, k - 1, [0, 0, V, R, R, V] + [R] * 10)):
        outs, d = rc.run(emu, flags | nat.VERIFY | nat.VERIFY_GCM | rc.VR, bad, sizes, mem, ctx, verify_damage_src_chunk=src_hit, verify_damage_src_off=100,
                         verify_damage_out_chunk=out_hit, verify_damage_out_off=20, **cfg)
        assert (V, R) == (-10, -11) and [int(x) for x in d["status"]] == exp, (mem, cfg, src_hit, out_hit, [int(x) for x in d["status"]])
        assert (d["dst_len"][2:] == 0).all() and outs[2:] == [b""] * 14, (mem, cfg, src_hit)
        assert outs[:2] == want[:2] and [int(x) for x in d["dst_len"][:2]] == [len(w) for w in want[:2]], (mem, cfg, src_hit)


# ---- 5. speculation has to lose and still be right ---------------------------------------------------------------------------
def test_a_valid_batch_inside_a_record_value_is_not_counted(emu, ctx):
    s = rc.nested_stream()
    assert rc.reference_walk(s) == (7, 2, rc.NONE, 0)                  # (the inner batch, attributes 1, is not one of them)
    outs, got = rc.check(emu, nat.CRC, s, rc.cut(s, rc.CUT), "host", ctx)
    assert got[:4] == (7, 2, rc.NONE, 0) and got[4] >= 1


def test_a_damaged_first_batch_of_a_chunk_is_reported_not_skipped(emu, ctx, segment):
    first = {}
    for p, l in rc.batches_of(segment):
        first.setdefault(p // rc.CUT, (p, l))
    j, (p, l) = sorted(first.items())[3]
    assert j > 0 and p % rc.CUT
    bad = rc.flip(segment, p + 20)
    outs, got = rc.check(emu, nat.CRC, bad, rc.cut(bad, rc.CUT), "host", ctx)
    assert got[2:4] == (p, rc.CRC) and got[4] >= 1


def test_a_batch_longer_than_many_chunks_and_three_thousand_empty_batches(emu, ctx):
    big = rc.make_batch(0, synth.gen_chunk("R", 5, 0, 0, 200000 - 61).tobytes()) + rc.make_batch(1, b"tail" * 30)
    sizes = rc.cut(big, rc.CUT)
    assert len(sizes) == 49
    outs, got = rc.check(emu, nat.CRC, big, sizes, "host", ctx)
    assert got[:4] == (2, 0, rc.NONE, 0)
    outs, got = rc.check(emu, nat.CRC, rc.flip(big, 150000), sizes, "host", ctx)
    assert got[:4] == (0, 0, 0, rc.CRC)
    empty = b"".join(rc.make_batch(i, b"", attributes=i % 3) for i in range(3000))
    assert len(empty) == 3000 * 61
    outs, got = rc.check(emu, nat.CRC, empty, rc.cut(empty, rc.CUT), "host", ctx, repaired=0)
    assert got[:4] == (3000, 2000, rc.NONE, 0)
    outs, got = rc.check(emu, nat.CRC, rc.flip(empty, 2000 * 61 + 22), rc.cut(empty, rc.CUT), "host", ctx)
    assert got[:4] == (2000, 1333, 2000 * 61, rc.CRC)


def test_no_memory_for_the_validator_is_said_per_chunk(emu, segment):
    import ctypes
    h = emu.ctx_create(0, 0, 0)
    try:
        s = segment[:rc.batches_of(segment)[2][0]]
        sizes = rc.cut(s, rc.CUT)
        want, d0 = rc.run(emu, nat.CRC, s, sizes, "host", h)         # (the context has its workspace: the validator's block is the one allocation left)
        emu.lib.hipemu_fail_alloc_at.argtypes = [ctypes.c_long]
        emu.lib.hipemu_fail_alloc_at(1)
        try:
            outs, d = rc.run(emu, nat.CRC | rc.VR, s, sizes, "host", h)
        finally:
            emu.lib.hipemu_fail_alloc_at(0)
        assert (d["status"] == nat.E_NOMEM).all() and (d["dst_len"] == 0).all()
        rc.check(emu, nat.CRC, s, sizes, "host", h, want=want, repaired=0)
    finally:
        emu.ctx_destroy(h)
