"""Record-batch validation of a segment streamed in several calls (tsx_transform_batch_stream) under the CPU emulator: the rules of the
entry point, one call against today's flag path, the call boundary at every byte of a header and around a batch's and the stream's end,
a segment in calls of 1, 3 and 16 chunks on a different context per call, damage, a batch open across five calls, speculation that has to
lose, and a compressing chain - all against tests/records_cases.py::reference_walk over the concatenated stream.  The same functions run
on the device in tests/test_zzzzzzzzzzzzzzzz_gpu_records_stream.py."""
import ctypes

import pytest

import tsxform
from tests import records_cases as rc
from tests import records_stream_cases as rs
from tsxform import synth

nat = tsxform._native
CE = nat.COMPRESS | nat.ENCRYPT
FLAGS = (0, nat.CRC, nat.ENCRYPT | nat.CRC)


@pytest.fixture()
def ctxs(emu):
    hs = [emu.ctx_create(0, 0, 0) for _ in range(3)]
    yield hs
    for h in hs:
        emu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    s = rc.valid_segment(300000)
    assert len(s) == 290455
    return s


def three_batches():
    s = rc.make_batch(0, b"a" * 139) + rc.make_batch(1, b"") + rc.make_batch(2, b"c" * 239, attributes=2)
    assert len(s) == 561 and rc.batches_of(s) == [(0, 200), (200, 61), (261, 300)]
    return s


# ---- 1. the rules -------------------------------------------------------------------------------------------------------------
def _rc_of(N, flags, data, sizes, state, ctx=None):
    try:
        rs.run_one(N, flags, data, sizes, "host", ctx, state)
    except nat.TsxError as e:
        return e.code
    return 0


def test_the_rules_of_the_entry_point_and_a_refused_call_leaves_the_state_as_it_was(emu, ctxs):
    N, s = emu, three_batches()
    assert ctypes.sizeof(nat.RecordsState) == 192
    never = nat.RecordsState()
    info = nat.RecordsInfo()
    assert N.lib.tsx_records_result(ctypes.byref(never), ctypes.byref(info)) == nat.E_INVAL
    assert _rc_of(N, nat.CRC | rc.VR, s[:100], [100], never) == nat.E_INVAL and bytes(never) == bytes(192)
    assert N.lib.tsx_records_begin(None, 5) == nat.E_INVAL
    st = N.records_begin(len(s))
    assert rs.result(N, st) == (False, (0, 0, rc.NONE, 0))
    for ctx in (None, ctxs[0]):
        before = bytes(st)
        assert _rc_of(N, nat.CRC, s[:100], [100], st, ctx) == nat.E_INVAL and bytes(st) == before            # without the flag
        assert _rc_of(N, nat.VERIFY_GCM | rc.VR, s[:100], [100], st, ctx) == nat.E_INVAL and bytes(st) == before   # what fails without a state
        assert _rc_of(N, nat.CRC | rc.VR, s + b"\0", [len(s) + 1], st, ctx) == nat.E_INVAL and bytes(st) == before   # more than was declared
        # a call without chunks, and one with empty chunks only, change nothing
        assert _rc_of(N, nat.CRC | rc.VR, b"", [], st, ctx) == 0 and bytes(st) == before
        outs, d = rs.run_one(N, nat.ENCRYPT | rc.VR, b"", [0, 0], "host", ctx, st)
        assert bytes(st) == before and list(d["status"]) == [0, 0] and list(d["dst_len"]) == [28, 28]
    outs, d = rs.run_one(N, nat.CRC | rc.VR, s[:230], [230], "host", None, st)       # 30 bytes of the second header are carried
    assert list(d["status"]) == [0] and rs.result(N, st) == (False, (1, 0, rc.NONE, 0))
    before = bytes(st)
    assert _rc_of(N, nat.CRC | rc.VR, s[230:] + b"\0", [len(s) - 230 + 1], st) == nat.E_INVAL and bytes(st) == before
    # every number of the state is checked: the carried-header count, the bytes consumed, the open batch's end
    words = list(st.opaque)
    assert 30 in [w >> 32 for w in words] + [w & 0xFFFFFFFF for w in words]
    for k, w in enumerate(words):
        for half in (0, 32):
            if (w >> half) & 0xFFFFFFFF == 30:
                bad = nat.RecordsState(); ctypes.memmove(ctypes.byref(bad), ctypes.byref(st), 192)
                bad.opaque[k] = (w & ~(0xFFFFFFFF << half)) | (61 << half)
                kept = bytes(bad)
                assert _rc_of(N, nat.CRC | rc.VR, s[230:], [len(s) - 230], bad) == nat.E_INVAL and bytes(bad) == kept
                assert N.lib.tsx_records_result(ctypes.byref(bad), ctypes.byref(info)) == nat.E_INVAL
    for k, w in enumerate(words):
        if w == 230:                                                     # consumed beyond the declared length
            bad = nat.RecordsState(); ctypes.memmove(ctypes.byref(bad), ctypes.byref(st), 192)
            bad.opaque[k] = len(s) + 1
            assert _rc_of(N, nat.CRC | rc.VR, b"", [], bad) == nat.E_INVAL
    copy = nat.RecordsState(); ctypes.memmove(ctypes.byref(copy), ctypes.byref(st), 192)     # the state may be copied
    for state in (st, copy):
        outs, d = rs.run_one(N, nat.CRC | rc.VR, s[230:], [len(s) - 230], "host", ctxs[1], state)
        assert list(d["status"]) == [0] and rs.result(N, state) == (True, (3, 1, rc.NONE, 0))
    assert _rc_of(N, nat.CRC | rc.VR, b"\0", [1], st) == nat.E_INVAL
    # an open batch's end is checked too
    st = N.records_begin(len(s))
    rs.run_one(N, rc.VR, s[:400], [400], "host", None, st)               # batch 3 [261, 561) is open
    words = list(st.opaque)
    assert words.count(561) == 2                                         # the declared length, and behind it the open batch's end
    bad = nat.RecordsState(); ctypes.memmove(ctypes.byref(bad), ctypes.byref(st), 192)
    bad.opaque[len(words) - 1 - words[::-1].index(561)] = 562
    assert _rc_of(N, rc.VR, s[400:], [161], bad) == nat.E_INVAL
    assert _rc_of(N, rc.VR, s[400:], [161], st) == 0 and rs.result(N, st) == (True, (3, 1, rc.NONE, 0))
    st = N.records_begin(0)
    assert rs.result(N, st) == (True, (0, 0, rc.NONE, 0))


# ---- 2. one call equals today's flag path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", rc.MEMS)
def test_one_call_with_the_declared_length_of_its_bytes_equals_the_flag_path(emu, ctxs, segment, mem):
    sizes = rc.cut(segment, rc.CUT)
    for ctx in (None, ctxs[0]):
        for flags in (nat.ENCRYPT | nat.CRC,) if ctx is None else (0, nat.ENCRYPT | nat.CRC):
            want, info = rc.check(emu, flags, segment, sizes, mem, ctx)
            runs, st = rs.check_calls(emu, flags, segment, [sizes], mem, [ctx] if ctx else None, want=[want])
            assert rs.result(emu, st) == (True, (19, 0, rc.NONE, 0))
            if ctx:
                assert rc.info(emu, ctx) == info and emu.records_result(st)[1].repaired_chunks == info[4] and emu.records_result(st)[1].ms > 0
    bad = rc.flip(segment, rc.long_batch(segment)[0] + 18)               # ... and a damaged one
    want, info = rc.check(emu, nat.CRC, bad, sizes, mem, ctxs[0])
    runs, st = rs.check_calls(emu, nat.CRC, bad, [sizes], mem, ctxs[:1], want=[want])
    assert rc.info(emu, ctxs[0])[:4] == info[:4] == rs.result(emu, st)[1]


# ---- 3. the boundary at every byte ------------------------------------------------------------------------------------------
def _variants(s):
    """(name, stream): clean, and a bit flipped in batch 1's length field, magic byte, CRC field and last byte."""
    return [("clean", s), ("length", rc.flip(s, 200 + 11)), ("magic", rc.flip(s, 200 + 16)), ("crc", rc.flip(s, 200 + 19)), ("last", rc.flip(s, 260))]


def boundary_cases():
    """[(name, stream, calls)]: two calls with the cut from 2 bytes in front of batch 1 to 63 bytes into it and +-2 around its end and the
    stream's end, chunks of 1, 7 and 64 bytes; three calls whose middle one holds 1 .. 61 bytes; an empty call and a call of empty chunks."""
    s = three_batches()
    out = []
    cuts = sorted(set(range(198, 264)) | set(range(259, 264)) | set(range(559, 562)))
    for name, v in _variants(s):
        for q in cuts:
            for size in (1, 7, 64):
                out.append(("%s cut %d by %d" % (name, q, size), v, [rs.chunks_of(q, size), rs.chunks_of(len(v) - q, size)]))
        for mid in (1, 20, 59, 60, 61):
            for size in (1, 7, 64):
                a = 200 + 3
                out.append(("%s middle %d by %d" % (name, mid, size), v, [rs.chunks_of(a, size), rs.chunks_of(mid, size), rs.chunks_of(len(v) - a - mid, size)]))
        out.append((name + " empty calls", v, [rs.chunks_of(230, 64), [], [0, 0, 0], rs.chunks_of(len(v) - 230, 7) + [0]]))
    return out


VARIANTS = ("clean", "length", "magic", "crc", "last")


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_call_boundary_at_every_byte_of_a_header_and_around_the_ends(emu, ctxs, variant):
    cases = boundary_cases()
    assert len(cases) == 5 * (69 * 3 + 15 + 1) and [n for n, _ in _variants(three_batches())] == list(VARIANTS)
    cases = [c for c in cases if c[0].startswith(variant + " ")]
    assert len(cases) == 69 * 3 + 15 + 1
    for k, (name, s, calls) in enumerate(cases):
        flags = FLAGS[(k + k // 3) % 3]                                  # (every chunk size meets every chain)
        try:
            rs.check_calls(emu, flags, s, calls, "device" if k % 2 else "host", ctxs if k % 5 else None, want=None if flags & nat.ENCRYPT else "source")
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_what_the_boundary_variants_are_in_the_references_words():
    # what the variants are, in the reference's words (batch 1's batchLength is 49: the flipped bit makes it 48)
    v = dict(_variants(three_batches()))
    assert rs.reference(v["length"])[2:] == (200, rc.LENGTH, 260) and rs.reference(v["magic"])[2:] == (200, rc.MAGIC, 260)
    assert rs.reference(v["crc"])[2:] == (200, rc.CRC, 260) and rs.reference(v["last"])[2:] == (200, rc.CRC, 260)


def test_a_length_beyond_the_declared_end_and_a_stream_that_ends_inside_a_header(emu, ctxs):
    s = three_batches()
    b = bytearray(s); b[200 + 8:200 + 12] = (0x7FFFFFFF).to_bytes(4, "big")
    b = bytes(b)
    assert rs.reference(b)[2:] == (200, rc.TRUNCATED, 260)
    tail = s + b"\x5A" * 60                                              # fewer than 61 bytes left: the verdict needs byte 561 only
    assert rs.reference(tail)[2:] == (561, rc.TRUNCATED, 561)
    for q in (199, 200, 201, 230, 260, 261, 262):
        for size in (1, 64):
            rs.check_calls(emu, nat.CRC, b, [rs.chunks_of(q, size), rs.chunks_of(len(b) - q, size)], "host", ctxs, want="source")
    for q in (560, 561, 562, 600):
        rs.check_calls(emu, nat.CRC, tail, [rs.chunks_of(q, 64), rs.chunks_of(len(tail) - q, 7)], "host", ctxs, want="source")


# ---- 4. the segment in calls of 1, 3 and 16 chunks ---------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 3, 16])
def test_the_segment_in_calls_of_a_few_chunks_on_a_different_context_per_call(emu, ctxs, segment, per):
    sizes = rc.cut(segment, rc.CUT, (0, 5, 40))
    calls = rs.split(sizes, per)
    flags = FLAGS[(per + 1) % 3] if per != 16 else nat.ENCRYPT | nat.CRC
    runs, st = rs.check_calls(emu, flags, segment, calls, "host", ctxs)
    assert rs.result(emu, st) == (True, (19, 0, rc.NONE, 0))
    rs.check_calls(emu, flags, segment, calls, "zero_copy" if flags & nat.ENCRYPT else "packed", None)     # pooled contexts


# ---- 5. damage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 5])
def test_damage_in_calls_of_a_few_chunks_and_every_later_call_is_refused_per_chunk(emu, ctxs, segment, per):
    cases, (p, l, j) = rc.damage_cases(segment)
    seen = set()
    for k, (name, s, fails) in enumerate(cases):
        calls = rs.split(rc.cut(s, rc.CUT), per)
        ref = rs.reference(s)
        assert (ref[3] != 0) == fails, (name, ref)
        seen.add(ref[3])
        exp = rs.expected_statuses(calls, ref)
        try:
            runs, st = rs.check_calls(emu, FLAGS[k % 3], s, calls, "host", ctxs, want=None if FLAGS[k % 3] & nat.ENCRYPT else "source")
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        if fails:
            hit = [k_ for k_, e in enumerate(exp) if rc.E_RECORDS in e]
            assert hit and all(e == [rc.E_RECORDS] * len(e) for e in exp[hit[0] + 1:]), name
            for (outs, d), e in list(zip(runs, exp))[hit[0] + 1:]:
                assert (d["status"] == rc.E_RECORDS).all() and (d["dst_len"] == 0).all(), name
    assert seen == {0, rc.TRUNCATED, rc.LENGTH, rc.MAGIC, rc.CRC}


# ---- 6. a batch open across calls ------------------------------------------------------------------------------------------------
def test_a_batch_of_ten_chunks_open_across_five_calls(emu, ctxs):
    big = rc.make_batch(0, b"head" * 25) + rc.make_batch(1, synth.gen_chunk("R", 5, 0, 0, 10 * rc.CUT - 61).tobytes(), attributes=3) + rc.make_batch(2, b"tail" * 30)
    assert rc.batches_of(big)[1] == (161, 10 * rc.CUT)
    sizes = rc.cut(big, rc.CUT)
    calls = rs.split(sizes, 2)
    assert len(calls) == 6 and sum(sum(c) for c in calls[:5]) < 161 + 10 * rc.CUT <= len(big)
    runs, st = rs.check_calls(emu, nat.CRC, big, calls, "host", ctxs, want="source")
    assert rs.result(emu, st) == (True, (3, 1, rc.NONE, 0))
    bad = rc.flip(big, 161 + 10 * rc.CUT - 1)                            # its last byte: the verdict falls where that byte is, the position lies in call 0
    ref = rs.reference(bad)
    assert ref == (1, 0, 161, rc.CRC, 161 + 10 * rc.CUT - 1)
    exp = rs.expected_statuses(calls, ref)
    assert exp[:5] == [[0, 0]] * 5 and exp[5] == [rc.E_RECORDS] * len(calls[5])
    rs.check_calls(emu, nat.CRC, bad, calls, "host", ctxs, want="source")
    rs.check_calls(emu, nat.ENCRYPT, bad, rs.split(sizes, 1), "zero_copy", None)


# ---- 7. speculation has to lose ----------------------------------------------------------------------------------------------------
def test_a_valid_batch_inside_a_record_value_on_the_first_byte_of_a_call_is_not_counted(emu, ctxs):
    s = rc.nested_stream()
    sizes = rc.cut(s, rc.CUT)
    assert rc.reference_walk(s) == (7, 2, rc.NONE, 0)
    runs, st = rs.check_calls(emu, nat.CRC, s, [sizes[:1], sizes[1:]], "host", ctxs, want="source")
    assert rs.result(emu, st) == (True, (7, 2, rc.NONE, 0))
    rs.check_calls(emu, nat.CRC, s, rs.split(sizes, 1), "device", ctxs, want="source")


# ---- 8. a compressing chain ------------------------------------------------------------------------------------------------------
def test_a_compressing_chain_with_both_verifiers_in_two_calls(emu, ctxs, segment):
    small = segment[:rc.batches_of(segment)[3][0]]
    sizes = rc.cut(small, -(-len(small) // 16))
    assert len(sizes) == 16
    rs.check_calls(emu, CE | nat.VERIFY | nat.VERIFY_GCM, small, [sizes[:8], sizes[8:]], "zero_copy", ctxs)
