"""Record-batch validation of a stream given in SEVERAL calls (tsx_transform_batch_stream): helpers shared by the emulated and the device
tests.  `N` is a tsxform._native.Native (emulated or real).  The yardstick is tests/records_cases.py::reference_walk over the concatenated
stream: whatever the cut into calls and chunks, the result after the last call is the one call's."""
import numpy as np

import tsxform
from tests import parity_cases as pc
from tests import records_cases as rc
from tsxform import synth

nat = tsxform._native
VR, E_RECORDS, NONE = rc.VR, rc.E_RECORDS, rc.NONE


def reference(stream):
    """reference_walk(stream) + (d,): d is the last byte the verdict needs - bad_pos for "fewer than 61 bytes left", bad_pos + 60 for
    length, beyond-the-stream and magic, the batch's last byte for CRC; None for a clean stream."""
    stream = bytes(stream)
    nb, nc, bad, why = rc.reference_walk(stream)
    if not why:
        d = None
    elif why == rc.TRUNCATED and len(stream) - bad < 61:
        d = bad
    elif why == rc.CRC:
        d = bad + 12 + int.from_bytes(stream[bad + 8:bad + 12], "big") - 1
    else:
        d = bad + 60
    return nb, nc, bad, why, d


def expected_statuses(calls, ref):
    """Per call, per chunk: the verdict falls in the call that holds byte d; there, TSX_E_RECORDS from the chunk on that holds stream position
    max(bad_pos, the call's first position); 0 in every call in front of it, TSX_E_RECORDS everywhere in every call behind it."""
    bad, d = ref[2], ref[4]
    out, base = [], 0
    for sizes in calls:
        n = sum(sizes)
        if d is None or d >= base + n:
            out.append([0] * len(sizes))
        elif d < base:
            out.append([E_RECORDS] * len(sizes))
        else:
            want, at, j = max(bad, base), base, None
            for i, s in enumerate(sizes):
                if s and at <= want < at + s:
                    j = i
                at += s
            assert j is not None, (calls, ref)
            out.append([0 if i < j else E_RECORDS for i in range(len(sizes))])
        base += n
    return out


def run_one(N, flags, data, sizes, mem="host", ctx=None, state=None, level=3, **cfg):
    """records_cases.run with a stream state: one transform batch whose chunks are `data` cut into `sizes`.  -> (outputs by dst_len, descs)."""
    data = np.frombuffer(bytes(data), np.uint8)
    assert sum(sizes) == data.size
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N)
    src = np.full(max(st, 16), 0xA5, np.uint8)
    src[5::7] = 2
    at = 0
    for s, o_ in zip(sizes, soff):
        src[o_:o_ + s] = data[at:at + s]; at += s
    slot = (N.transformed_bound(max(list(sizes) + [0]), flags) + 63) // 64 * 64
    dst = np.full(max(dt, len(sizes) * slot, 16) + 64, 0xEE, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level)
    registered = mem in ("zero_copy", "packed_zc")
    if mem == "packed_zc":
        cfg = dict(cfg, zero_copy_packed=1)
    with N.configured(**cfg):
        if mem == "device":
            ds, dd = N.device_malloc(src.size), N.device_malloc(dst.size)
            try:
                N.h2d(ds, src); N.h2d(dd, dst)
                N.transform_batch(p, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx, src_size=src.size, state=state)
                N.d2h(dst, dd)
            finally:
                N.device_free(ds); N.device_free(dd)
        else:
            if registered:
                N.host_register(dst)
            try:
                N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED if mem.startswith("packed") else nat.MEM_HOST, ctx=ctx, state=state)
            finally:
                if registered:
                    N.host_unregister(dst)
    return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))], d


def run_calls(N, flags, stream, calls, mem="host", ctxs=None, declared=None, **cfg):
    """`stream` in len(calls) calls on ONE state; calls: a list of chunk-size lists; ctxs: the context of call k is ctxs[k % len(ctxs)]
    (None: the pool); declared: the length the stream is begun with (default: its own).  flags without VALIDATE_RECORDS: the same calls
    without a state.  -> ([(outputs, descs)] per call, state)."""
    stream = bytes(stream)
    assert sum(sum(c) for c in calls) == len(stream)
    state = N.records_begin(len(stream) if declared is None else declared) if flags & VR else None
    out, at = [], 0
    for k, sizes in enumerate(calls):
        n = sum(sizes)
        ctx = ctxs[k % len(ctxs)] if ctxs else None
        out.append(run_one(N, flags, stream[at:at + n], list(sizes), mem, ctx, state, **cfg))
        at += n
    return out, state


def result(N, state):
    done, r = N.records_result(state)
    return done, (int(r.batches), int(r.compressed_batches), int(r.first_bad_pos), int(r.first_bad_reason))


def check_calls(N, flags, stream, calls, mem="host", ctxs=None, want=None, **cfg):
    """The calls with the flag on one state: every call's statuses and dst_len by the rule, the result after the last call reference_walk's;
    the bytes of a delivered chunk are `want`'s (per call, per chunk; "source": the chunk's own bytes - a chain that copies; None: those of
    the same calls without the flag).  -> (runs, state)."""
    ref = reference(stream)
    exp = expected_statuses(calls, ref)
    if want is None:
        plain, _ = run_calls(N, flags, stream, calls, mem, ctxs, **cfg)
        assert all((d["status"] == 0).all() for _, d in plain)
        want = [o for o, _ in plain]
    runs, state = run_calls(N, flags | VR, stream, calls, mem, ctxs, **cfg)
    at = 0
    for k, ((outs, d), e) in enumerate(zip(runs, exp)):
        assert [int(x) for x in d["status"]] == e, (mem, cfg, k, calls[k], ref, [int(x) for x in d["status"]])
        for i, s in enumerate(calls[k]):
            if e[i]:
                assert outs[i] == b"" and d["dst_len"][i] == 0, (k, i)
            elif want == "source":
                assert outs[i] == bytes(stream[at:at + s]), (k, i)
            else:
                assert outs[i] == want[k][i] and int(d["dst_len"][i]) == len(want[k][i]), (k, i)
            at += s
    done, got = result(N, state)
    assert done and got == ref[:4], (mem, cfg, calls, got, ref)
    return runs, state


def split(sizes, per):
    """A chunk-size list in calls of `per` chunks."""
    return [sizes[a:a + per] for a in range(0, len(sizes), per)] or [[]]


def chunks_of(n, size):
    """n bytes in chunks of `size` (none for n == 0)."""
    return [min(size, n - a) for a in range(0, n, size)]
