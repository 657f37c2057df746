"""Per-batch keys, AADs and IVs: bodies shared by the emulated (tests/test_emu_keying.py) and the device tests
(tests/test_zzzzzzzzz_gpu_keying.py).  Every segment a broker uploads has a data key and a 32-byte AAD of its own and every chunk an IV
of its own; the rest of the suite runs under synth.KEY / synth.AAD and segment 0, where a stale or cross-member read of the key
schedule, the AAD or an IV gives the right bytes.  Here every batch draws (key, AAD, segment) from a seeded generator and every
expectation comes from OpenSSL (and libzstd 1.5.7) through the oracle - never from the library under test.
`N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import ctypes as C
import threading

import numpy as np
import pytest

import tsxform
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
SEED = 20261018
AAD_LENGTHS = [0, 1, 15, 16, 17, 20, 31, 32, 33, 48, 63, 64]
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
# first / last partial block, one block, the 64 KiB sub-block edges of gcm_ctr_ghash_kernel, two sub-blocks and a byte
BATCH_SIZES = [0, 1, 15, 16, 17, 4097, 65535, 65536, 65537, 131073]
SETUP_SIZES = [0, 17, 65537]
# an incompressible chunk of s bytes becomes a frame of s + 10: 995 .. 1030 walks the frame over 63, 64 and 65 AES blocks and every
# residue mod 16 - where gcm_encrypt_wave's lane ownership (j = lane + 64 k) and its any / last logic change
FUSED_R_SIZES = list(range(995, 1031)) + [0, 1]
FUSED_R_EDGES = [995, 998, 999, 1013, 1014, 1015, 1030, 0, 1]           # frames of 63, 64 and 65 blocks, whole and partial last block
FUSED_K_SIZE = 70001
SEPARATE_SIZES = [0, 1, 1000, 1013]
TAMPER_SIZES = [1, 17, 65537, 131073]


def need157(o):
    if not o.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")


def draw(rng, aad_len=32):
    """A fresh (key, AAD, segment number)."""
    return rng.bytes(32), rng.bytes(aad_len), int(rng.integers(1, 1 << 32))


def sweep_params(aad_len):
    """The (key, AAD, segment) of the sweep at this AAD length, and the generator its data comes from."""
    rng = np.random.default_rng([SEED, 1, aad_len])
    return draw(rng, aad_len), rng


def rand_chunks(rng, sizes):
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]


_K = {}


def k_chunks(size, n=16):
    """n Kafka-like chunks of `size` bytes (generated once: ~0.3 s per MiB)."""
    if (size, n) not in _K:
        _K[(size, n)] = [synth.gen_chunk("K", SEED % 1000, 7, i, size) for i in range(n)]
    return _K[(size, n)]


def rotated(xs, k):
    k %= len(xs)
    return xs[k:] + xs[:k]


def run_transform_keyed(N, flags, chunks, key, aad, segment, **kw):
    """parity_cases.run_transform under this key and AAD, with the IVs of this segment."""
    return pc.run_transform(N, flags, chunks, key=key, aad=aad, segment=segment, **kw)


def run_detransform_keyed(N, flags, blobs, out_sizes, key, aad, segment, **kw):
    return pc.run_detransform(N, flags, blobs, out_sizes, key=key, aad=aad, segment=segment, **kw)


def expected_blob(o, flags, key, aad, segment, i, chunk):
    """IV || C || TAG of chunk i as OpenSSL writes it (over libzstd's frame with compression)."""
    body = chunk.tobytes()
    if flags & nat.COMPRESS:
        body = o.zstd_compress_chunk(body)
    return o.gcm_encrypt_chunk(key, synth.iv_for(segment, i), aad, body, openssl=True)


def expected_blobs(o, flags, key, aad, segment, chunks, frames=None):
    """frames: libzstd's frames of the chunks where the caller already has them (the same chunks under many keys)."""
    if frames is not None and flags & nat.COMPRESS:
        return [o.gcm_encrypt_chunk(key, synth.iv_for(segment, i), aad, f, openssl=True) for i, f in enumerate(frames)]
    return [expected_blob(o, flags, key, aad, segment, i, c) for i, c in enumerate(chunks)]


def check_keyed(N, o, flags, chunks, key, aad, segment, what="", expected=None, **kw):
    """One batch there and back: status 0, OpenSSL's bytes, the oracle's CRC32C, and detransform under the same key and AAD restores
    every chunk."""
    outs, d = run_transform_keyed(N, flags, chunks, key, aad, segment, **kw)
    exp = expected if expected is not None else expected_blobs(o, flags, key, aad, segment, chunks)
    for i, c in enumerate(chunks):
        tag = (what, len(aad), i, int(c.size))
        assert d["status"][i] == 0, tag + (int(d["status"][i]),)
        assert outs[i] == exp[i], "%s, AAD of %d bytes, chunk %d (n=%d): bytes differ from OpenSSL's" % tag
        if flags & nat.CRC:
            assert d["crc32c"][i] == o.crc32c(c.tobytes()), tag
    back, d2 = run_detransform_keyed(N, flags, outs, [int(c.size) for c in chunks], key, aad, segment, ctx=kw.get("ctx"))
    for i, c in enumerate(chunks):
        assert d2["status"][i] == 0 and back[i] == c.tobytes(), "%s, AAD of %d bytes, chunk %d (n=%d): not restored" % (what, len(aad), i, int(c.size))
    return outs


# ---- body 1: parameter sweep ------------------------------------------------------------------------------------------------
def sweep_batch_kernels(N, o, aad_len, sizes=BATCH_SIZES):
    """gcm_ctr_ghash_kernel + gcm_final_kernel, with and without the CRC stage in front."""
    (key, aad, seg), rng = sweep_params(aad_len)
    chunks = rand_chunks(rng, sizes)
    exp = expected_blobs(o, nat.ENCRYPT, key, aad, seg, chunks)
    for flags in (nat.ENCRYPT, nat.ENCRYPT | nat.CRC):
        check_keyed(N, o, flags, chunks, key, aad, seg, "batch kernels, flags %d" % flags, expected=exp)


def sweep_setup_kernel(N, o, aad_len, sizes=SETUP_SIZES):
    """The key schedule by gcm_setup_kernel instead of the host: the same bytes (transform and detransform both run under the hook)."""
    (key, aad, seg), rng = sweep_params(aad_len)
    chunks = rand_chunks(rng, sizes)
    with N.configured(gcm_setup_kernel=1):
        check_keyed(N, o, nat.ENCRYPT, chunks, key, aad, seg, "setup kernel")


def sweep_fused(N, o, aad_len, r_sizes=FUSED_R_SIZES, k_size=FUSED_K_SIZE):
    """gcm_encrypt_wave: the compressor wave encrypts the frame it has just written."""
    need157(o)
    (key, aad, seg), rng = sweep_params(aad_len)
    chunks = rand_chunks(rng, r_sizes) + [k_chunks(k_size, 1)[0]]
    check_keyed(N, o, FULL, chunks, key, aad, seg, "fused compressor wave")


def sweep_separate(N, o, aad_len, sizes=SEPARATE_SIZES):
    """One launch per stage: the frames wait in the staging buffer and the batch kernels encrypt them."""
    need157(o)
    (key, aad, seg), rng = sweep_params(aad_len)
    chunks = rand_chunks(rng, sizes)
    with N.configured(stages_separate=1):
        check_keyed(N, o, nat.COMPRESS | nat.ENCRYPT, chunks, key, aad, seg, "separate launches")


def check_aad_len_65_is_refused(N):
    """aad_len is 0 .. 64; 65 fails the call with TSX_E_INVAL in both directions and no descriptor is touched.  (make_params refuses 65
    before the library sees it: the field is set afterwards.)"""
    key, aad, seg = draw(np.random.default_rng([SEED, 2]), 64)
    src = np.zeros(4096, np.uint8); dst = np.zeros(8192, np.uint8)
    for flags in (nat.ENCRYPT, FULL):
        p = nat.Native.make_params(flags, key, aad)
        p.aad_len = 65
        for call in (N.transform_batch, N.detransform_batch):
            d = pc.make_descs([100, 200], [0, 128], [0, 1024], [512, 512], segment=seg); d["status"] = -7; d["dst_len"] = 5
            with pytest.raises(nat.TsxError) as e:
                call(p, d, src, dst, dst.size)
            assert e.value.code == nat.E_INVAL
            assert list(d["status"]) == [-7, -7] and list(d["dst_len"]) == [5, 5]
        p.aad_len = 64
        d = pc.make_descs([100, 200], [0, 128], [0, 1024], [512, 512], segment=seg)
        N.transform_batch(p, d, src, dst, dst.size)
        assert list(d["status"]) == [0, 0]


# ---- body 2: consecutive batches on one context, changing keys -----------------------------------------------------------------
def consecutive_plan(o, chunk_size, nchunks=16, batches=8, tag=3):
    """(flags, chunks, key, aad, segment, expected blobs) per batch: the full chain and encrypt-only batches alternate, each batch has
    the Kafka-like chunks in an order of its own."""
    rng = np.random.default_rng([SEED, tag, chunk_size])
    base = k_chunks(chunk_size, nchunks)
    frames = [o.zstd_compress_chunk(c.tobytes()) for c in base]
    plan = []
    for b in range(batches):
        key, aad, seg = draw(rng)
        flags = nat.ENCRYPT | nat.CRC if b % 2 else FULL
        k = int(rng.integers(0, nchunks))
        chunks = rotated(base, k)
        plan.append((flags, chunks, key, aad, seg, expected_blobs(o, flags, key, aad, seg, chunks, rotated(frames, k))))
    return plan


def check_consecutive_batches(N, o, chunk_size, explicit, nchunks=16):
    """Eight batches back to back on ONE context (an explicit one, then whatever the pool hands out), each under a fresh key, AAD and
    segment, each followed by its detransform: OpenSSL's bytes under THAT batch's key every time, and no key material left behind."""
    need157(o)
    plan = consecutive_plan(o, chunk_size, nchunks)
    ctx = N.ctx_create(0, 0, 0) if explicit else None
    try:
        for b, (flags, chunks, key, aad, seg, exp) in enumerate(plan):
            check_keyed(N, o, flags, chunks, key, aad, seg, "batch %d" % b, expected=exp, ctx=ctx)
        if explicit:
            res = N.lib.tsx_debug_key_residue; res.restype = C.c_int; res.argtypes = [C.c_void_p]
            assert res(ctx) == 0
    finally:
        if explicit:
            N.ctx_destroy(ctx)
    return plan


# ---- body 3: concurrent members of the compressor service under different keys -----------------------------------------------
def check_concurrent_members(N, o, threads, batches, chunk_size, nchunks=16):
    """`threads` context-less callers with registered host buffers, `batches` full-chain batches of `nchunks` chunks each, every (thread, batch)
    under a key, AAD and segment of its own (odd batches packed).  Each thread compares its output with libzstd + OpenSSL under that
    batch's key (computed before the threads start), restores it straight away, and hands one chunk of its neighbour's latest output
    (the neighbour's expected blob until it has published one) to detransform under its OWN key: OpenSSL says BadTag, so must the
    library.  -> number of compressing batches."""
    need157(o)
    rng = np.random.default_rng([SEED, 4, chunk_size])
    base = k_chunks(chunk_size, nchunks)
    frames = [o.zstd_compress_chunk(c.tobytes()) for c in base]
    sizes = [chunk_size] * nchunks
    soff, doff, caps, st, dt = pc.layout(sizes, FULL, N)
    sets = []
    for t in range(threads):
        chunks = rotated(base, t)
        per = []
        for b in range(batches):
            key, aad, seg = draw(rng)
            per.append((key, aad, seg, expected_blobs(o, FULL, key, aad, seg, chunks, rotated(frames, t))))
        sets.append((chunks, per))
    srcs, dsts = [], []
    for t in range(threads):
        src = np.zeros(st, np.uint8)
        for c, o_ in zip(sets[t][0], soff):
            src[o_:o_ + c.size] = c
        dst = np.zeros(dt, np.uint8)
        N.host_register(src); N.host_register(dst)
        srcs.append(src); dsts.append(dst)
    published = {}                                                      # thread -> first blob of its latest batch
    errors = []

    def worker(t):
        chunks, per = sets[t]
        nb = (t + 1) % threads
        try:
            for b, (key, aad, seg, exp) in enumerate(per):
                p = nat.Native.make_params(FULL, key, aad)
                d = pc.make_descs(sizes, soff, doff, caps, segment=seg)
                N.transform_batch(p, d, srcs[t], dsts[t], dsts[t].size, nat.MEM_HOST_PACKED if b % 2 else nat.MEM_HOST)
                got = [dsts[t][int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(nchunks)]
                if (d["status"] != 0).any():
                    errors.append((t, b, "status", [int(x) for x in d["status"]]))
                bad = [i for i in range(nchunks) if got[i] != exp[i]]
                if bad:
                    errors.append((t, b, "bytes differ from OpenSSL's under this batch's key", bad))
                if any(int(d["crc32c"][i]) != o.crc32c(chunks[i].tobytes()) for i in range(nchunks)):
                    errors.append((t, b, "crc"))
                published[t] = got[0]
                back, d2 = run_detransform_keyed(N, FULL, got, sizes, key, aad, seg)
                if (d2["status"] != 0).any() or back != [c.tobytes() for c in chunks]:
                    errors.append((t, b, "detransform", [int(x) for x in d2["status"]]))
                other = published.get(nb, sets[nb][1][0][3][0])
                try:
                    o.gcm_decrypt_chunk(key, aad, other, openssl=True)
                    errors.append((t, b, "OpenSSL accepts the neighbour's chunk under this key"))
                except o.BadTag:
                    pass
                back, d3 = run_detransform_keyed(N, FULL, [other], [chunk_size], key, aad, seg)
                if d3["status"][0] != nat.E_TAG_MISMATCH or d3["dst_len"][0] != 0:
                    errors.append((t, b, "neighbour's chunk under this key", int(d3["status"][0]), int(d3["dst_len"][0])))
        except Exception as e:                                          # noqa: BLE001 - reported through the list
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    try:
        [x.start() for x in th]
        [x.join() for x in th]
    finally:
        for a in srcs + dsts:
            N.host_unregister(a)
    assert not errors, errors[:6]
    return threads * batches


# ---- body 4: tamper matrix ---------------------------------------------------------------------------------------------------
def flip_bit(blob, at, bit=0):
    x = bytearray(blob); x[at] ^= 1 << bit
    return bytes(x)


def encrypt_only_variants(n, blob):
    """(label, damaged IV || C || TAG, capacity of its slot) for a chunk of n bytes."""
    assert len(blob) == n + 28
    v = [("iv byte 0", flip_bit(blob, 0), n), ("iv byte 11", flip_bit(blob, 11, 7), n),
         ("first ciphertext byte", flip_bit(blob, 12, 3), n), ("last ciphertext byte", flip_bit(blob, 12 + n - 1, 5), n)]
    for at in (65535, 65536):                                           # the last byte of a 64 KiB sub-block and the first of the next
        if at < n:
            v.append(("ciphertext byte %d" % at, flip_bit(blob, 12 + at, at & 7), n))
    for i in range(16):
        v.append(("tag byte %d" % i, flip_bit(blob, 12 + n + i, i % 8), n))
    v.append(("cut by one byte", blob[:-1], n - 1))
    v.append(("one byte appended", blob + b"\x5a", n + 1))
    return v


def oracle_status(o, key, aad, blob):
    try:
        o.gcm_decrypt_chunk(key, aad, blob, openssl=True)
        return 0
    except o.BadTag:
        return nat.E_TAG_MISMATCH


def detransform_into_filled_slots(N, flags, blobs, caps, key, aad, ctx, stride):
    """One detransform batch in device memory whose destination starts as 0xAB everywhere; slot i is `stride` bytes wide and is handed
    to the library with capacity caps[i].  -> (descs, the destination afterwards)."""
    soff, st = [], 0
    for b in blobs:
        soff.append(st); st += (len(b) + 15) // 16 * 16 + 16
    src = np.zeros(st, np.uint8)
    for b, o_ in zip(blobs, soff):
        src[o_:o_ + len(b)] = np.frombuffer(b, np.uint8)
    total = stride * len(blobs)
    d = pc.make_descs([len(b) for b in blobs], soff, [i * stride for i in range(len(blobs))], caps)
    ds, dd = N.device_malloc(src.size), N.device_malloc(total)
    try:
        N.h2d(ds, src); N.h2d(dd, np.full(total, 0xAB, np.uint8))
        N.detransform_batch(nat.Native.make_params(flags, key, aad), d, ds, dd, total, nat.MEM_DEVICE, ctx=ctx, src_size=src.size)
        back = np.zeros(total, np.uint8); N.d2h(back, dd)
    finally:
        N.device_free(ds); N.device_free(dd)
    return d, back


def check_matrix(N, o, flags, cases, key, aad, ctx, stride):
    """cases: (label, blob, slot capacity, the chunk the blob restores or None).  The statuses are exactly the OpenSSL oracle's; a
    rejected chunk reports no bytes and its slot holds the 0xAB it started with or zeros - nothing of a plaintext (none of the test's
    chunks is made of those two values alone); an accepted one is restored."""
    want = [oracle_status(o, key, aad, b) for _, b, _, _ in cases]
    assert want.count(0) == sum(1 for c in cases if c[3] is not None), "the oracle accepts a damaged chunk or rejects a clean one"
    d, back = detransform_into_filled_slots(N, flags, [c[1] for c in cases], [c[2] for c in cases], key, aad, ctx, stride)
    got = [int(x) for x in d["status"]]
    assert got == want, [(cases[i][0], len(cases[i][1]), got[i], want[i]) for i in range(len(cases)) if got[i] != want[i]]
    for i, (label, blob, cap, chunk) in enumerate(cases):
        slot = back[i * stride:(i + 1) * stride]
        if chunk is not None:
            assert d["dst_len"][i] == chunk.size and slot[:chunk.size].tobytes() == chunk.tobytes(), (label, len(blob))
        else:
            assert d["dst_len"][i] == 0, (label, len(blob), int(d["dst_len"][i]))
            assert np.isin(slot, (0, 0xAB)).all(), "%s (%d bytes): unauthenticated bytes left in the slot" % (label, len(blob))


def check_tamper_matrix(N, o, sizes=TAMPER_SIZES, compressed_sizes=(1000, 70001)):
    """Every one-bit flip that the device suite did not cover - IV, first and last ciphertext byte, both sides of a sub-block edge,
    each of the 16 tag bytes - and the two one-byte length changes, with one untouched blob per size, in ONE detransform batch; then
    two damaged compressed chunks, which must fail as tag mismatches (the frame decoder never sees them), through the block form of the
    decoder and the chunk form."""
    rng = np.random.default_rng([SEED, 5])
    key, aad, seg = draw(rng)
    chunks = rand_chunks(rng, sizes)
    assert all(not np.isin(c, (0, 0xAB)).all() for c in chunks)
    blobs = check_keyed(N, o, nat.ENCRYPT, chunks, key, aad, seg, "tamper matrix")
    cases = []
    for c, blob in zip(chunks, blobs):
        cases.append(("untouched", blob, int(c.size), c))
        cases += [(label, b, cap, None) for label, b, cap in encrypt_only_variants(int(c.size), blob)]
    stride = (max(sizes) + 1 + 63) // 64 * 64
    kchunks = [synth.gen_chunk("K", SEED % 1000, 9, i, s) for i, s in enumerate(compressed_sizes)]
    cflags = nat.COMPRESS | nat.ENCRYPT
    kblobs, kd = run_transform_keyed(N, cflags, kchunks, key, aad, seg)
    assert (kd["status"] == 0).all()
    if o.zstd_version().startswith("1.5.7"):
        assert kblobs == expected_blobs(o, cflags, key, aad, seg, kchunks)
    kcases = []
    for c, blob in zip(kchunks, kblobs):
        kcases += [("untouched", blob, int(c.size), c), ("last ciphertext byte", flip_bit(blob, len(blob) - 17, 2), int(c.size), None),
                   ("last tag byte", flip_bit(blob, len(blob) - 1, 7), int(c.size), None)]
    kstride = (max(compressed_sizes) + 63) // 64 * 64
    ctx = N.ctx_create(0, 0, 0)
    try:
        for form in ("block", "chunk"):
            with N.configured(**({"dec_block_chunks": 0} if form == "chunk" else {})):
                check_matrix(N, o, nat.ENCRYPT, cases, key, aad, ctx, stride)
                check_matrix(N, o, cflags, kcases, key, aad, ctx, kstride)
                took = pc.blockmode_chunks(N, ctx, len(kcases))
                assert (took >= 0) if form == "block" else (took == -1), (form, took)
    finally:
        N.ctx_destroy(ctx)
    return len(cases), len(kcases)
