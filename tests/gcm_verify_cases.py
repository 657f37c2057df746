"""Verify on upload, AES-GCM stage (TSX_VERIFY_GCM): helpers shared by the emulated and the device tests.  `N` is a tsxform._native.Native
(emulated or real); `o` is the oracle module.  The damage comes from the library's test hook verify_damage_out_chunk / _off: XOR 1 into one
byte of a chunk's delivered IV || C || TAG, behind the GCM stage and in front of the verifier, flag or no flag."""
import numpy as np

import tsxform
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
VG = getattr(nat, "VERIFY_GCM", 0x80)
E_VERIFY = getattr(nat, "E_VERIFY", -10)
ENC = nat.ENCRYPT
CE = nat.COMPRESS | nat.ENCRYPT
# memory kinds of run_transform: where the device delivers a chunk, and how it gets to the caller
MEMS = ("zero_copy", "host", "device", "packed", "packed_zc")
ENC_SIZES = [0, 1, 15, 16, 17, 4095, 65535, 65536, 65537, 131077, 200000]


def run_transform(N, flags, chunks, mem="zero_copy", level=3, ctx=None, **cfg):
    """One transform batch.  mem: "zero_copy" = host memory, slot layout, dst registered (the device writes the caller's buffer and the
    verifier reads it back); "host" = the same, dst pageable (the context's output buffer and the copy engine); "device"; "packed" =
    TSX_MEM_HOST_PACKED, dst pageable; "packed_zc" = packed, dst registered with room for every slot (a compressing batch is packed down
    in place).  cfg: test hooks for the call.  -> (outputs by dst_len, descs)."""
    sizes = [int(c.size) for c in chunks]
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N)
    src = np.zeros(max(st, 16), np.uint8)
    for c, o_ in zip(chunks, soff):
        src[o_:o_ + c.size] = c
    slot = (N.transformed_bound(max(sizes + [0]), flags) + 63) // 64 * 64
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
                N.transform_batch(p, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx, src_size=src.size)
                N.d2h(dst, dd)
            finally:
                N.device_free(ds); N.device_free(dd)
        else:
            if registered:
                N.host_register(dst)
            try:
                N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED if mem.startswith("packed") else nat.MEM_HOST, ctx=ctx)
            finally:
                if registered:
                    N.host_unregister(dst)
    return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))], d


def enc_chunks(sizes=ENC_SIZES):
    """Encrypt-only chunks: the block edge, the 64 KiB sub-block edge, a partial last block behind a full sub-block."""
    return [synth.gen_chunk("K" if i % 2 else "R", 61, 0, i, s) for i, s in enumerate(sizes)]


def comp_chunks():
    """K 131073, R 65791 (raw blocks: the frame crosses a sub-block edge), zeros 140000 (a frame of a few bytes), K 7, an empty chunk."""
    return [synth.gen_chunk("K", 53, 0, 0, 131073), synth.gen_chunk("R", 53, 0, 1, 65791), np.zeros(140000, np.uint8), synth.gen_chunk("K", 53, 0, 2, 7),
            np.zeros(0, np.uint8)]


def damage_enc_chunks():
    return enc_chunks([17, 65537, 0])


def damage_comp_chunks():
    return [synth.gen_chunk("R", 53, 0, 1, 65791), synth.gen_chunk("K", 53, 0, 2, 7)]


def check_clean(N, flags, chunks, mem, level=3, ctx=None, want=None, **cfg):
    """The batch with the flag: every chunk TSX_OK and the bytes of `want` (default: of the run without the flag).  -> the outputs."""
    if want is None:
        want, d0 = run_transform(N, flags, chunks, mem, level, ctx, **cfg)
        assert (d0["status"] == 0).all(), (mem, cfg, list(d0["status"]))
    outs, d = run_transform(N, flags | VG, chunks, mem, level, ctx, **cfg)
    assert (d["status"] == 0).all(), (mem, cfg, list(d["status"]))
    assert outs == want and [int(x) for x in d["dst_len"]] == [len(w) for w in want], (mem, cfg)
    return outs


def positions(L, full=True):
    """Offsets into a delivered IV || C || TAG whose ciphertext has L bytes: the IV's ends, the first block's ends and the second block's
    first byte, both sides of the first sub-block edge, the last ciphertext byte, the tag's first and last byte (a hit on the tag alone
    proves the GHASH path, not just the compare).  full=False: the last tag byte and one ciphertext byte (the IV's last where L = 0)."""
    if not full:
        return sorted({12 + L + 15, 12 + L - 1 if L else 11})
    at = [0, 11, 12, 27, 28, 12 + 65535, 12 + 65536, 12 + L - 1, 12 + L, 12 + L + 15]
    return sorted({p for p in at if 0 <= p < L + 28})


def targets(clean_outs, full=True):
    """[(chunk, offset)] over the chunks of a clean run's outputs."""
    return [(j, p) for j, out in enumerate(clean_outs) for p in positions(len(out) - 28, full)]


def check_damage(N, flags, chunks, mem, at, level=3, ctx=None, base=None, unflagged=True, **cfg):
    """Every (chunk j, offset) of `at`.  With the flag: chunk j alone is TSX_E_VERIFY with dst_len 0, every other chunk TSX_OK with the
    undamaged run's bytes.  Without it, the same hook: every chunk TSX_OK, the delivered bytes differ from the clean ones in that one bit,
    and detransform says TSX_E_TAG_MISMATCH for chunk j - the hook reached the output, and the flag is what catches it.  A clean run
    afterwards passes.  base: the clean run's outputs where the caller has them; unflagged=False leaves the runs without the flag out
    (full-size chunks on the device: a second of compression each).  -> damaged positions tried."""
    sizes = [int(c.size) for c in chunks]
    if base is None:
        base = check_clean(N, flags, chunks, mem, level, ctx, **cfg)
    for j, off in at:
        hook = dict(cfg, verify_damage_out_chunk=j, verify_damage_out_off=off)
        outs, d = run_transform(N, flags | VG, chunks, mem, level, ctx, **hook)
        assert [int(x) for x in d["status"]] == [E_VERIFY if i == j else 0 for i in range(len(chunks))], (mem, j, off, list(d["status"]))
        assert d["dst_len"][j] == 0 and outs[j] == b"", (mem, j, off)
        assert all(outs[i] == base[i] for i in range(len(chunks)) if i != j), (mem, j, off)
        if mem.startswith("packed"):                                    # a failed chunk takes no room: its successor starts where it would have
            assert [int(x) for x in d["dst_off"]] == [sum(len(x) for x in outs[:i]) for i in range(len(chunks))], (mem, j, off)
        if not unflagged:
            continue
        outs, d = run_transform(N, flags, chunks, mem, level, ctx, **hook)
        assert (d["status"] == 0).all(), (mem, j, off, list(d["status"]))
        hit = bytearray(base[j]); hit[off] ^= 1
        assert outs[j] == bytes(hit) and all(outs[i] == base[i] for i in range(len(chunks)) if i != j), (mem, j, off)
        back, d2 = pc.run_detransform(N, flags, outs, sizes)
        assert [int(x) for x in d2["status"]] == [nat.E_TAG_MISMATCH if i == j else 0 for i in range(len(chunks))], (mem, j, off, list(d2["status"]))
    assert check_clean(N, flags, chunks, mem, level, ctx, want=base, **cfg) == base
    return len(at)
