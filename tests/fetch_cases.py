"""The fetch side in a broker's shapes: foreign and damaged Zstandard frames BEHIND the GCM stage, mixed verdicts through the 16..256-chunk
piece pipeline, segment-sized slots laid back to back, and what one context (or the pool) carries from a batch to the next.  Bodies shared
by the emulated (tests/test_emu_fetch.py) and the device tests (the gpu_fetch file).

The corpus is built on the CPU without the code under test: one (key, AAD, segment) per batch from a fixed seed, an IV of its own for
every chunk, every blob `o.gcm_encrypt_chunk(key, iv, aad, frame, openssl=True)` - a damaged frame too, so that its tag is valid and only
the decoder can refuse it.  The reference of a chunk (`expect`): shorter than 28 bytes -> TSX_E_SHORT_CHUNK; OpenSSL refuses the blob ->
TSX_E_TAG_MISMATCH; otherwise libzstd's verdict on the frame at the slot's capacity, judged by frame_vocab_cases.apply_rules.  One decoder
form is never the only evidence for the other.  `N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import collections
import ctypes as C
import threading

import numpy as np

import tsxform
from tests import checksum_cases as cc
from tests import frame_vocab_cases as fv
from tests import keying_cases as kc
from tests import parity_cases as pc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
SEED = 20261021
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
JAVA = nat.COMPRESS | nat.ENCRYPT                                        # the flags word GpuDetransformChunkEnumeration.java passes
FILL = 0xAB
CLEAN, BAD_FRAME, ACCEPTED, BAD_TAG, SHORT, SMALL = "clean", "bad frame", "accepted damage", "bad tag", "short", "slot too small"
FAILING = (BAD_FRAME, BAD_TAG, SHORT, SMALL)
SMALL_SOURCE = 65536                                                     # batches of 256 and 257 chunks take sources up to this size only
K60000 = ("K level -5", "K window 10", "K checksum")                     # the three K(60000) frames of the vocabulary: they fill a slot of 60000
TOO_SMALL_OF = ("skewlow 5000", "K level -5")
TAMPERS = ("iv", "first ciphertext byte", "last ciphertext byte", "tag")

# cls; name; frame: the Zstandard frame inside the blob (None: no blob of 28 bytes or more); size: the source's size, which the slot's
# capacity comes from; tamper: which bit of the blob is flipped (bad tag); raw: the blob's length where it holds no frame (short);
# shrink: bytes the slot lacks (slot too small); kind: the damaged region (bad frame); blocks: the frame's block count (clean)
Template = collections.namedtuple("Template", "cls name frame size tamper raw shrink kind blocks")


def _t(cls, name, frame, size, tamper=None, raw=0, shrink=0, kind=None, blocks=0):
    return Template(cls, name, frame, int(size), tamper, raw, shrink, kind, blocks)


_CORPUS = None


def corpus(o):
    """{class: [Template]} - see the module text.  Built once; libzstd and the inspector alone decide what goes where."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    cc.need157(o)
    V, D = fv.vocabulary(o), fv.damaged(o)
    clean = [_t(CLEAN, name, f, len(x), blocks=len(zi.parse_frame(f, decode=False)[1])) for name, x, f in V]
    by_name = {t.name: t for t in clean}
    bad = []
    for kind in fv.KINDS:                                               # the first flip of each kind that libzstd rejects
        first = next((d for d in D if d.kind == kind and "flip" in d.how and isinstance(d.verdict, str)), None)
        if first is not None:
            bad.append(_t(BAD_FRAME, "%s, %s, base %d" % (kind, first.how, first.base), first.blob, first.size, kind=kind))
    for how in ("truncation", "insertion"):
        first = next(d for d in D if d.how == how and isinstance(d.verdict, str))
        bad.append(_t(BAD_FRAME, "%s at %s, base %d" % (how, first.kind, first.base), first.blob, first.size))
    acc = []
    for d in D:                                                         # libzstd decodes it to OTHER bytes, and RFC 8878 has no objection
        if len(acc) < 3 and isinstance(d.verdict, bytes) and not fv.inspector_is_strict(d.blob):
            if d.verdict != _base_source(o, d.base):
                acc.append(_t(ACCEPTED, "%s, %s, base %d" % (d.kind, d.how, d.base), d.blob, d.size))
    tag = [_t(BAD_TAG, "%s of %s" % (how, clean[k].name), clean[k].frame, clean[k].size, tamper=how) for k, how in zip((10, 12, 13, 0), TAMPERS)]
    short = [_t(SHORT, "%d bytes" % n, None, 1000, raw=n) for n in (0, 27)]
    small = [by_name[name]._replace(cls=SMALL, shrink=1) for name in TOO_SMALL_OF]
    _CORPUS = {CLEAN: clean, BAD_FRAME: bad, ACCEPTED: acc, BAD_TAG: tag, SHORT: short, SMALL: small}
    return _CORPUS


_BASE = {}


def _base_source(o, bi):
    """What the undamaged frame of damaged-corpus base `bi` restores, by libzstd."""
    if bi not in _BASE:
        x, params = fv._bases()[bi]
        _BASE[bi] = fv.libzstd_verdict(o, fv.libzstd_frame(o, x, params), x.size)
        assert _BASE[bi] == x.tobytes()
    return _BASE[bi]


def check_corpus(o):
    """Conditions on the inputs, asserted before the first call: nothing here is a measurement of the code under test."""
    co = corpus(o)
    for cls in (CLEAN, BAD_FRAME, ACCEPTED, BAD_TAG, SHORT, SMALL):
        assert co[cls], "corpus class %r is empty" % cls
    kinds = {t.kind for t in co[BAD_FRAME] if t.kind}
    print("fetch corpus: %s; damage kinds among the bad frames: %d of %d" % ({k: len(v) for k, v in co.items()}, len(kinds), len(fv.KINDS)))
    assert kinds == set(fv.KINDS), "libzstd accepts every flip of: %s" % sorted(set(fv.KINDS) - kinds)
    assert len(co[CLEAN]) == 18 and len(co[ACCEPTED]) == 3 and len(co[BAD_TAG]) == 4 and len(co[SMALL]) == 2
    assert max(t.blocks for t in co[CLEAN]) > fv.ZB_MAX_BLOCKS
    for t in co[BAD_FRAME]:
        assert isinstance(fv.libzstd_verdict(o, t.frame, t.size), str), t.name
    for t in co[ACCEPTED]:
        v = fv.libzstd_verdict(o, t.frame, t.size)
        assert isinstance(v, bytes) and len(v) == t.size, t.name
    for name in K60000:
        assert [t.size for t in co[CLEAN] if t.name == name] == [60000], name
    small = {cls: [t for t in ts if t.size <= SMALL_SOURCE] for cls, ts in co.items()}
    assert all(small[cls] for cls in small) and len({t.kind for t in small[BAD_FRAME] if t.kind}) >= 10
    assert max(t.size for ts in small.values() for t in ts) == 60000     # segment caps of 60000: the K(60000) frames fill their slots
    return co


# ---- the cut of a batch -------------------------------------------------------------------------------------------------------------
def pieces(n):
    """[(first chunk, chunks)] of a host-memory fetch of n chunks, restated from run_batch_inner (csrc/tsx_batch.hip): 16 .. 256 chunks go
    in pieces of max(8, ceil(n / 8)) chunks, at most 8 of them, the last piece taking what is left; anything else is one piece."""
    if not 16 <= n <= 256:
        return [(0, n)]
    per = max(8, (n + 7) // 8)
    cut = [(lo, min(per, n - lo)) for lo in range(0, n, per)]
    if len(cut) > 8:
        cut = cut[:7] + [(cut[7][0], n - cut[7][0])]
    return cut


def check_pieces_rule():
    want = {15: [15], 16: [8, 8], 17: [8, 8, 1], 33: [8, 8, 8, 8, 1], 65: [9] * 7 + [2], 256: [32] * 8, 257: [257], 40: [8] * 5, 3: [3]}
    for n, sizes in want.items():
        assert [c for _, c in pieces(n)] == sizes, (n, pieces(n))
        assert [lo for lo, _ in pieces(n)] == [sum(sizes[:k]) for k in range(len(sizes))]


def block_form_pieces(n):
    """What tsx_debug_blockmode_pieces says after a host-memory fetch of n chunks: 0 beyond 256 chunks (the chunk form's)."""
    return 0 if n > 256 else len(pieces(n))


# ---- a batch ------------------------------------------------------------------------------------------------------------------------
class Plan:
    """n chunks: templates, slot capacities, source and destination offsets.  Nothing of a key yet."""

    def __init__(self, templates, caps, layout):
        self.t = list(templates)
        self.n = len(self.t)
        self.segment_caps = caps == "segment"
        seg = (max(t.size for t in self.t) + 15) // 16 * 16
        self.slot = [seg if self.segment_caps else t.size for t in self.t]          # what the layout reserves
        self.cap = [t.size - t.shrink if t.shrink else s for s, t in zip(self.slot, self.t)]     # what the descriptor says: a slot too small is one byte under the CONTENT size
        self.doff, at = [], 0
        for s in self.slot:
            self.doff.append(at)
            at += (s + 15) // 16 * 16 + (16 if layout == "padded" else 0)
        self.total = max(at, 16)
        if layout == "contiguous" and self.segment_caps:
            assert self.doff == [i * seg for i in range(self.n)]
        self.blob_len = [t.raw if t.frame is None else len(t.frame) + 28 for t in self.t]
        self.soff, at = [], 0
        for s in self.blob_len:
            self.soff.append(at); at += (s + 15) // 16 * 16 + 16
        self.src_total = max(at, 16)

    def failing(self):
        return [i for i, t in enumerate(self.t) if t.cls in FAILING]


def fail_positions(n):
    """Where a failing chunk must sit: index 0, the last chunk of piece 0, the first of piece 1, the first of piece 4 (its compute stream
    is piece 0's again), index n - 1."""
    cut = pieces(n)
    at = {0, cut[0][1] - 1, n - 1}
    if len(cut) > 1:
        at.add(cut[1][0])
    if len(cut) > 4:
        at.add(cut[4][0])
    return sorted(at)


def make_plan(o, n, caps, layout, small=False, rot=0):
    """The fixed rule.  Chunks 1 .. 6 (inside piece 0 whatever the cut) are the three K(60000) frames, then the first and the third of
    them around a bad frame: under segment caps of 60000 laid back to back the first three are ONE copy and the bad frame breaks the
    second run.  Failing chunks sit at fail_positions(n), at index 5 and evenly over the rest, max(8, n // 4) of them from 16 chunks
    on: the first eight are two of each failing class, then three bad frames to one of the others.  Every other chunk cycles through the
    clean frames and the accepted damage.  `rot` turns the cycles, so that batches of one size differ."""
    co = corpus(o)
    if small:
        co = {cls: [t for t in ts if t.size <= SMALL_SOURCE] for cls, ts in co.items()}
    if n < 8:                                                           # too short for the runs: bad frame, clean, bad tag, clean, ...
        order = [co[CLEAN][(rot + i) % len(co[CLEAN])] if i % 2 else (co[BAD_TAG][(rot + i) % 4] if i % 4 else co[BAD_FRAME][(rot + i) % len(co[BAD_FRAME])])
                 for i in range(n)]
        return Plan(order, caps, layout)
    by_name = {t.name: t for t in corpus(o)[CLEAN]}
    k1, k2, k3 = (by_name[x] for x in K60000)
    slots = [None] * n
    nbf = len(co[BAD_FRAME])
    slots[1:7] = [k1, k2, k3, k1, co[BAD_FRAME][rot % nbf], k3]
    fixed = [i for i in fail_positions(n) if slots[i] is None]
    want = max(len(fixed) + 1, 8 if n >= 16 else 0, n // 4)
    free = [i for i in range(n) if slots[i] is None and i not in fixed]
    more = want - 1 - len(fixed)
    spread = [free[(2 * k + 1) * len(free) // (2 * more)] for k in range(more)] if more > 0 else []
    assert len(set(spread)) == len(spread)
    others = [co[BAD_TAG][0], co[SHORT][0], co[SMALL][0], None, co[BAD_TAG][1], co[SHORT][1], co[SMALL][1]]      # with index 5's: two of each
    tail = co[BAD_TAG][2:] + co[SHORT] + co[SMALL] + co[BAD_TAG][:2]
    nf = 1
    for j, i in enumerate(sorted(fixed + spread)):
        t = others[j] if j < len(others) else (None if (j - len(others)) % 4 else tail[((j - len(others)) // 4 + rot) % len(tail)])
        if t is None:
            t = co[BAD_FRAME][(rot + nf) % nbf]; nf += 1
        slots[i] = t
    rest = [i for i in range(n) if slots[i] is None]
    nacc = max(0, min(len(co[ACCEPTED]), len(rest) + 5 - (n + 1) // 2))                 # accepted damage where half the batch stays clean without it
    for k in range(nacc):
        slots[rest[(2 * k + 1) * len(rest) // (2 * nacc)]] = co[ACCEPTED][(k + rot) % len(co[ACCEPTED])]
    for j, i in enumerate(i for i in rest if slots[i] is None):
        slots[i] = co[CLEAN][(j + rot) % len(co[CLEAN])]
    return Plan(slots, caps, layout)


def check_plan(o, p, mixed=True):
    """Conditions on a batch, from the reference alone: (for 16 chunks and more) at least two chunks of each failing class - by what the
    reference expects at the slot's capacity, not by the template's name - and at least half clean chunks; a failing chunk at each of
    fail_positions."""
    exp = [expect_of(o, t, cap) for t, cap in zip(p.t, p.cap)]
    if not mixed:
        assert all(t.cls == CLEAN and isinstance(e, bytes) for t, e in zip(p.t, exp))
        return exp
    for i in fail_positions(p.n):
        assert p.t[i].cls in FAILING and not isinstance(exp[i], bytes), (p.n, i, p.t[i].name)
    if p.n >= 16:
        per = collections.Counter(p.t[i].cls for i in p.failing() if not isinstance(exp[i], bytes))
        assert all(per[cls] >= 2 for cls in FAILING), (p.n, dict(per))
        clean = sum(t.cls == CLEAN and isinstance(e, bytes) for t, e in zip(p.t, exp))
        assert 2 * clean >= p.n, (p.n, clean)
    return exp


_VERDICT = {}


def expect_of(o, t, cap):
    """The reference for a chunk in a slot of `cap` bytes, as far as it does not depend on the key: the restored bytes, or the status (an
    int) where only one is right, or libzstd's error name (a str): any status of fv.REJECT."""
    if t.cls == SHORT:
        return nat.E_SHORT_CHUNK
    if t.cls == BAD_TAG:
        return nat.E_TAG_MISMATCH
    key = (t.frame, cap)
    if key not in _VERDICT:
        _VERDICT[key] = fv.libzstd_verdict(o, t.frame, cap)
    return _VERDICT[key]


def tamper(blob, how):
    at = {"iv": (5, 1), "first ciphertext byte": (12, 3), "last ciphertext byte": (len(blob) - 17, 5), "tag": (len(blob) - 9, 6)}[how]
    return kc.flip_bit(blob, at[0], at[1])


def blobs_of(o, p, key, aad, segment):
    """IV || C || TAG of every chunk of the plan under this key, by OpenSSL; the oracle's verdict on each is asserted here."""
    out = []
    for i, t in enumerate(p.t):
        if t.frame is None:
            out.append(bytes([0x5A] * t.raw)); continue
        b = o.gcm_encrypt_chunk(key, synth.iv_for(segment, i), aad, t.frame, openssl=True)
        if t.tamper:
            b = tamper(b, t.tamper)
        assert kc.oracle_status(o, key, aad, b) == (nat.E_TAG_MISMATCH if t.tamper else 0), (i, t.name)
        out.append(b)
    assert [len(b) for b in out] == p.blob_len
    return out


def hook(N, name):
    f = getattr(N.lib, name); f.restype = C.c_int; f.argtypes = [C.c_void_p]
    return f


Result = collections.namedtuple("Result", "status dst_len crc outs")


def run_plan(N, o, p, exp, keyed, flags, mem, ctx, dst=None):
    """One detransform batch of plan p under keyed = (key, AAD, segment), checked against the reference `exp` (check_plan's).
    mem: "pageable", "registered" or "device".  dst: the caller's own host destination (a view of a larger buffer that it watches); it
    must hold FILL.  -> Result."""
    key, aad, seg = keyed
    blobs = blobs_of(o, p, key, aad, seg)
    src = np.zeros(p.src_total, np.uint8)
    for b, at in zip(blobs, p.soff):
        src[at:at + len(b)] = np.frombuffer(b, np.uint8)
    if dst is None:
        dst = np.full(p.total, FILL, np.uint8)
    assert dst.size == p.total and (dst == FILL).all()
    d = pc.make_descs(p.blob_len, p.soff, p.doff, p.cap, segment=seg)
    d["status"] = -77; d["dst_len"] = 123; d["crc32c"] = 0x5A5A5A5A      # nothing of a reused descriptor survives
    prm = nat.Native.make_params(flags, key, aad)
    if mem == "device":
        ds, dd = N.device_malloc(src.size), N.device_malloc(dst.size)
        try:
            N.h2d(ds, src); N.h2d(dd, dst)
            N.detransform_batch(prm, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx, src_size=src.size)
            N.d2h(dst, dd)
        finally:
            N.device_free(ds); N.device_free(dd)
    else:
        if mem == "registered":
            N.host_register(src); N.host_register(dst)
        try:
            N.detransform_batch(prm, d, src, dst, dst.size, nat.MEM_HOST, ctx=ctx)
        finally:
            if mem == "registered":
                N.host_unregister(dst); N.host_unregister(src)
    status = [int(x) for x in d["status"]]
    lens = [int(x) for x in d["dst_len"]]
    outs = [dst[p.doff[i]:p.doff[i] + lens[i]].tobytes() for i in range(p.n)]
    wrong = []
    image = np.full(p.total, FILL, np.uint8)                            # what the destination must look like
    for i, (t, e) in enumerate(zip(p.t, exp)):
        if isinstance(e, int):
            if status[i] != e:
                wrong.append((i, t.name, "status %d, the reference %d" % (status[i], e)))
        else:
            cls, err = fv.apply_rules(t.frame, p.cap[i], e, status[i], outs[i])
            if err:
                wrong.append((i, t.name, err))
        if status[i] != 0:
            if lens[i] != 0:
                wrong.append((i, t.name, "status %d with dst_len %d" % (status[i], lens[i])))
        elif isinstance(e, bytes):
            image[p.doff[i]:p.doff[i] + len(e)] = np.frombuffer(e, np.uint8)
            if flags & nat.CRC and int(d["crc32c"][i]) != o.crc32c(e):
                wrong.append((i, t.name, "crc32c %08x of %d restored bytes, the oracle %08x" % (int(d["crc32c"][i]), len(e), o.crc32c(e))))
    assert not wrong, (p.n, mem, wrong[:8])
    if mem != "device":                                                 # no byte outside the restored bytes of the OK chunks has changed
        diff = np.flatnonzero(dst != image)
        assert diff.size == 0, "%d chunks, %s: %d bytes differ from the expected image, the first at %d (%s)" % (p.n, mem, diff.size, int(diff[0]), _where(p, int(diff[0])))
    else:
        in_slot = np.zeros(p.total, bool)
        for i in range(p.n):
            in_slot[p.doff[i]:p.doff[i] + p.cap[i]] = True
        gaps = np.flatnonzero(~in_slot & (dst != FILL))
        assert gaps.size == 0, "%d chunks, device: %d bytes between the slots changed, the first at %d (%s)" % (p.n, gaps.size, int(gaps[0]), _where(p, int(gaps[0])))
        for i, t in enumerate(p.t):
            if t.cls == BAD_TAG:
                assert np.isin(dst[p.doff[i]:p.doff[i] + p.cap[i]], (0, FILL)).all(), "chunk %d (%s): unauthenticated bytes in the slot" % (i, t.name)
    return Result(status, lens, [int(x) for x in d["crc32c"]], outs)


def _where(p, at):
    i = max(k for k in range(p.n) if p.doff[k] <= at)
    return "chunk %d, %s, byte %d of a slot of %d" % (i, p.t[i].name, at - p.doff[i], p.cap[i])


def block_form_floor(p):
    """Chunks the block form must have decoded itself: clean, a source of its own, at most ZB_MAX_BLOCKS blocks, a slot that holds them."""
    return sum(t.cls == CLEAN and len(t.frame) > 0 and t.blocks <= fv.ZB_MAX_BLOCKS for t in p.t)


# ---- body 1 -------------------------------------------------------------------------------------------------------------------------
SHAPES = [15, 16, 17, 33, 65, 256, 257]
MEMS = ("pageable", "registered", "device")


def keyed(*tag):
    return kc.draw(np.random.default_rng([SEED] + [int(x) for x in tag]))


def check_shapes(N, o, n, caps, layout, mem, flags=FULL):
    """A mixed batch of n chunks on an explicit context: the cut, the reference, the destination image, the block form's share."""
    check_corpus(o)
    check_pieces_rule()
    p = make_plan(o, n, caps, layout, small=n >= 256, rot=n)
    exp = check_plan(o, p)
    ctx = N.ctx_create(0, 0, 0)
    try:
        res = run_plan(N, o, p, exp, keyed(1, n), flags, mem, ctx)
        took = pc.blockmode_chunks(N, ctx, n)
        cut = hook(N, "tsx_debug_blockmode_pieces")(ctx)
    finally:
        N.ctx_destroy(ctx)
    print("%d chunks, %s caps, %s, %s: statuses %s, block form kept %d (floor %d), %d pieces" %
          (n, caps, layout, mem, dict(collections.Counter(res.status)), took, block_form_floor(p), cut))
    if n > 256:
        assert took == -1 and cut == 0, (took, cut)
    else:
        assert took >= block_form_floor(p), (took, block_form_floor(p))
        assert cut == (block_form_pieces(n) if mem != "device" else 1), (n, mem, cut)
    return res


# ---- body 2 -------------------------------------------------------------------------------------------------------------------------
def check_forms_and_cuts(N, o, sizes=(33, 65)):
    """The plans of 33 and 65 chunks as cut by default, in one piece, and through the chunk form: each held to the reference on its own,
    then equal to each other in statuses, lengths, bytes and CRCs."""
    check_corpus(o)
    for n in sizes:
        p = make_plan(o, n, "segment", "contiguous", small=True, rot=n + 1)
        exp = check_plan(o, p)
        ctx = N.ctx_create(0, 0, 0)
        res = {}
        try:
            for form, cfg in (("pieces", {}), ("one piece", {"no_dec_pieces": 1}), ("chunk form", {"dec_block_chunks": 0})):
                with N.configured(**cfg):
                    res[form] = run_plan(N, o, p, exp, keyed(2, n), FULL, "pageable", ctx)
                    cut, took = hook(N, "tsx_debug_blockmode_pieces")(ctx), pc.blockmode_chunks(N, ctx, n)
                assert cut == {"pieces": block_form_pieces(n), "one piece": 1, "chunk form": 0}[form], (n, form, cut)
                assert (took == -1) if form == "chunk form" else (took >= block_form_floor(p)), (n, form, took)
        finally:
            N.ctx_destroy(ctx)
        assert res["pieces"] == res["one piece"] == res["chunk form"], n


# ---- body 3 -------------------------------------------------------------------------------------------------------------------------
def sequence_plans(o):
    """Calls A .. E (E is A's plan): (name, plan, reference)."""
    co = [t for t in corpus(o)[CLEAN] if t.size <= 272000]              # (the one larger source, 310000 bytes, is in the other bodies' batches)
    a = Plan([co[i % len(co)] for i in range(40)], "segment", "contiguous")
    plans = [("A", a, check_plan(o, a, mixed=False))]
    for name, n, small, layout in (("B", 17, True, "contiguous"), ("C", 3, True, "padded"), ("D", 257, True, "contiguous")):
        p = make_plan(o, n, "segment", layout, small=small, rot=3)
        plans.append((name, p, check_plan(o, p)))
    plans.append(("E", a, plans[0][2]))
    assert a.slot[0] == 272000 and plans[1][1].slot[0] == 60000 and plans[3][1].slot[0] == 60000
    assert all(plans[1][1].t[i].cls in FAILING for i in fail_positions(17)) and {BAD_FRAME, BAD_TAG} <= {t.cls for t in plans[1][1].t}
    return plans


def check_one_context_in_sequence(N, o):
    """Five fetches of different shapes on ONE explicit context into disjoint regions of ONE host buffer that is filled once: every call is
    held to the reference, its region to its image, and every byte of the buffer outside its region to what it was before the call - the
    plaintext of the earlier calls stays where a leak would have to put it."""
    check_corpus(o)
    plans = sequence_plans(o)
    at, offs = 0, []
    for _, p, _ in plans:
        offs.append(at); at += p.total + 4096
    big = np.full(at, FILL, np.uint8)
    ctx = N.ctx_create(0, 0, 0)
    try:
        for k, (name, p, exp) in enumerate(plans):
            before = big.copy()
            region = big[offs[k]:offs[k] + p.total]
            res = run_plan(N, o, p, exp, keyed(3, k), FULL, "pageable", ctx, dst=region)
            before[offs[k]:offs[k] + p.total] = region
            assert (big == before).all(), "call %s wrote outside its region" % name
            assert pc.blockmode_chunks(N, ctx, p.n) >= block_form_floor(p) if p.n <= 256 else pc.blockmode_chunks(N, ctx, p.n) == -1, name
            print("call %s: %d chunks, statuses %s" % (name, p.n, dict(collections.Counter(res.status))))
    finally:
        N.ctx_destroy(ctx)


# ---- body 4 -------------------------------------------------------------------------------------------------------------------------
def check_pooled_callers(N, o, threads=4, shapes=(17, 33, 40)):
    """`threads` callers without a context, each with a key, AAD and segment of its own, each making one fetch per shape (in an order of
    its own), all released together: every batch is held to the reference, and the pool has every context back afterwards."""
    check_corpus(o)
    work = []
    for t in range(threads):
        mine = []
        for k in range(len(shapes)):
            n = shapes[(k + t) % len(shapes)]
            p = make_plan(o, n, "segment", "contiguous" if (k + t) % 2 else "padded", small=True, rot=7 * t + k)
            mine.append((p, check_plan(o, p)))
        work.append(mine)
    gate = threading.Barrier(threads)
    errors = []

    def caller(t):
        try:
            gate.wait()
            for k, (p, exp) in enumerate(work[t]):
                run_plan(N, o, p, exp, keyed(4, t), FULL, "pageable", None)
        except BaseException as e:                                      # noqa: BLE001 - reported through the list
            errors.append((t, repr(e)[:2000]))

    th = [threading.Thread(target=caller, args=(t,)) for t in range(threads)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errors, errors[:4]
    assert N.pool_stats(0)["in_use"] == 0
