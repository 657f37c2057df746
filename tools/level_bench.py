#!/usr/bin/env python3
"""Zstandard levels 1, 2 and 3 side by side on one device, one process: bench.py's `value` shape (8 x 1 GiB segments of content K resident
in HBM, 4 MiB chunks, CRC32C + Zstd + AES-256-GCM, 5 callers, device-resident batches) and its `value_B` shape (64 distinct chunks of content
B replicated over the same batch).  The levels run in alternating order (1 2 3, then 3 2 1, ...); for every run: GiB/s of original bytes,
transformed / original, and the compressor service's kernel time; a sample of every level's timed chunks is checked against libzstd
(+ the oracle's GCM).  One JSON line per run, then a summary line.
--checksum: every level runs twice per round, with and without a content checksum in its frames (TSX_ZSTD_CHECKSUM), alternating the same
way; the frames with one are checked against libzstd's own ZSTD_c_checksumFlag frames.
--verify: the same for verify on upload (TSX_VERIFY): every level without and with it, alternating (off on, on off, ... in one process); the
rows of the verifying runs carry the verifier's own time of the last batch (tsx_timing.unzstd_ms, unzstd_launches).
--verify-gcm: the same for the GCM stage's verify on upload (TSX_VERIFY_GCM): off on, on off in one process; the verifying runs' rows carry
the GCM stage's time and launches of the last batch (tsx_timing.gcm_ms, gcm_launches: the verifier's, the waves encrypt their own frames).
The rows are appended to --out as well (default with --verify-gcm: profiles/gcm_verify_level_bench.jsonl).
--records: record-batch validation (TSX_VALIDATE_RECORDS) off / on / on / off in one process, on ONE segment of content B that is a valid
stream from its first byte to its last (64 distinct B chunks, each cut at its last complete batch, repeated up to 256 chunks of 4 MiB:
batches cross chunk boundaries wherever they fall), level 3, --callers contexts.  The validating runs' rows carry the validator's own time
and counters of the last 256-chunk batch (tsx_records_info.ms, repaired_chunks, batches) and, next to them, the separate-stage CRC
kernels' crc_ms over the same bytes (tsx_crc32c_batch): what streaming those bytes through a CRC costs.  Default --out:
profiles/records_level_bench.jsonl.
--records-stream: the same segment, 5 callers, with the validation STREAMED over four calls of 64 chunks (tsx_transform_batch_stream, one state
per segment) against the one 256-chunk call: off / streamed / one call / off in one process, and a fifth run with the same four calls per segment without
the flag (a caller issues its calls one after another: what batches of 64 cost by themselves).  The rows carry GiB/s, the validator's time
summed over the segment's calls (records_ms; records_ms_calls: per call of the last segment) and the pinned source a broker's upload thread
would hold for such a batch (pinned_source_bytes: gpuBatchChunks x chunk size).  Default --out: profiles/records_stream_level_bench.jsonl.
--records-frames: the same segment, 5 callers, TSX_VALIDATE_RECORDS alone / with TSX_VALIDATE_FRAMES / with it / alone in one process (the
64 generated pieces repeat four times: every repetition's base offsets are moved up, which needs no new CRC, so that the order of offsets
holds over the whole stream).  Per run the GiB/s, tsx_records_info.ms and the records read.  Default --out:
profiles/records_frames_level_bench.jsonl.
--device-profile: TSX_ZSTD_PROFILE_DEVICE (standard frames from the lane-parallel parse, no library's bytes) against the exact level 3 of
profile 1.5.7 in the same process: 1.5.7 / device / device / 1.5.7 per content.  Two regimes: the `value` shape (the defaults: 5 callers,
8 x 1 GiB) and a lone segment (--callers 1 --segments 1: one 256-chunk batch at a time).  Every row carries GiB/s, frames / original and
the service's kernel time; the exact rows' sample is compared with libzstd's frames, the device rows' sample is opened with the oracle's
GCM and DECODED by libzstd.  Default --out: profiles/device_profile_level_bench.jsonl.
  python tools/level_bench.py [--steps 20] [--warmup 5] [--callers 5] [--rounds 2] [--contents K,B] [--segments 8] [--levels 3] [--checksum] [--verify]
                              [--verify-gcm] [--records] [--records-stream] [--records-frames] [--device-profile] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GiB = float(1 << 30)


def _gen_b_chunk(a):
    """(worker of a spawned process pool) one chunk of content B."""
    from tsxform import synth
    return synth.gen_chunk("B", a[0], a[1], a[2], a[3])


def _gen_b_stream_piece(a):
    """(worker of a spawned process pool) one chunk of content B cut at the end of its last complete batch."""
    from tsxform import synth
    c = synth.gen_chunk("B", a[0], a[1], a[2], a[3])
    p, l = synth.record_batches_of(c)[-1]
    return c[:p + l]


def records_bench(args, emit):
    import torch  # before libtsxform: one shared HIP runtime
    import tsxform
    from tsxform import synth
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    nat = tsxform._native
    N = tsxform.get()
    dev = torch.device("cuda", 0)
    CH, T = synth.CHUNK, args.callers
    t_gen = time.perf_counter()
    with ProcessPoolExecutor(16, mp_context=mp.get_context("spawn")) as ex:
        pieces = list(ex.map(_gen_b_stream_piece, [(1000, 0, c, CH) for c in range(64)]))
    parts = [pieces[i % 64] for i in range(256)]
    if args.records_frames:
        for i in range(64, 256):
            c = parts[i].copy()
            for p_, l_ in synth.record_batches_of(c):
                c[p_:p_ + 8] = np.frombuffer((int.from_bytes(bytes(c[p_:p_ + 8]), "big") + ((i // 64) << 40)).to_bytes(8, "big"), np.uint8)
            parts[i] = c
    stream = np.concatenate(parts)
    total = int(stream.size)
    n = (total + CH - 1) // CH
    gen_s = time.perf_counter() - t_gen
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    slot = (N.transformed_bound(CH, flags) + 63) // 64 * 64
    src = torch.from_numpy(stream).to(dev)
    dsts = [torch.empty(n * slot, dtype=torch.uint8, device=dev) for _ in range(T)]
    d = np.zeros(n, nat.DESC_DTYPE)
    d["src_off"] = np.arange(n, dtype=np.uint64) * CH; d["src_len"] = CH; d["src_len"][n - 1] = total - (n - 1) * CH
    d["dst_off"] = np.arange(n, dtype=np.uint64) * slot; d["dst_cap"] = slot
    for i in range(n):
        d["iv"][i] = np.frombuffer(synth.iv_for(0, i), np.uint8)
    ctxs = [N.ctx_create(0, n, CH) for _ in range(T)]
    dc = d.copy()
    N.crc32c_batch(dc, src.data_ptr(), nat.MEM_DEVICE, ctx=ctxs[0], src_size=total)
    N.crc32c_batch(dc, src.data_ptr(), nat.MEM_DEVICE, ctx=ctxs[0], src_size=total)
    crc_ms = N.ctx_timing(ctxs[0]).crc_ms
    rows = []
    PER = 64                                                            # chunks per call of a streamed segment
    last_ms = [[] for _ in range(T)]
    # (the fifth run of --records-stream: the same four calls per segment without the flag - what the smaller batches cost by themselves)
    for mode in (("off", "streamed", "one call", "off", "off, four calls") if args.records_stream else
                 ("one call", "one call, frames", "one call, frames", "one call") if args.records_frames else ("off", "one call", "one call", "off")):
        on = not mode.startswith("off")
        frames = mode.endswith("frames")
        cut = mode in ("streamed", "off, four calls")
        p = nat.Native.make_params(flags | (nat.VALIDATE_RECORDS if on else 0) | (nat.VALIDATE_FRAMES if frames else 0), synth.KEY, synth.AAD, zstd_level=3)
        ds = [d.copy() for _ in range(T)]

        def step(t):
            if not cut:
                N.transform_batch(p, ds[t], src.data_ptr(), dsts[t].data_ptr(), dsts[t].numel(), nat.MEM_DEVICE, ctx=ctxs[t], src_size=total)
                return
            state = N.records_begin(total) if on else None
            last_ms[t] = []
            for lo in range(0, n, PER):
                N.transform_batch(p, ds[t][lo:lo + PER], src.data_ptr(), dsts[t].data_ptr(), dsts[t].numel(), nat.MEM_DEVICE, ctx=ctxs[t], src_size=total, state=state)
                if on:
                    last_ms[t].append(N.records_result(state)[1].ms)
            if not on:
                return
            done, info = N.records_result(state)
            assert done and info.first_bad_reason == 0, (done, info.first_bad_pos, info.first_bad_reason)
        for w in range(max(args.warmup, 1)):
            for t in (range(T) if w == 0 else range(1)):
                step(t)
        torch.cuda.synchronize()
        N.service_quiesce(0)

        def worker(t):
            for _ in range(t, args.steps, T):
                step(t)
        t0 = time.perf_counter()
        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        [x.start() for x in th]
        [x.join() for x in th]
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        N.service_quiesce(0)
        ok = all(bool((x["status"] == 0).all()) for x in ds) and all(bool((x["dst_len"] == ds[0]["dst_len"]).all()) for x in ds)
        r = N.ctx_records(ctxs[0])
        row = {"content": "B stream", "level": 3, "records": on, "mode": mode, "calls_per_segment": (n + PER - 1) // PER if cut else 1,
               "pinned_source_bytes": (PER if cut else n) * CH, "gibs": round(args.steps * total / GiB / el, 3), "elapsed_s": round(el, 3), "chunks": n, "stream_bytes": total,
               "steps": args.steps, "callers": T, "all_ok": bool(ok), "records_ms": round(sum(last_ms[0]) if mode == "streamed" else r.ms, 3),
               "records_ms_calls": [round(x, 3) for x in last_ms[0]] if mode == "streamed" else None, "repaired_chunks": r.repaired_chunks, "batches": r.batches,
               "frames": frames, "records_read": r.records, "first_bad_reason": r.first_bad_reason,
               "first_bad_pos": None if r.first_bad_pos == 0xFFFFFFFFFFFFFFFF else r.first_bad_pos, "crc_ms": round(crc_ms, 3), "generated_in_s": round(gen_s, 1)}
        rows.append(row)
        emit(row)
    emit({"metric": "GiB/s of original bytes, record-batch validation " + " / ".join(r["mode"] for r in rows), "runs": [r["gibs"] for r in rows],
          "records_ms": [r["records_ms"] for r in rows if r["records"]], "crc_ms": crc_ms, "all_ok": all(r["all_ok"] for r in rows), "tsxform": N.version()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--callers", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="each round runs every level once; odd rounds in reverse order")
    ap.add_argument("--contents", default="K,B")
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--check", type=int, default=16, help="timed chunks per run checked against libzstd")
    ap.add_argument("--levels", default="1,2,3")
    ap.add_argument("--checksum", action="store_true", help="each level with and without TSX_ZSTD_CHECKSUM, alternating")
    ap.add_argument("--verify", action="store_true", help="each level without and with TSX_VERIFY, alternating")
    ap.add_argument("--verify-gcm", action="store_true", help="each level without and with TSX_VERIFY_GCM, alternating")
    ap.add_argument("--records", action="store_true", help="TSX_VALIDATE_RECORDS off / on / on / off on one valid segment of content B")
    ap.add_argument("--records-stream", action="store_true", help="the same segment: off / streamed in four calls of 64 chunks / one 256-chunk call / off")
    ap.add_argument("--records-frames", action="store_true", help="the same segment: TSX_VALIDATE_RECORDS alone / with TSX_VALIDATE_FRAMES / with it / alone")
    ap.add_argument("--device-profile", action="store_true", help="profile 1.5.7 level 3 / device / device / 1.5.7 in one process")
    ap.add_argument("--out", default=None, help="append every JSON line to this file as well")
    args = ap.parse_args()
    if args.device_profile and not args.out:
        args.out = os.path.join(ROOT, "profiles", "device_profile_level_bench.jsonl")
    if args.records_stream and not args.out:
        args.out = os.path.join(ROOT, "profiles", "records_stream_level_bench.jsonl")
    if args.records_frames and not args.out:
        args.out = os.path.join(ROOT, "profiles", "records_frames_level_bench.jsonl")
    if args.records and not args.out:
        args.out = os.path.join(ROOT, "profiles", "records_level_bench.jsonl")
    if args.verify_gcm and not args.out:
        args.out = os.path.join(ROOT, "profiles", "gcm_verify_level_bench.jsonl")

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.records or args.records_stream or args.records_frames:
        return records_bench(args, emit)
    import torch  # before libtsxform: one shared HIP runtime
    import tsxform
    from oracle import oracle as o
    from tsxform import synth
    nat = tsxform._native
    N = tsxform.get()
    dev = torch.device("cuda", 0)
    CH, cps = synth.CHUNK, 256
    n = args.segments * cps
    T = args.callers
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    levels = [(int(x), ck, vf, gv, nat.ZSTD_PROFILE_1_5_7) for x in args.levels.split(",") for ck in ((False, True) if args.checksum else (False,))
              for vf in ((False, True) if args.verify else (False,)) for gv in ((False, True) if args.verify_gcm else (False,))]
    if args.device_profile:
        exact, device = (3, False, False, False, nat.ZSTD_PROFILE_1_5_7), (0, False, False, False, nat.ZSTD_PROFILE_DEVICE)
        levels, args.rounds = [exact, device, device, exact], 1

    def libzstd_frame(raw, level, checksum):
        """libzstd's frame as oracle/zstd_ref.c makes it, with ZSTD_c_checksumFlag on request."""
        if not checksum:
            return o.zstd_compress_chunk(raw, level)
        Z = ctypes.CDLL(o.lib().orc_zstd_path().decode())
        Z.ZSTD_createCCtx.restype = ctypes.c_void_p; Z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
        Z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t; Z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        Z.ZSTD_CCtx_setPledgedSrcSize.restype = ctypes.c_size_t; Z.ZSTD_CCtx_setPledgedSrcSize.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong]
        Z.ZSTD_compress2.restype = ctypes.c_size_t; Z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        Z.ZSTD_compressBound.restype = ctypes.c_size_t; Z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        Z.ZSTD_isError.restype = ctypes.c_uint; Z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        a = np.frombuffer(raw, np.uint8)
        out = np.zeros(Z.ZSTD_compressBound(a.size), np.uint8)
        c = Z.ZSTD_createCCtx()
        Z.ZSTD_CCtx_setPledgedSrcSize(c, a.size)
        for prm, v in ((200, 1), (100, level), (201, 1)):
            Z.ZSTD_CCtx_setParameter(c, prm, v)
        r = Z.ZSTD_compress2(c, out.ctypes.data, out.size, a.ctypes.data, a.size)
        Z.ZSTD_freeCCtx(c)
        assert not Z.ZSTD_isError(r)
        return out[:r].tobytes()
    slot = (N.transformed_bound(CH, flags) + 63) // 64 * 64
    src = torch.empty(n * CH, dtype=torch.uint8, device=dev)
    dsts = [torch.empty(n * slot, dtype=torch.uint8, device=dev) for _ in range(T)]
    d = np.zeros(n, nat.DESC_DTYPE)
    d["src_off"] = np.arange(n, dtype=np.uint64) * CH; d["src_len"] = CH
    d["dst_off"] = np.arange(n, dtype=np.uint64) * slot; d["dst_cap"] = slot
    for i in range(n):
        d["iv"][i] = np.frombuffer(synth.iv_for(i // cps, i % cps), np.uint8)
    ctxs = [N.ctx_create(0, n, CH) for _ in range(T)]
    rows = []
    for content in args.contents.split(","):
        t_gen = time.perf_counter()
        if content == "K":
            for i in range(n):
                src[i * CH:(i + 1) * CH] = synth.gen_chunk("K", 1000 + i // cps, i // cps, i % cps, CH, device=dev)
            distinct = n

            def host_chunk(i):
                return src[i * CH:(i + 1) * CH].cpu().numpy()
        else:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            distinct = 64
            with ProcessPoolExecutor(16, mp_context=mp.get_context("spawn")) as ex:
                hb = list(ex.map(_gen_b_chunk, [(1000, 0, c, CH) for c in range(distinct)]))
            for i in range(n):
                src[i * CH:(i + 1) * CH] = torch.from_numpy(hb[i % distinct]).to(dev)

            def host_chunk(i, hb=hb):
                return hb[i % distinct]
        torch.cuda.synchronize()
        gen_s = time.perf_counter() - t_gen
        order = []
        for r in range(args.rounds):
            order += levels if r % 2 == 0 else levels[::-1]
        for level, ck, vf, gv, profile in order:
            p = nat.Native.make_params(flags | (nat.ZSTD_CHECKSUM if ck else 0) | (nat.VERIFY if vf else 0) | (nat.VERIFY_GCM if gv else 0), synth.KEY, synth.AAD, zstd_level=level,
                                       zstd_profile=profile)
            ds = [d.copy() for _ in range(T)]

            def step(t):
                N.transform_batch(p, ds[t], src.data_ptr(), dsts[t].data_ptr(), dsts[t].numel(), nat.MEM_DEVICE, ctx=ctxs[t])
            for w in range(max(args.warmup, 1)):
                for t in (range(T) if w == 0 else range(1)):
                    step(t)
            torch.cuda.synchronize()
            N.service_quiesce(0)
            s0 = N.service_stats(0)

            def worker(t):
                for _ in range(t, args.steps, T):
                    step(t)
            t0 = time.perf_counter()
            th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            [x.start() for x in th]
            [x.join() for x in th]
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            N.service_quiesce(0)
            s1 = N.service_stats(0)
            ok = all(bool((x["status"] == 0).all()) for x in ds) and all(bool((x["dst_len"] == ds[0]["dst_len"]).all()) for x in ds)
            rng = np.random.default_rng(level * 1000 + len(rows))
            sample = sorted(set(int(i) for i in rng.integers(0, n, args.check))) if content == "K" else list(range(min(args.check, distinct)))
            host = dsts[0]
            for i in sample:
                got = host[i * slot:i * slot + int(ds[0]["dst_len"][i])].cpu().numpy().tobytes()
                raw = np.ascontiguousarray(host_chunk(i)).tobytes()
                if profile == nat.ZSTD_PROFILE_DEVICE:                  # no library's bytes: libzstd has to restore the chunk from the frame
                    ok = ok and o.zstd_decompress_chunk(o.gcm_decrypt_chunk(synth.KEY, synth.AAD, got)) == raw
                    continue
                exp = o.gcm_encrypt_chunk(synth.KEY, ds[0]["iv"][i].tobytes(), synth.AAD, libzstd_frame(raw, level, ck))
                ok = ok and got == exp
            tm = N.ctx_timing(ctxs[0])
            row = {"content": content, "profile": "device" if profile == nat.ZSTD_PROFILE_DEVICE else "1.5.7", "level": level, "checksum": ck, "verify": vf, "verify_gcm": gv, "gcm_ms": round(tm.gcm_ms, 2), "gcm_launches": tm.gcm_launches, "unzstd_ms": round(tm.unzstd_ms, 2), "unzstd_launches": tm.unzstd_launches, "gibs": round(args.steps * n * CH / GiB / el, 3), "elapsed_s": round(el, 3),
                   "ratio": round(float(ds[0]["dst_len"].astype(np.int64).sum() - 28 * n) / (n * CH), 4),
                   "kernel_ms": round(s1["kernel_ms"] - s0["kernel_ms"], 1), "launches": s1["launches"] - s0["launches"],
                   "chunks": n, "distinct_chunks": distinct, "steps": args.steps, "callers": T,
                   "checked_chunks": len(sample), "exact_vs_libzstd": bool(ok), "generated_in_s": round(gen_s, 1)}
            if profile == nat.ZSTD_PROFILE_DEVICE:
                row["decoded_by_libzstd"] = row.pop("exact_vs_libzstd")
            rows.append(row)
            emit(row)
    if args.device_profile:
        by = {}
        for r in rows:
            by.setdefault("%s_%s" % (r["content"], r["profile"]), []).append(r)
        emit({"metric": "GiB/s of original bytes, profile 1.5.7 level 3 / device / device / 1.5.7 (runs in order)", "callers": T, "segments": args.segments,
              "runs": {k: [r["gibs"] for r in v] for k, v in by.items()}, "ratio": {k: v[0]["ratio"] for k, v in by.items()},
              "kernel_ms": {k: [r["kernel_ms"] for r in v] for k, v in by.items()},
              "all_ok": all(r.get("exact_vs_libzstd", r.get("decoded_by_libzstd")) for r in rows), "libzstd": o.zstd_version(), "tsxform": N.version()})
        return
    summary = {}
    for r in rows:
        k = "%s_L%d%s%s%s" % (r["content"], r["level"], "_checksum" if r["checksum"] else "", "_verify" if r["verify"] else "", "_verify_gcm" if r["verify_gcm"] else "")
        summary.setdefault(k, []).append(r["gibs"])
    emit({"metric": "GiB/s of original bytes per level (runs in order)", "runs": summary,
                      "ratio": {"%s_L%d%s%s%s" % (r["content"], r["level"], "_checksum" if r["checksum"] else "", "_verify" if r["verify"] else "", "_verify_gcm" if r["verify_gcm"] else ""): r["ratio"] for r in rows},
                      "all_exact": all(r["exact_vs_libzstd"] for r in rows), "libzstd": o.zstd_version(), "tsxform": N.version()})


if __name__ == "__main__":
    main()
