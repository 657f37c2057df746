#!/usr/bin/env python3
"""Fetch-side latency of the inverse chain (GCM verify + decrypt, Zstd frame decode, CRC32C) for small batches: 1 .. 256 chunks of
4 MiB, device resident and host -> host (registered buffers), with the block-parallel decoder form (csrc/zstd_dec_blocks.hip, the
default for batches of <= 256 chunks) and with the chunk-serial form alone (test hook dec_block_chunks = 0).  One JSON line per row.
  python tools/dec_latency.py [NMAX] [--checksum] [--forms blocks,chunks] [--chunks 1,2,4,8,16,64,256] [--mems device,host] [--lib libtsxform.so]
--checksum: every row twice, on frames with a content checksum (TSX_ZSTD_CHECKSUM: each fetch verifies it) and on the same chunks' frames
without, alternating; --lib: another build of the library (a parent tree's, for a side-by-side run in one call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tsxform  # noqa: E402
from tests import parity_cases as pc  # noqa: E402
from tsxform import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("nmax", nargs="?", type=int, default=256)
ap.add_argument("--checksum", action="store_true")
ap.add_argument("--forms", default="blocks,chunks")
ap.add_argument("--chunks", default="1,2,4,8,16,64,256")
ap.add_argument("--mems", default="device,host")
ap.add_argument("--lib", default="")
ap.add_argument("--iters", type=int, default=6)
args = ap.parse_args()
nat = tsxform._native
N = nat.Native(args.lib) if args.lib else nat.Native()
N.init(1, [0])
sys.path.insert(0, os.path.join(ROOT, "tools"))
from numa_bind import bind_to_gpu_numa_node
AFFINITY = bind_to_gpu_numa_node(0)                              # before any host buffer is allocated (profiles/r04_broker_numa.txt)
dev = torch.device("cuda", 0)
CH = synth.CHUNK
NMAX = args.nmax
flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
slot = (N.transformed_bound(CH, flags) + 63) // 64 * 64
params = nat.Native.make_params(flags, synth.KEY, synth.AAD)
src = torch.empty(NMAX * CH, dtype=torch.uint8, device=dev)
for i in range(NMAX):
    src[i * CH:(i + 1) * CH] = synth.gen_chunk("K", 1000, 0, i % 256, CH, device=dev)
kinds = [False, True] if args.checksum else [False]
d = np.zeros(NMAX, nat.DESC_DTYPE); d["src_off"] = np.arange(NMAX, dtype=np.uint64) * CH; d["src_len"] = CH
d["dst_off"] = np.arange(NMAX, dtype=np.uint64) * slot; d["dst_cap"] = slot
for i in range(NMAX):
    d["iv"][i] = np.frombuffer(synth.iv_for(0, i), np.uint8)
ctx = N.ctx_create(0, NMAX, CH)
mids, hmids, descs = {}, {}, {}
for ck in kinds:
    mids[ck] = torch.empty(NMAX * slot, dtype=torch.uint8, device=dev)
    descs[ck] = d.copy()
    pk = nat.Native.make_params(flags | (nat.ZSTD_CHECKSUM if ck else 0), synth.KEY, synth.AAD)
    N.transform_batch(pk, descs[ck], src.data_ptr(), mids[ck].data_ptr(), mids[ck].numel(), nat.MEM_DEVICE, ctx=ctx)
    assert (descs[ck]["status"] == 0).all()
    hmids[ck] = mids[ck].cpu().numpy()
    N.host_register(hmids[ck])
back = torch.empty(NMAX * CH, dtype=torch.uint8, device=dev)
hback = np.zeros(NMAX * CH, np.uint8)
N.host_register(hback)
for form in args.forms.split(","):
    N.debug_config("dec_block_chunks", 256 if form == "blocks" else 0)
    for n, ck in [(x, k) for x in (int(v) for v in args.chunks.split(",")) if x <= NMAX for k in kinds]:
        d, mid, hmid = descs[ck], mids[ck], hmids[ck]
        e = np.zeros(n, nat.DESC_DTYPE); e["src_off"] = d["dst_off"][:n]; e["src_len"] = d["dst_len"][:n]
        e["dst_off"] = np.arange(n, dtype=np.uint64) * CH; e["dst_cap"] = CH
        for mem in args.mems.split(","):
            ts = []
            for it in range(args.iters):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                if mem == "device":
                    N.detransform_batch(params, e, mid.data_ptr(), back.data_ptr(), back.numel(), nat.MEM_DEVICE, ctx=ctx)
                else:
                    N.detransform_batch(params, e, hmid, hback, hback.size, nat.MEM_HOST, ctx=ctx)
                ts.append(time.perf_counter() - t0)
            tm = N.ctx_timing(ctx)
            ok = bool((e["status"] == 0).all() and (e["crc32c"] == d["crc32c"][:n]).all())
            if mem == "device":
                ok = ok and bool(torch.equal(back[:n * CH], src[:n * CH]))
            else:
                ok = ok and bool(np.array_equal(hback[:n * CH], src[:n * CH].cpu().numpy()))
            taken = pc.blockmode_chunks(N, ctx, n)
            print(json.dumps({"form": form, "chunks": n, "mem": mem, "checksum": ck, "unzstd_launches": int(tm.unzstd_launches), "ms_median": round(float(np.median(ts[1:])) * 1e3, 3), "ms_min": round(min(ts[1:]) * 1e3, 3),
                              "gibs": round(n * CH / 2**30 / float(np.median(ts[1:])), 2), "unzstd_ms": round(tm.unzstd_ms, 3), "gcm_ms": round(tm.gcm_ms, 3),
                              "decoded_by_block_form": taken, "exact": ok}), flush=True)
