// The batch pipelines of libtsxform's front end (tsx_api.hip: lifecycle, contexts, entry points): one planning step, then the compressing
// forward chain as members of the compressor service (run_compress) or everything else as ordinary kernels (run_batch_inner), and the
// small kernels both queue.  Where the checks of an upload run, and when their codes reach the descriptors, is decided here; what they
// do is tsx_checks.hip's.  See include/tsxform.h for the contract.
#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "tsx_ctx.h"

#define TSX_SUB_BYTES ((size_t)64 << 20) /* input bytes per sub-batch: >= 1000 workgroups of the GCM / CRC kernels */
#define TSX_COMP_PIECES_MAX 8           /* members of one compressing host-memory batch (a completion counter + flag each) */

// buffers pinned through tsx_host_register: the only host ranges the device is KNOWN to address end to end (zero-copy output)
static std::mutex g_reg_mu;
static std::vector<std::pair<uintptr_t, size_t>> g_registered;
void registered_range_add(void* p, size_t bytes) { std::lock_guard<std::mutex> lk(g_reg_mu); g_registered.push_back({(uintptr_t)p, bytes}); }
void registered_range_remove(void* p) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (size_t i = 0; i < g_registered.size(); i++) if (g_registered[i].first == (uintptr_t)p) { g_registered.erase(g_registered.begin() + (long)i); break; }
}
void registered_range_forget_all() { std::lock_guard<std::mutex> lk(g_reg_mu); g_registered.clear(); }

// Can the device address ALL of [p, p + bytes)?  Zero-copy output lets the compressor waves write there; a buffer of which only a
// prefix is registered, or that spans two registrations, would fault the process (the broker's JVM) at the first byte behind the
// mapping.  Known extents only: a range inside ONE tsx_host_register'ed buffer, or inside one allocation the runtime reports
// (hipHostMalloc'ed memory); anything else takes the copy path.
static uint8_t* device_alias_of_range(void* p, size_t bytes) {
    if (!p || !bytes) return nullptr;
    bool inside = false;
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        for (const auto& r : g_registered) if ((uintptr_t)p >= r.first && (uintptr_t)p - r.first <= r.second && bytes <= r.second - ((uintptr_t)p - r.first)) { inside = true; break; }
    }
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || !dp) { (void)hipGetLastError(); return nullptr; }      // pageable memory
    if (inside) return (uint8_t*)dp;
#ifndef HIPEMU
    void* base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)dp) == hipSuccess && base && (uintptr_t)dp >= (uintptr_t)base &&
        bytes <= size - ((uintptr_t)dp - (uintptr_t)base)) return (uint8_t*)dp;
    (void)hipGetLastError();
#endif
    return nullptr;
}

// Waits for an event of a batch that is NOT the compressor's, with the safety net of svc_rotate.
hipError_t wait_event_watching(tsx_ctx* c, hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    bool asked = false;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        (void)hipGetLastError();
        const auto age = std::chrono::steady_clock::now() - t0;
        if (!asked && age > std::chrono::milliseconds(SVC_ROTATE_AFTER_MS)) { svc_rotate(c->dev); asked = true; }
        // A single-chunk fetch is 1.6 ms.  Only the first 200 us are polled without a sleep (a piece that is nearly done); after that the thread
        // sleeps between looks - 20 us while the batch is young (a sleep's real granularity is ~60 us: + <= 4 % on a single-chunk fetch), 50 us up
        // to 20 ms, 500 us beyond.  Every ChunkCache worker (ForkJoinPool, parallelism = #cores by default) waits in here: round 5 spun for 3 ms,
        // i.e. a whole core per fetch in flight.
        if (age > std::chrono::microseconds(200))
            std::this_thread::sleep_for(std::chrono::microseconds(age > std::chrono::milliseconds(20) ? 500 : age > std::chrono::milliseconds(3) ? 50 : 20));
    }
}

float ev_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; hipEventElapsedTime(&ms, a, b); return ms; }

// ---- small glue kernels ---------------------------------------------------------------------------
// Builds the GCM work items of a batch from the descriptors (and, after compression, the frame sizes),
// checks slot capacities and initialises status / dst_len.  mode 0 = transform, 1 = detransform.
__global__ void plan_gcm_kernel(tsx_chunk_desc* __restrict__ descs, uint32_t n, const uint32_t* __restrict__ zlen, uint64_t mid_stride,
                                int have_mid, int mode, int mid_is_out, tsx_gcm_chunk* __restrict__ g, int32_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tsx_chunk_desc d = descs[i];
    tsx_gcm_chunk c;
    int32_t st = status[i];
    if (mode == 0) {
        uint32_t len = have_mid ? zlen[i] : d.src_len;
        c.in_off = have_mid ? (uint64_t)i * mid_stride : d.src_off;
        c.out_off = d.dst_off;
        c.len = len;
        for (int k = 0; k < 12; k++) c.iv[k] = d.iv[k];
        if (st == TSX_OK && (uint64_t)len + 28 > d.dst_cap) st = TSX_E_DST_TOO_SMALL;
        descs[i].dst_len = st == TSX_OK ? len + 28 : 0;
    } else {
        c.in_off = d.src_off;
        c.out_off = mid_is_out ? (uint64_t)i * mid_stride : d.dst_off;
        c.len = d.src_len >= 28 ? d.src_len - 28 : 0;
        for (int k = 0; k < 12; k++) c.iv[k] = 0;
        if (st == TSX_OK && d.src_len < 28) st = TSX_E_SHORT_CHUNK;
        if (st == TSX_OK && !mid_is_out && c.len > d.dst_cap) st = TSX_E_DST_TOO_SMALL;
        if (!mid_is_out) descs[i].dst_len = st == TSX_OK ? c.len : 0;
    }
    c.skip = st != TSX_OK;
    status[i] = st;
    g[i] = c;
}

// dst slot <- src span, 16 B per lane when both sides are 16-byte aligned (chunk offsets must be).
// from_mid: source is the compressed-frame staging buffer with per-chunk length zlen[i].
__global__ __launch_bounds__(256) void copy_chunks_kernel(tsx_chunk_desc* __restrict__ descs, const uint32_t* __restrict__ zlen,
                                                          uint64_t mid_stride, int from_mid, const uint8_t* __restrict__ src,
                                                          uint8_t* __restrict__ dst, int32_t* __restrict__ status, uint32_t blocks_per_chunk) {
    const uint32_t i = blockIdx.x / blocks_per_chunk, part = blockIdx.x % blocks_per_chunk;
    const tsx_chunk_desc d = descs[i];
    if (status[i] != TSX_OK) return;
    const uint32_t len = from_mid ? zlen[i] : d.src_len;
    if (len > d.dst_cap) {
        if (part == 0 && threadIdx.x == 0) { status[i] = TSX_E_DST_TOO_SMALL; descs[i].dst_len = 0; }
        return;
    }
    const uint8_t* s = src + (from_mid ? (uint64_t)i * mid_stride : d.src_off);
    uint8_t* o = dst + d.dst_off;
    const uint32_t q = len >> 4;
    for (uint32_t p = part * 256 + threadIdx.x; p < q; p += blocks_per_chunk * 256)
        reinterpret_cast<uint4*>(o)[p] = reinterpret_cast<const uint4*>(s)[p];
    if (part == 0) {
        for (uint32_t b = (q << 4) + threadIdx.x; b < len; b += 256) o[b] = s[b];
        if (threadIdx.x == 0) descs[i].dst_len = len;
    }
}

// First kernel of a batch of ordinary kernels (fetches above all).  A copy of 48 bytes, or of the 21 KB key schedule, is a blit KERNEL of
// the runtime (__amd_rocclr_copyBuffer, 512-thread workgroups): every fetch used to queue five of them (descriptors up, key schedule up,
// descriptors down, two wipes), and they were the kernels that got stuck next to the compressor service (all six stuck dispatches of
// profiles/r05_kernel_trace_blocked_fetch.csv.gz are copyBuffer kernels; next to guest waves such a copy waits for the launch to end).
// So nothing small is copied any more: this kernel reads the batch's descriptors - and, for the first piece of an encrypted batch, the key
// schedule the host built - straight from the context's pinned memory into their device-side places and starts every status from
// TSX_OK; publish_status_kernel / crc32c_final_kernel write the results back there; wipe_key_kernel clears the key material.
__global__ __launch_bounds__(256) void begin_batch_kernel(const tsx_chunk_desc* __restrict__ hd_descs, tsx_chunk_desc* __restrict__ descs, int32_t* __restrict__ status,
                                                          uint32_t n, const uint4* __restrict__ hd_key, uint4* __restrict__ d_key, uint32_t key_words16) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint4* s = reinterpret_cast<const uint4*>(hd_descs + i);
        uint4* d = reinterpret_cast<uint4*>(descs + i);
        const uint4 a = s[0], b = s[1], c = s[2];
        d[0] = a; d[1] = b; d[2] = c;
        status[i] = TSX_OK;
    }
    if (hd_key) for (uint32_t k = i; k < key_words16; k += gridDim.x * blockDim.x) d_key[k] = hd_key[k];
}
static_assert(sizeof(tsx_chunk_desc) == 48 && sizeof(tsx_gcm_key) % 16 == 0, "begin_batch_kernel moves descriptors and the key schedule as 16-byte words");

// Last kernel of an encrypted batch: the key schedule and the raw key bytes do not stay behind in the context
__global__ __launch_bounds__(256) void wipe_key_kernel(uint4* __restrict__ d_key, uint32_t key_words16, uint4* __restrict__ d_keyraw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint4 z; z.x = z.y = z.z = z.w = 0;
    for (uint32_t k = i; k < key_words16; k += gridDim.x * blockDim.x) d_key[k] = z;
    if (i < 8) d_keyraw[i] = z;
}
void launch_wipe_key(tsx_ctx* c, hipStream_t st) {
    hipLaunchKernelGGL(wipe_key_kernel, dim3(6), dim3(256), 0, st, (uint4*)c->d_key, (uint32_t)(sizeof(tsx_gcm_key) / 16), (uint4*)c->d_keyraw);
}

__global__ void init_status_kernel(int32_t* status, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) status[i] = TSX_OK;
}

// mirror != nullptr: the whole descriptor as it stands goes to the batch's pinned copy as well (what the caller gets back; a CRC stage that
// runs afterwards adds its word there itself)
__global__ void publish_status_kernel(tsx_chunk_desc* descs, const int32_t* status, uint32_t n, tsx_chunk_desc* mirror) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    descs[i].status = status[i];
    if (status[i] != TSX_OK) descs[i].dst_len = 0;
    if (mirror) {
        const uint4* s = reinterpret_cast<const uint4*>(descs + i);
        uint4* d = reinterpret_cast<uint4*>(mirror + i);
        const uint4 a = s[0], b = s[1], c = s[2];
        d[0] = a; d[1] = b; d[2] = c;
    }
}

// Zeroes what a failed chunk of the inverse chain left in its output slot (device-memory calls: a forged chunk's
// unauthenticated plaintext must not stay readable - JCE's doFinal releases nothing on a bad tag,
// DecryptionChunkEnumeration.java:54-62).  Up to min(dst_cap, src_len) bytes can have been written.
__global__ __launch_bounds__(256) void scrub_failed_kernel(const tsx_chunk_desc* __restrict__ descs, const int32_t* __restrict__ status,
                                                           uint8_t* __restrict__ dst, uint32_t blocks_per_chunk) {
    const uint32_t i = blockIdx.x / blocks_per_chunk, part = blockIdx.x % blocks_per_chunk;
    if (status[i] == TSX_OK) return;
    const tsx_chunk_desc d = descs[i];
    const uint32_t len = d.src_len < d.dst_cap ? d.src_len : d.dst_cap;
    uint8_t* o = dst + d.dst_off;
    const uint32_t q = len >> 4;                                         // slots are 16-byte aligned
    uint4 z; z.x = z.y = z.z = z.w = 0;
    for (uint32_t p = part * 256 + threadIdx.x; p < q; p += blocks_per_chunk * 256) reinterpret_cast<uint4*>(o)[p] = z;
    if (part == 0) for (uint32_t b = (q << 4) + threadIdx.x; b < len; b += 256) o[b] = 0;
}

// ---- the launches more than one path queues ------------------------------------------------------------------------------------------
// Chunks [lo, lo + n) of the batch; all on stream st.  A chunk above 1 MiB is cut over 16 workgroups.
static uint32_t blocks_per_chunk(const tsx_run& r) { return r.max_len > (1u << 20) ? 16 : 1; }

static void launch_copy_chunks(const tsx_run& r, hipStream_t st, uint32_t lo, uint32_t n, int from_mid, const uint8_t* src) {
    tsx_ctx* c = r.c;
    const uint32_t bpc = blocks_per_chunk(r);
    hipLaunchKernelGGL(copy_chunks_kernel, dim3(n * bpc), dim3(256), 0, st, c->d_descs + lo, (const uint32_t*)(c->d_zlen + lo), (uint64_t)c->mid_stride, from_mid, src, r.d_dst, c->d_status + lo, bpc);
}

static void launch_scrub_failed(const tsx_run& r, hipStream_t st, uint32_t lo, uint32_t n) {
    tsx_ctx* c = r.c;
    const uint32_t bpc = blocks_per_chunk(r);
    hipLaunchKernelGGL(scrub_failed_kernel, dim3(n * bpc), dim3(256), 0, st, (const tsx_chunk_desc*)(c->d_descs + lo), (const int32_t*)(c->d_status + lo), r.d_dst, bpc);
}

// The GCM stage: its work items from the descriptors (plan_gcm_kernel), then the kernels.  mode 0 = encrypt, 1 = decrypt; have_mid: the input
// is the frames of the staging buffer (sizes in d_zlen); mid_is_out: the output goes there.  max_len: the longest input of a chunk.
static void launch_gcm_stage(const tsx_run& r, hipStream_t st, uint32_t lo, uint32_t n, int have_mid, int mode, int mid_is_out, uint32_t max_len,
                             const uint8_t* in, uint8_t* out) {
    tsx_ctx* c = r.c;
    hipLaunchKernelGGL(plan_gcm_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c->d_descs + lo, n, (const uint32_t*)(c->d_zlen + lo), (uint64_t)c->mid_stride, have_mid, mode, mid_is_out,
                       c->d_gchunks + lo, c->d_status + lo);
    tsx_launch_gcm(st, c->dev->d_aes, c->d_key, c->d_gchunks + lo, n, max_len, in, out, c->d_partials + (size_t)lo * c->partials_per_chunk, c->d_status + lo, mode);
    c->timing.gcm_launches += 2;
}

// ---- batch drivers ---------------------------------------------------------------------------------
static int validate(const tsx_chunk_desc* descs, uint32_t n, size_t src_size, size_t dst_size, bool need_dst, uint32_t* max_len, uint32_t* max_out,
                    size_t* in_bytes, bool* monotonic) {
    *max_len = 0; *max_out = 0; *in_bytes = 0; *monotonic = true;
    uint64_t prev_src_end = 0, prev_dst_end = 0;
    for (uint32_t i = 0; i < n; i++) {
        const tsx_chunk_desc& d = descs[i];
        if ((d.src_off & 15) || (need_dst && (d.dst_off & 15))) return TSX_E_INVAL;       // 16-byte aligned slots
        if (need_dst && (d.dst_off > dst_size || d.dst_cap > dst_size - d.dst_off)) return TSX_E_INVAL;   // no wrap-around
        if (d.src_len >= (1u << 30) + 4096) return TSX_E_INVAL;                             // chunk.size <= 2^30 - 1 (RemoteStorageManagerConfig.java:122-130)
        if (d.src_off > src_size || d.src_len > src_size - d.src_off) return TSX_E_INVAL;    // inside the caller's source buffer, no wrap-around
        if (d.src_len > *max_len) *max_len = d.src_len;
        if (need_dst && d.dst_cap > *max_out) *max_out = d.dst_cap;
        if (d.src_off + d.src_len > *in_bytes) *in_bytes = d.src_off + d.src_len;
        if (d.src_off < prev_src_end || (need_dst && d.dst_off < prev_dst_end)) *monotonic = false;
        prev_src_end = d.src_off + d.src_len;
        if (need_dst) prev_dst_end = d.dst_off + d.dst_cap;
    }
    return TSX_OK;
}

// test hook `trace`: where a batch spends its time, as seen from the calling thread (microseconds since the first mark of the call)
struct tsx_trace {
    std::chrono::steady_clock::time_point t0; bool on;
    tsx_trace() : t0(std::chrono::steady_clock::now()), on(g_cfg.trace) {}
    void mark(const char* what) const { if (on) fprintf(stderr, "[tsx trace %p] %9.0f us  %s\n", (const void*)this, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what); }
};

// ---- the planning step: what both pipelines do first ----------------------------------------------------------------------------------
// Validates (a call that fails with TSX_E_INVAL has touched nothing of the caller's descriptors), lays the bound-sized slots of a packed
// batch out, decides whether the output is written straight into the caller's buffer (zero_copy_ok: the pipeline's own condition; then
// the device must be able to address ALL of the buffer), reserves the workspace and says where the kernels read and write.
struct tsx_plan { size_t in_bytes, out_bytes; bool monotonic; };      // input bytes spanned; size of the output area the kernels see; chunks in order

static int plan_batch(tsx_run& r, bool (*zero_copy_ok)(const tsx_run&, size_t out_bytes), tsx_plan* pl) {
    tsx_ctx* c = r.c;
    uint32_t max_len, max_out;
    int rc = validate(r.descs, r.n, r.src_size, r.dst_size, r.mode != 2 && !r.packed, &max_len, &max_out, &pl->in_bytes, &pl->monotonic);
    if (rc) return rc;
    pl->out_bytes = r.dst_size;
    if (r.packed) {
        // the kernels still write one bound-sized slot per chunk; only the bytes produced end up, back to back, in the caller's buffer
        const size_t slot = (tsx_transformed_bound(max_len, r.flags) + 63) & ~(size_t)63;
        if (slot >= ((size_t)1 << 32)) return TSX_E_INVAL;
        for (uint32_t i = 0; i < r.n; i++) { r.descs[i].dst_off = (uint64_t)i * slot; r.descs[i].dst_cap = (uint32_t)slot; }
        pl->out_bytes = (size_t)r.n * slot; max_out = (uint32_t)slot;
    }
    r.max_len = max_len; r.max_out = max_out;
    r.zc_dst = zero_copy_ok(r, pl->out_bytes) ? device_alias_of_range(r.dst, r.packed ? pl->out_bytes : r.dst_size) : nullptr;
    c->last_zero_copy = r.zc_dst != nullptr;
    // (the CRC of restored bytes runs over dst_cap-sized slots: only the inverse chain sizes its partial sums by max_out)
    rc = reserve_or_drain(c, r.n, max_len, r.mode == 1 ? max_out : 0, r.flags, r.host, pl->in_bytes, r.zc_dst ? 0 : pl->out_bytes);
    if (rc) return rc;
    r.d_src = r.host ? c->d_in : (const uint8_t*)r.src;
    r.d_dst = r.zc_dst ? r.zc_dst : r.host ? c->d_out : (uint8_t*)r.dst;
    return TSX_OK;
}

// ---- the one place that packs ---------------------------------------------------------------------------------------------------------
// Chunks [sb.lo, sb.lo + sb.n) of a packed batch, whose descriptors still name their bound-sized slots: every chunk gets its final
// dst_off (the sum of the dst_len in front of it), a chunk that is not TSX_OK takes no room (dst_len = 0), and one that no longer fits
// the caller's buffer - and every chunk behind it - is TSX_E_DST_TOO_SMALL.  move(to, slot_off, len) brings a chunk's bytes from its slot
// to offset `to` of the caller's buffer.
template <class Mover>
static int pack_chunks(const tsx_run& r, const tsx_sub& sb, size_t* packed_at, bool* packed_full, Mover move) {
    for (uint32_t i = sb.lo; i < sb.lo + sb.n; i++) {
        tsx_chunk_desc& d = r.descs[i];
        const size_t slot_off = d.dst_off;
        d.dst_off = *packed_at;
        if (d.status != TSX_OK) { d.dst_len = 0; continue; }
        if (*packed_full || *packed_at + d.dst_len > r.dst_size) { *packed_full = true; d.status = TSX_E_DST_TOO_SMALL; d.dst_len = 0; continue; }
        if (d.dst_len) { const int rc = move(*packed_at, slot_off, d.dst_len); if (rc) return rc; }
        *packed_at += d.dst_len;
    }
    return TSX_OK;
}

// The bytes chunks [lo, lo + n) produced travel back on out_st (host-memory batches; their descriptors are on the host already).
// Exactly dst_len bytes per chunk: a slot's slack may hold bytes of an earlier batch on this (possibly pooled) context.
static int copy_back(const tsx_run& r, const tsx_sub& sb, size_t* packed_at, bool* packed_full, hipStream_t out_st) {
    tsx_ctx* c = r.c;
    if (r.packed) return pack_chunks(r, sb, packed_at, packed_full, [&](size_t to, size_t slot_off, size_t len) -> int {
        // packed output lands at any byte of the caller's buffer.  The copy engines move a D2H copy of ODD size to an ODD host
        // address at 12 GB/s instead of 31 (110 us instead of 42 per 1.3 MB chunk, profiles/r03_copy_engine_probe.txt; every
        // other combination of size and address is fast): such a copy goes as its 64-byte multiple + the last < 64 bytes.
        uint8_t* const hp = (uint8_t*)r.dst + to;
        const size_t tail = (((uintptr_t)hp & 1) && (len & 1) && len > 4096) ? (len & 63) : 0;
        HIPCHK(hipMemcpyAsync(hp, c->d_out + slot_off, len - tail, hipMemcpyDeviceToHost, out_st));
        if (tail) HIPCHK(hipMemcpyAsync(hp + (len - tail), c->d_out + slot_off + (len - tail), tail, hipMemcpyDeviceToHost, out_st));
        return TSX_OK;
    });
    // slot layout: neighbours that produced back-to-back bytes (restored chunks fill their slots: the usual fetch) travel as ONE copy
    size_t run_at = 0, run_len = 0;
    for (uint32_t i = sb.lo; i < sb.lo + sb.n; i++) {
        const tsx_chunk_desc& d = r.descs[i];
        if (d.status != TSX_OK || d.dst_len == 0) continue;
        if (run_len && d.dst_off == run_at + run_len) { run_len += d.dst_len; continue; }
        if (run_len) HIPCHK(hipMemcpyAsync((uint8_t*)r.dst + run_at, c->d_out + run_at, run_len, hipMemcpyDeviceToHost, out_st));
        run_at = d.dst_off; run_len = d.dst_len;
    }
    if (run_len) HIPCHK(hipMemcpyAsync((uint8_t*)r.dst + run_at, c->d_out + run_at, run_len, hipMemcpyDeviceToHost, out_st));
    return TSX_OK;
}

// ---- the compressing forward chain: members of the device's service ---------------------------------------------------------------------
// Zero-copy output (round 4).  The wave that finishes a chunk writes its bytes straight into the caller's buffer over PCIe when the device
// can address ALL of it (device_alias_of_range): posted writes of a few ms of a second-long wave, released to system scope before the
// chunk is counted done.  No device output buffer, no copy-out phase: with 32-48 callers a segment's 256 output copies stood 0.3-1.0 s
// in the copy engine's queue behind the other callers' (profiles/r04_broker_shape_experiments.txt).  Slot layout (TSX_MEM_HOST, what
// GpuTransformChunkEnumeration.java issues): nothing is left to do on the host.  Packed layout: pooled contexts (256-chunk segments) let
// the waves fill bound-sized slots in the caller's buffer when it has room for them and pack them down in place; an explicit context's
// 2048-chunk batch would spend ~90 ms of one host thread on that behind the kernel - it keeps the copy path, which packs piece by piece
// while later pieces run (test hook zero_copy_packed takes it anyway).
static bool compress_zero_copy_ok(const tsx_run& r, size_t out_bytes) {
    return r.host && r.fuse_stages && !g_cfg.no_zero_copy_out && (!r.packed || (r.dst_size >= out_bytes && (r.pooled || g_cfg.zero_copy_packed)));
}

// Test hook stages_separate: CRC, compressor, GCM (or the copy into the slots) as separate launches around the service's members, the
// statuses in d_status.  Three steps of run_compress, each a failure of which leaves through its abandon_all.
// ... in front of the input copies: the descriptors go up, every status starts from TSX_OK
static int separate_begin(const tsx_run& r) {
    tsx_ctx* c = r.c;
    HIPCHK(hipMemcpyAsync(c->d_descs, c->h_descs, (size_t)r.n * sizeof(tsx_chunk_desc), hipMemcpyHostToDevice, c->st));
    hipLaunchKernelGGL(init_status_kernel, dim3((r.n + 255) / 256), dim3(256), 0, c->st, c->d_status, r.n);
    return TSX_OK;
}
// ... a piece's input has landed: its CRC, finished before the piece is published
static int separate_crc(const tsx_run& r, const tsx_sub& sb) {
    tsx_ctx* c = r.c;
    if ((r.flags & TSX_CRC)) { tsx_launch_crc32c(c->st, c->dev->d_crc, r.d_src, c->d_descs + sb.lo, sb.n, r.max_len, c->d_partials + (size_t)sb.lo * c->partials_per_chunk, 0); c->timing.crc_launches += 2; }
    return hipStreamSynchronize(c->st) != hipSuccess ? TSX_E_DEVICE : TSX_OK;
}
// ... a piece's member has completed (and been verified): its frames are in the staging buffer; GCM (or the copy into the slots), the
// status publication and the descriptors' way back to the pinned mirror follow.  upload_key: the first piece brings the key schedule.
static int separate_finish(const tsx_run& r, const tsx_sub& sb, bool upload_key) {
    tsx_ctx* c = r.c;
    tsx_chunk_desc* dd = c->d_descs + sb.lo;
    uint8_t* dmid = c->d_mid + (size_t)sb.lo * c->mid_stride;
    if (r.enc) {
        if (upload_key) {
            tsx_gcm_key_build_host(r.params->key, r.params->aad, r.params->aad_len, c->h_key);
            HIPCHK(hipMemcpyAsync(c->d_key, c->h_key, sizeof(tsx_gcm_key), hipMemcpyHostToDevice, c->st));
        }
        launch_gcm_stage(r, c->st, sb.lo, sb.n, 1, 0, 0, (uint32_t)tsx_transformed_bound(r.max_len, TSX_COMPRESS), dmid, r.d_dst);
    } else launch_copy_chunks(r, c->st, sb.lo, sb.n, 1, dmid);
    hipLaunchKernelGGL(publish_status_kernel, dim3((sb.n + 255) / 256), dim3(256), 0, c->st, dd, (const int32_t*)(c->d_status + sb.lo), sb.n, (tsx_chunk_desc*)nullptr);
    HIPCHK(hipMemcpyAsync(c->h_descs + sb.lo, dd, (size_t)sb.n * sizeof(tsx_chunk_desc), hipMemcpyDeviceToHost, c->st));
    return hipStreamSynchronize(c->st) != hipSuccess ? TSX_E_DEVICE : TSX_OK;
}

// Any compressing batch - explicit context or pooled, device or host memory - takes this way.  The batch is cut into at most comp_pieces
// members when its input comes from host memory (piece k + 1's input copy overlaps piece k's waves; a member is published when ITS input
// has landed: what is in the queue is runnable), otherwise it is one member (several beyond TSX_SVC_MEMBER_MAX chunks).  The waves run the
// whole chain of a chunk and own its descriptor in the context's pinned mirror: nothing but tickets goes to the device - no descriptor
// upload, no status kernels, no key upload (a small copy or kernel queued next to second-long waves waits for them: measured in rounds 3-4).
// In order: plan, cut the pieces, stage descriptors and key, queue the input copies, submit, then per piece wait / verify / hand back.
static int run_compress(tsx_run& r) {
    tsx_ctx* c = r.c;
    tsx_device* dev = c->dev;
    const uint32_t n = r.n;
    tsx_plan pl;
    int rc = plan_batch(r, compress_zero_copy_ok, &pl);
    if (rc) return rc;
    const bool monotonic = pl.monotonic;
    memset(&c->timing, 0, sizeof c->timing);
    tsx_timing& t = c->timing;
    c->verify_block_form = 0; c->verify_fallback = 0;
    // per chunk, what a check has to say (0: nothing; tsx_checks.hip): the two verifiers' of a piece, one after the other; the record
    // validator's of the whole batch
    const bool zverify = r.flags & TSX_VERIFY, gverify = r.flags & TSX_VERIFY_GCM, records = r.flags & TSX_VALIDATE_RECORDS;
    std::vector<int32_t> vcode(zverify || gverify ? n : 0, 0), rcode(records ? n : 0, 0);
    // ---- the pieces ----
    std::vector<tsx_sub> subs;
    {
        uint32_t pieces = 1;
        if (r.host && monotonic && !g_cfg.no_pipeline) { pieces = g_cfg.comp_pieces < 1 ? 1 : g_cfg.comp_pieces > TSX_COMP_PIECES_MAX ? TSX_COMP_PIECES_MAX : g_cfg.comp_pieces; if (n < 8 * pieces && !g_cfg.sub_bytes) pieces = n >= 16 ? 2 : 1; }
        uint32_t per = (n + pieces - 1) / pieces;
        if (per > TSX_SVC_MEMBER_MAX) per = TSX_SVC_MEMBER_MAX;
        if ((n + per - 1) / per > TSX_COMP_PIECES_MAX) return TSX_E_INVAL;                // (> 131072 chunks in one call)
        for (uint32_t lo = 0; lo < n; lo += per) {
            const uint32_t cnt = n - lo < per ? n - lo : per;
            size_t a = r.descs[lo].src_off, b = a;
            if (monotonic) b = (size_t)(r.descs[lo + cnt - 1].src_off + r.descs[lo + cnt - 1].src_len);
            else { a = 0; b = pl.in_bytes; }
            subs.push_back({lo, cnt, a, b});
        }
    }
    const size_t ns = subs.size();
    c->last_members = (uint32_t)ns;
    for (size_t k = 1; k < ns; k++) for (auto& e : c->sub_ev[k]) if (!e) HIPCHK(hipEventCreate(&e));
    // ---- descriptors and key schedule, where the waves read and write them: the context's pinned memory ----
    memcpy(c->h_descs, r.descs, (size_t)n * sizeof(tsx_chunk_desc));
    const bool self_status = r.fuse_stages;
    if (self_status) for (uint32_t i = 0; i < n; i++) { c->h_descs[i].status = TSX_E_DEVICE; c->h_descs[i].dst_len = 0; }   // the waves own them from here: a
                                                                        // stale TSX_OK the caller handed in must not survive a chunk that never ran
    if (r.enc && r.fuse_stages) tsx_gcm_key_build_host(r.params->key, r.params->aad, r.params->aad_len, c->h_key);
    hipStream_t cin = r.pooled ? dev->copy_in : c->st_in, cout_ = r.pooled ? dev->copy_out : c->st_out;
    const auto t_begin = std::chrono::steady_clock::now();
    uint64_t ids[TSX_COMP_PIECES_MAX] = {0};
    size_t submitted = 0;
    auto abandon_all = [&](int code) {
        // nothing of this call may still be running when it returns with an error: members that were published are taken back (their
        // tickets become stale) only once the service kernel is gone; copies that were queued (they read the caller's source) have drained
        if (submitted) { svc_pause(dev); for (size_t k = 0; k < submitted; k++) if (ids[k]) svc_retire(dev, ids[k], true); svc_resume(dev);
                         (void)hipMemcpy(c->d_segdone, dev->h_zeros, 64, hipMemcpyHostToDevice); memset(c->h_segflag, 0, 64); }
        (void)hipGetLastError();
        if (r.host) { (void)hipStreamSynchronize(cin); (void)hipStreamSynchronize(cout_); }
        (void)hipStreamSynchronize(c->st);
        return code;
    };
    // every HIP failure from the first queued copy on leaves through abandon_all (a bare return would leave copies of the caller's buffer,
    // or published members that read a key about to be wiped, in flight)
#define HIPCHK_AB(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { tsx_set_err(#x, e_); return abandon_all(TSX_E_DEVICE); } } while (0)
    if (!self_status && (rc = separate_begin(r))) return abandon_all(rc);
    // ---- input copies, all queued at once; every piece is published when its own bytes are on the device ----
    if (r.host) {
        HIPCHK_AB(hipEventRecord(c->ev[EV_H2D_FIRST], cin));
        for (size_t k = 0; k < ns; k++) {
            const tsx_sub& sb = subs[k];
            if ((k == 0 || monotonic) && sb.in_hi > sb.in_lo) HIPCHK_AB(hipMemcpyAsync(c->d_in + sb.in_lo, (const uint8_t*)r.src + sb.in_lo, sb.in_hi - sb.in_lo, hipMemcpyHostToDevice, cin));
            HIPCHK_AB(hipEventRecord(c->sub_ev[k][SUB_STAGED_IN], cin));
        }
    }
    for (size_t k = 0; k < ns; k++) {
        const tsx_sub& sb = subs[k];
        if (r.host && hipEventSynchronize(c->sub_ev[k][SUB_STAGED_IN]) != hipSuccess) return abandon_all(TSX_E_DEVICE);
        if (k == 0) t.h2d_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        if (!self_status && (rc = separate_crc(r, sb))) return abandon_all(rc);
        tsx_zseg m; memset(&m, 0, sizeof m);
        m.n = sb.n; m.profile = r.params->zstd_profile; m.level = (r.params->zstd_level == 1 || r.params->zstd_level == 2) ? (uint32_t)r.params->zstd_level : 3u;
        if (r.flags & TSX_ZSTD_CHECKSUM) m.level |= TSX_ZSEG_CHECKSUM;
        m.src_base = r.d_src; m.descs = (self_status ? c->hd_descs : c->d_descs) + sb.lo; m.mid = c->d_mid + (size_t)sb.lo * c->mid_stride; m.mid_stride = c->mid_stride;
        m.zlen = c->d_zlen + sb.lo; m.status = c->d_status + sb.lo; m.work = (uint8_t*)c->d_zwork + (size_t)sb.lo * tsx_zstd_workspace_bytes(1, 0);
        if (self_status) {
            m.fuse.crc = (r.flags & TSX_CRC) ? dev->d_crc : nullptr;
            m.fuse.out = r.d_dst; m.fuse.self_status = 1;
            if (r.enc) { m.fuse.aes = dev->d_aes; m.fuse.key = c->hd_key; m.fuse.key_on_host = 1; }
        }
        __atomic_store_n(&c->h_segflag[k], 0u, __ATOMIC_RELEASE);
        m.done = c->d_segdone + k; m.flag = c->hd_segflag + k;
        rc = svc_submit(dev, m, &c->h_segflag[k], &ids[k]);
        if (rc == TSX_E_INVAL) return abandon_all(rc);
        submitted = k + 1;
        if (rc) return abandon_all(rc);
    }
    // ---- record-batch validation: every piece's input has landed (the last piece was published when its own had); the validator's two
    // kernels run while the service compresses, and their verdicts are in hand before the first piece is handed back ----
    if (records && (rc = records_validate(r, r.host ? c->sub_ev[ns - 1][SUB_STAGED_IN] : nullptr, rcode.data()))) return abandon_all(rc);
    // ---- completions, in order; a piece's bytes travel back (or are packed down) while the later pieces still run ----
    size_t packed_at = 0; bool packed_full = false;
    const auto t_pub = std::chrono::steady_clock::now();
    for (size_t k = 0; k < ns; k++) {
        const tsx_sub& sb = subs[k];
        if ((rc = svc_wait(dev, &c->h_segflag[k]))) return abandon_all(rc);
        svc_retire(dev, ids[k], false);
        ids[k] = 0;
        if (k + 1 == ns) t.zstd_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_pub).count();
        // verify on upload: the piece's frames and their source chunks are both still on the device; the later pieces keep compressing.
        // Its codes are applied behind separate_finish, which overwrites h_descs
        if (zverify && (rc = verify_piece(r, sb, self_status, vcode.data()))) return abandon_all(rc);
        if (!self_status && (rc = separate_finish(r, sb, k == 0))) return abandon_all(rc);
        if (zverify) check_apply(c->h_descs, vcode.data(), sb.lo, sb.n);
        // verify on upload, GCM stage: the piece's delivered bytes, before its descriptors reach the caller and before copy_back / pack_chunks
        // move them (chunks the Zstandard verifier has just failed are skipped; without the flag only its test hook acts)
        if (r.enc && (rc = gcm_verify_piece(r, sb, vcode.data()))) return abandon_all(rc);
        if (gverify) check_apply(c->h_descs, vcode.data(), sb.lo, sb.n);
        if (records) check_apply(c->h_descs, rcode.data(), sb.lo, sb.n);
        memcpy(r.descs + sb.lo, c->h_descs + sb.lo, (size_t)sb.n * sizeof(tsx_chunk_desc));
        if (r.zc_dst) {
            // the bytes are where they belong; a packed batch is packed down in place.  (compress_zero_copy_ok: dst_size >= out_bytes, the
            // room of every slot - a chunk moves towards the front only and packed_full stays false)
            if (r.packed) (void)pack_chunks(r, sb, &packed_at, &packed_full, [&](size_t to, size_t slot_off, size_t len) -> int {
                if (slot_off != to) memmove((uint8_t*)r.dst + to, (const uint8_t*)r.dst + slot_off, len);
                return TSX_OK;
            });
        } else if (r.host) {
            if ((rc = copy_back(r, sb, &packed_at, &packed_full, cout_))) return abandon_all(rc);
        }
    }
    const auto t_done = std::chrono::steady_clock::now();
    if (r.host && !r.zc_dst) { HIPCHK_AB(hipEventRecord(c->ev[EV_D2H_LAST], cout_)); HIPCHK_AB(hipEventSynchronize(c->ev[EV_D2H_LAST])); }
#undef HIPCHK_AB
    t.zstd_launches = (uint32_t)ns;
    t.d2h_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_done).count();
    t.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (!r.host) { t.h2d_ms = 0; t.d2h_ms = 0; }
    return TSX_OK;
}

// ---- everything else: forward chain without compression, the inverse chain, CRC only ---------------------------------------------------
// Enqueues the kernels of chunks [lo, lo + n) on compute stream st; e[SUB_BEGUN .. SUB_DONE] (the piece's row of sub_ev) are recorded at the
// stage boundaries.
// stage_key: this piece's first kernel also brings the key schedule the host built (c->h_key) to the device (c->d_key); c->ev_key is
// recorded behind it.  Nothing here is a copy: descriptors and key come in through begin_batch_kernel, results leave through the kernels
// that produce them (tsx_chunk_desc mirror in pinned memory).
static int launch_stages(const tsx_run& r, const tsx_sub& sb, hipEvent_t* e, hipStream_t st, bool stage_key) {
    tsx_ctx* c = r.c;
    const uint32_t n = sb.n, lo = sb.lo, flags = r.flags;
    tsx_chunk_desc* dd = c->d_descs + lo;
    tsx_chunk_desc* const hm = c->hd_descs + lo;                       // the batch's descriptors in pinned memory, as the device addresses them
    int32_t* ds = c->d_status + lo;
    uint8_t* dmid = c->d_mid ? c->d_mid + (size_t)lo * c->mid_stride : nullptr;
    // the Zstd workspace of chunk i is slot i of the batch, whichever piece it travels in: pieces of one batch co-reside
    void* dzw = c->d_zwork ? (uint8_t*)c->d_zwork + (size_t)lo * tsx_zstd_workspace_bytes(1, 0) : nullptr;
    uint32_t* const dpart = c->d_partials + (size_t)lo * c->partials_per_chunk;     // this piece's slice of the CRC / GHASH partial sums
    tsx_timing& t = c->timing;
    memcpy(c->h_descs + lo, r.descs + lo, (size_t)n * sizeof(tsx_chunk_desc));
    {
        const uint32_t kw = stage_key ? (uint32_t)(sizeof(tsx_gcm_key) / 16) : 0u;
        const uint32_t blocks = std::max((n + 255u) / 256u, stage_key ? 6u : 1u);
        hipLaunchKernelGGL(begin_batch_kernel, dim3(blocks), dim3(256), 0, st, (const tsx_chunk_desc*)hm, dd, ds, n,
                           stage_key ? (const uint4*)c->hd_key : (const uint4*)nullptr, (uint4*)c->d_key, kw);
        if (stage_key) HIPCHK(hipEventRecord(c->ev_key, st));
    }
    HIPCHK(hipEventRecord(e[SUB_BEGUN], st));
    if (r.mode == 2) {
        tsx_launch_crc32c(st, c->dev->d_crc, r.d_src, dd, n, r.max_len, dpart, 0);
        HIPCHK(hipEventRecord(e[SUB_STAGE1], st)); HIPCHK(hipEventRecord(e[SUB_STAGE2], st));
        t.crc_launches += 2;
        hipLaunchKernelGGL(publish_status_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dd, (const int32_t*)ds, n, hm);      // a reused descriptor must not keep an old status
    } else if (r.mode == 0) {
        // forward chain WITHOUT compression (producers compress: RemoteStorageManager.java:381-398 leaves Zstd out): CRC32C of the chunk,
        // then AES-256-GCM (or the plain copy) as batch kernels - milliseconds of work, no residency to protect
        if (flags & TSX_CRC) { tsx_launch_crc32c(st, c->dev->d_crc, r.d_src, dd, n, r.max_len, dpart, 0); t.crc_launches += 2; }
        HIPCHK(hipEventRecord(e[SUB_STAGE1], st));
        HIPCHK(hipEventRecord(e[SUB_STAGE2], st));
        if (r.enc) {
            launch_gcm_stage(r, st, lo, n, 0, 0, 0, r.max_len, r.d_src, r.d_dst);
            gcm_verify_in_stream(r, sb, st);                            // TSX_VERIFY_GCM (and its test hook): behind the stage, in front of the publication
        } else launch_copy_chunks(r, st, lo, n, 0, r.d_src);
        hipLaunchKernelGGL(publish_status_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dd, (const int32_t*)ds, n, hm);
    } else {
        HIPCHK(hipEventRecord(e[SUB_STAGE1], st));
        const uint8_t* zsrc = r.d_src;    // where the Zstd frames live when there is no encryption
        if (r.enc) {
            launch_gcm_stage(r, st, lo, n, 0, 1, r.comp ? 1 : 0, r.max_len, r.d_src, r.comp ? dmid : r.d_dst);
            zsrc = dmid;
        }
        HIPCHK(hipEventRecord(e[SUB_STAGE2], st));
        if (r.comp) {
            const uint32_t* skip = nullptr; uint32_t skip_stride = 0;
            if (c->d_bwork && c->bwork_cap >= tsx_zstd_blockmode_bytes(r.n, r.max_out) && dec_use_blocks(r.n, r.max_out)) {
                c->last_used_blocks = true;
                // one workgroup per block; what that form does not take (or gives up on) is decoded by the chunk-serial kernel behind it.
                // A piece of a batch works in its own part of the workspace (the layout is per chunk: headers, then arenas, of THIS launch).
                void* const bw = (uint8_t*)c->d_bwork + tsx_zstd_blockmode_bytes(lo, r.max_out);
                t.unzstd_launches += tsx_launch_zstd_decompress_blocks(st, zsrc, r.enc ? 1 : 0, (uint64_t)c->mid_stride, dd, n, r.max_out, r.d_dst, ds, bw);
                skip = tsx_zstd_blockmode_skip(bw, &skip_stride);
                c->blk_pieces.push_back({lo, n}); c->last_max_out = r.max_out;
            }
            // (a batch decode next to running uploads takes the scratch-free build of the chunk-serial kernel: a dispatch that needs scratch
            //  waits for the compressor service's kernel - and its scratch - to go away)
            bool busy_service = false;
            if (!skip) busy_service = svc_busy(c->dev);
            t.unzstd_launches += tsx_launch_zstd_decompress(st, zsrc, r.enc ? 1 : 0, (uint64_t)c->mid_stride, dd, n, r.d_dst, ds, dzw, skip, skip_stride, busy_service);
        } else if (!r.enc) launch_copy_chunks(r, st, lo, n, 0, r.d_src);
        hipLaunchKernelGGL(publish_status_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dd, (const int32_t*)ds, n, hm);
        if (r.enc && !r.comp) launch_scrub_failed(r, st, lo, n);   // decrypted straight into the caller's slots: nothing of a chunk that failed its tag check stays
    }
    HIPCHK(hipEventRecord(e[SUB_STAGE3], st));
    if (r.mode == 1 && (flags & TSX_CRC)) {
        // CRC of the restored bytes; upper bound of a restored chunk is its slot capacity
        tsx_launch_crc32c(st, c->dev->d_crc, r.d_dst, dd, n, r.max_out, dpart, 1, hm);
        t.crc_launches += 2;
    }
    HIPCHK(hipEventRecord(e[SUB_DONE], st));                                 // the batch's descriptors in pinned memory are filled in when this event has passed
    return TSX_OK;
}

// Zero-copy output for the encrypt-only forward chain (producers compress: RemoteStorageManager.java:381-398 leaves Zstd out): the GCM
// kernel's waves write IV || C || TAG straight into the caller's slots when the device can address the WHOLE buffer - the compress path
// got this in round 4.  Slot layout only (a packed batch still travels through the device buffer: its chunks are packed by the copies).
static bool stages_zero_copy_ok(const tsx_run& r, size_t) { return r.mode == 0 && r.enc && r.host && !r.packed && !g_cfg.no_zero_copy_out; }

static int run_batch_inner(tsx_run& r) {
    tsx_ctx* c = r.c;
    const uint32_t n = r.n;
    const tsx_trace tr;
    tsx_plan pl;
    int rc = plan_batch(r, stages_zero_copy_ok, &pl);
    if (rc) return rc;
    tr.mark("workspace reserved");
    hipStream_t st = c->st;
    memset(&c->timing, 0, sizeof c->timing);
    // ---- sub-batches: a host-memory batch is cut into pieces whose H2D copy, kernels and D2H copy overlap (device-memory batches have
    // nothing to overlap): pieces of >= 64 MiB in order on ONE compute stream, three streams in all (the chunk-serial frame decoder is bound
    // by per-chunk latency - ~30 ms however few chunks a launch has: its pieces are >= 512 chunks).
    std::vector<tsx_sub> subs;
    const bool pipelined = r.host && pl.monotonic && !g_cfg.no_pipeline;
    // A fetch of 16 .. 256 chunks (a consumer catching up: ChunkCache.java:159-184 with a large prefetch.max.size) decodes in the block
    // form, whose cost is a ~1.5 ms chain of short kernels + a part proportional to the chunks: cut into up to 8 pieces of >= 8 chunks,
    // spread over the context's compute streams so that the pieces' chains overlap each other, the later pieces' copy-in and the earlier
    // pieces' copy-out.  (Round 3 only cut batches of >= 512 chunks: 64 chunks took 7 ms device resident and 17 ms host to host.)
    c->blk_pieces.clear(); c->last_used_blocks = false;
    const bool inv_blocks = r.mode == 1 && r.comp && pipelined && n >= 16 && c->d_bwork && dec_use_blocks(n, r.max_out) && !g_cfg.no_dec_pieces;
    if (pipelined) {
        size_t budget = g_cfg.sub_bytes > 0 ? (size_t)g_cfg.sub_bytes : TSX_SUB_BYTES;
        size_t max_subs = TSX_MAX_SUBS;
        if (pl.in_bytes / budget + 1 > max_subs) budget = pl.in_bytes / max_subs + 1;
        uint32_t min_chunks = r.comp ? 512u : 1u;
        if (inv_blocks) { max_subs = 8; budget = 0; min_chunks = (n + 7) / 8 < 8 ? 8u : (n + 7) / 8; }
        uint32_t lo = 0;
        while (lo < n) {
            uint32_t hi = lo; size_t bytes = 0;
            while (hi < n && (bytes < budget || hi - lo < min_chunks) && subs.size() + 1 <= max_subs) { bytes += r.descs[hi].src_len; hi++; }
            if (subs.size() + 1 == max_subs) hi = n;
            subs.push_back({lo, hi - lo, (size_t)r.descs[lo].src_off, (size_t)(r.descs[hi - 1].src_off + r.descs[hi - 1].src_len)});
            lo = hi;
        }
    } else subs.push_back({0, n, 0, pl.in_bytes});
    const size_t ns = subs.size();
    const bool multi = inv_blocks && ns > 1;                            // pieces side by side: piece k on compute stream k mod 4
    for (size_t k = 1; k < ns; k++) for (auto& e : c->sub_ev[k]) if (!e) HIPCHK(hipEventCreate(&e));
    if (multi) for (size_t k = 1; k < ns && k < 4; k++) if (!c->st_pc[k - 1]) HIPCHK(hipStreamCreateWithFlags(&c->st_pc[k - 1], hipStreamNonBlocking));
    auto stream_of = [&](size_t k) { return (multi && k % 4) ? c->st_pc[k % 4 - 1] : st; };
    HIPCHK(hipEventRecord(c->ev[EV_BEGIN], st));
    bool stage_key = false;
    if (r.enc) {
        // The key schedule is built on the host (~10 us with the host's carry-less multiplier) and travels as ONE 21 KB copy in front of the
        // batch's GCM kernels instead of a raw-key copy + gcm_setup_kernel: that kernel was 0.17 of a single-chunk fetch's 1.7 ms and, on a
        // busy device, one more small kernel waiting for a slot.  Test hook gcm_setup_kernel keeps the kernel (both
        // produce the same schedule).
        if (!g_cfg.gcm_setup_kernel) {
            tsx_gcm_key_build_host(r.params->key, r.params->aad, r.params->aad_len, c->h_key);    // piece 0's first kernel takes it to the device
            stage_key = true;
        } else {
            memcpy(c->h_keyraw, r.params->key, 32); memcpy(c->h_keyraw + 32, r.params->aad, 64);
            HIPCHK(hipMemcpyAsync(c->d_keyraw, c->h_keyraw, 96, hipMemcpyHostToDevice, st));    // (run_batch wipes both device copies whatever was written)
            tsx_launch_gcm_setup(st, c->dev->d_aes, c->d_keyraw, c->d_keyraw + 32, r.params->aad_len, c->d_key);
            if (multi) HIPCHK(hipEventRecord(c->ev_key, st));
        }
    }
    if (r.host) HIPCHK(hipEventRecord(c->ev[EV_H2D_FIRST], c->st_in));
    size_t packed_at = 0; bool packed_full = false;
    auto enqueue_piece = [&](size_t k) -> int {
        const tsx_sub& sb = subs[k];
        hipEvent_t* e = c->sub_ev[k];
        hipStream_t ks = stream_of(k);
        if (r.host) {
            // pageable memory is staged by the runtime (the call returns when the source has been read); memory pinned with
            // tsx_host_register goes by DMA and the call returns at once - either way the copy overlaps the kernels of earlier pieces
            if (sb.in_hi > sb.in_lo) HIPCHK(hipMemcpyAsync(c->d_in + sb.in_lo, (const uint8_t*)r.src + sb.in_lo, sb.in_hi - sb.in_lo, hipMemcpyHostToDevice, c->st_in));
            HIPCHK(hipEventRecord(e[SUB_STAGED_IN], c->st_in));
            HIPCHK(hipStreamWaitEvent(ks, e[SUB_STAGED_IN], 0));
        }
        if (multi && ks != st && r.enc) HIPCHK(hipStreamWaitEvent(ks, c->ev_key, 0));      // (piece 0 went first: its begin kernel staged the key)
        return launch_stages(r, sb, e, ks, stage_key && k == 0);
    };
    // The restored chunks of a fetch are what crosses PCIe (4 MiB each against 1.3 MB in): one copy stream moves them at ~31 GB/s - 8.7 of a
    // 64-chunk window's 10.4 ms; the pieces' copies alternate between two streams.
    std::vector<int32_t> rcode;                                         // TSX_VALIDATE_RECORDS (transform only: run_batch clears the flag elsewhere)
    if (r.flags & TSX_VALIDATE_RECORDS) rcode.assign(n, 0);
    bool out2 = inv_blocks && multi && r.host;
    if (out2 && !c->st_out2 && hipStreamCreateWithFlags(&c->st_out2, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->st_out2 = nullptr; out2 = false; }
    auto collect_piece = [&](size_t k) -> int {
        const tsx_sub& sb = subs[k];
        if (tr.on) {                                                    // (test hook: which stage a waiting batch is waiting in)
            static const char* const names[SUB_EV_COUNT] = {"descriptors up + status init", "stage 1", "stage 2", "stage 3", "descriptors down", "copy-in landed"};
            if (r.host) { (void)hipEventSynchronize(c->sub_ev[k][SUB_STAGED_IN]); tr.mark(names[SUB_STAGED_IN]); }
            for (int q = SUB_BEGUN; q <= SUB_DONE; q++) { (void)hipEventSynchronize(c->sub_ev[k][q]); tr.mark(names[q]); }
        }
        HIPCHK(wait_event_watching(c, c->sub_ev[k][SUB_DONE]));              // descriptors of piece k are on the host
        memcpy(r.descs + sb.lo, c->h_descs + sb.lo, (size_t)sb.n * sizeof(tsx_chunk_desc));
        if (!rcode.empty()) check_apply(r.descs, rcode.data(), sb.lo, sb.n);
        if (r.zc_dst) return TSX_OK;                                    // the bytes are in the caller's buffer already
        if (r.host && r.mode != 2) return copy_back(r, sb, &packed_at, &packed_full, (out2 && (k & 1)) ? c->st_out2 : c->st_out);
        return TSX_OK;
    };
    if (multi || !rcode.empty()) {
        for (size_t k = 0; k < ns; k++) if ((rc = enqueue_piece(k))) return rc;
        // record-batch validation of a chain that does not compress: behind the last piece's input copy, and its verdicts are in hand
        // before the first piece's descriptors reach the caller (the pieces are all queued first: no copy-out overlaps a later piece's kernels)
        if (!rcode.empty() && (rc = records_validate(r, r.host ? c->sub_ev[ns - 1][SUB_STAGED_IN] : nullptr, rcode.data()))) return rc;
        for (size_t k = 0; k < ns; k++) if ((rc = collect_piece(k))) return rc;
        if (multi) for (size_t k = 1; k < ns; k++) HIPCHK(hipStreamWaitEvent(st, c->sub_ev[k][SUB_DONE], 0));   // the batch's end event covers every piece
    } else {
        // software pipeline on the host: copy-in + kernels of piece k are queued before the host waits for piece k - 1's descriptors
        // (they say how many bytes each chunk produced) and queues its copy-out
        for (size_t k = 0; k <= ns; k++) {
            if (k < ns && (rc = enqueue_piece(k))) return rc;
            if (k < ns) tr.mark("piece enqueued (copy-in + kernels)");
            if (k > 0 && (rc = collect_piece(k - 1))) return rc;
            if (k > 0) tr.mark("piece collected (descriptors back, copy-out queued)");
        }
    }
    if (r.host) HIPCHK(hipEventRecord(c->ev[EV_D2H_LAST], c->st_out));
    if (r.enc) {
        // the key material leaves the device behind the batch's last kernel (every piece's chain has been joined into st above); the pinned
        // originals are wiped by run_batch
        launch_wipe_key(c, st);
        c->key_wiped = true;
    }
    HIPCHK(hipEventRecord(c->ev[EV_END], st));
    HIPCHK(hipStreamSynchronize(st));
    tr.mark("compute stream idle");
    if (r.host) { HIPCHK(hipStreamSynchronize(c->st_in)); HIPCHK(hipStreamSynchronize(c->st_out)); if (out2) HIPCHK(hipStreamSynchronize(c->st_out2)); }
    tr.mark("copy streams idle");
    HIPCHK(hipGetLastError());
    tsx_timing& t = c->timing;
    for (size_t k = 0; k < ns; k++) {
        hipEvent_t* e = c->sub_ev[k];
        const float a = ev_ms(e[SUB_BEGUN], e[SUB_STAGE1]), b = ev_ms(e[SUB_STAGE1], e[SUB_STAGE2]), d = ev_ms(e[SUB_STAGE2], e[SUB_STAGE3]), f = ev_ms(e[SUB_STAGE3], e[SUB_DONE]);
        if (r.mode == 2) t.crc_ms += a;
        else if (r.mode == 0) { t.crc_ms += (r.flags & TSX_CRC) ? a : 0; t.gcm_ms += d; }
        else { t.gcm_ms += r.enc ? b : 0; t.unzstd_ms += d; t.crc_ms += (r.flags & TSX_CRC) ? f : 0; }
    }
    t.total_ms = ev_ms(c->ev[EV_BEGIN], c->ev[EV_END]);
    if (r.host) {
        // with pieces in flight the copies overlap the kernels: h2d_ms / d2h_ms are the spans of the copy streams, not additive
        t.h2d_ms = ev_ms(c->ev[EV_H2D_FIRST], c->sub_ev[ns - 1][SUB_STAGED_IN]);
        t.d2h_ms = r.mode != 2 ? ev_ms(c->sub_ev[0][SUB_DONE], c->ev[EV_D2H_LAST]) : 0;
        const float tail = ev_ms(c->ev[EV_BEGIN], c->ev[EV_D2H_LAST]);
        if (r.mode != 2 && tail > t.total_ms) t.total_ms = tail;
    }
    return TSX_OK;
}

// The pinned copies of the key and of its schedule do not outlive the batch in readable form
static void ctx_wipe_host_key(tsx_ctx* c) { memset(c->h_keyraw, 0, 128); memset(c->h_key, 0, sizeof(tsx_gcm_key)); }

// Every stream this context owns is idle afterwards
static void ctx_sync_streams(tsx_ctx* c) {
    hipStreamSynchronize(c->st_in); hipStreamSynchronize(c->st); hipStreamSynchronize(c->st_out);
    if (c->st_out2) hipStreamSynchronize(c->st_out2);
    for (auto& q : c->st_pc) if (q) hipStreamSynchronize(q);
}

int run_batch(tsx_ctx* c, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src, size_t src_size, void* dst,
              size_t dst_size, int mem_kind, int mode, bool pooled, tsx_rec_stream* rs) {
    if (!descs || (n && !src) || (mode != 2 && (!params || (n && !dst)))) return TSX_E_INVAL;
    if (mem_kind != TSX_MEM_HOST && mem_kind != TSX_MEM_DEVICE && mem_kind != TSX_MEM_HOST_PACKED) return TSX_E_INVAL;
    const bool packed = mem_kind == TSX_MEM_HOST_PACKED;
    if (packed && mode != 0) return TSX_E_INVAL;
    uint32_t flags = mode == 2 ? TSX_CRC : params->flags;
    if (flags & ~(TSX_COMPRESS | TSX_ENCRYPT | TSX_CRC | TSX_ZSTD_CHECKSUM | TSX_VERIFY | TSX_VERIFY_GCM | TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES)) return TSX_E_INVAL;
    // the content checksum is the compressor's to write; a decoder verifies whatever frame declares one, asked or not.  Verify on upload
    // reads back what the compressor wrote: both modify TSX_COMPRESS on transform and mean nothing anywhere else
    if (mode == 0 && (flags & (TSX_ZSTD_CHECKSUM | TSX_VERIFY)) && !(flags & TSX_COMPRESS)) return TSX_E_INVAL;
    // ... and the GCM verifier reads back what the GCM stage wrote: a modifier of TSX_ENCRYPT on transform
    if (mode == 0 && (flags & TSX_VERIFY_GCM) && !(flags & TSX_ENCRYPT)) return TSX_E_INVAL;
    // ... and the record-batch validator reads the source of an upload: a modifier of any transform
    // ... and the walk over a batch's records is part of that validator's visit to the batch: a modifier of TSX_VALIDATE_RECORDS
    if (mode == 0 && (flags & TSX_VALIDATE_FRAMES) && !(flags & TSX_VALIDATE_RECORDS)) return TSX_E_INVAL;
    if (mode != 0) flags &= ~(TSX_ZSTD_CHECKSUM | TSX_VERIFY | TSX_VERIFY_GCM | TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES);
    if (mode != 2) {
        if (params->aad_len > 64) return TSX_E_INVAL;
        if ((flags & TSX_COMPRESS) && !(params->zstd_level >= 0 && params->zstd_level <= 3)) return TSX_E_UNSUPPORTED;   // 0 = 3 (the library default), 1, 2, 3
        if ((flags & TSX_COMPRESS) && params->zstd_profile > TSX_ZSTD_PROFILE_DEVICE) return TSX_E_UNSUPPORTED;
        // the device profile has one parse - levels name libzstd's parsers; a fetch ignores the profile (callers build one parameter block for
        // both directions, and a Zstandard decoder reads every profile's frames)
        if (mode == 0 && (flags & TSX_COMPRESS) && params->zstd_profile == TSX_ZSTD_PROFILE_DEVICE && params->zstd_level != 0) return TSX_E_UNSUPPORTED;
    }
    memset(&c->records, 0, sizeof c->records); c->records.first_bad_pos = ~0ull;
    if (rs) {
        // a call on a stream (the entry point has checked the state): the flag is what it is for, and it never takes more than was declared
        if (mode != 0 || !(flags & TSX_VALIDATE_RECORDS)) return TSX_E_INVAL;
        uint64_t bytes = 0;
        for (uint32_t i = 0; i < n; i++) bytes += descs[i].src_len;
        if (bytes > rs->total - rs->consumed) return TSX_E_INVAL;
        if (rs->first_bad_reason) {
            // the verdict has fallen in an earlier call: nothing is allocated or launched, nothing of this call is delivered
            uint32_t max_len, max_out; size_t in_bytes; bool monotonic;
            const int vrc = validate(descs, n, src_size, dst_size, !packed, &max_len, &max_out, &in_bytes, &monotonic);
            if (vrc) return vrc;
            for (uint32_t i = 0; i < n; i++) { descs[i].status = TSX_E_RECORDS; descs[i].dst_len = 0; }
            rs->consumed += bytes;
            tsx_records_info& o = c->records;
            o.batches = rs->batches; o.compressed_batches = rs->compressed; o.first_bad_pos = rs->first_bad_pos; o.first_bad_reason = rs->first_bad_reason; o.repaired_chunks = rs->repaired;
            return TSX_OK;
        }
    }
    if (n == 0) return TSX_OK;
    tsx_device_scope keep;
    if (hipSetDevice(c->dev->hip_id) != hipSuccess) return TSX_E_DEVICE;
    tsx_run r{};
    r.c = c; r.params = params; r.descs = descs; r.n = n; r.src = src; r.dst = dst; r.src_size = src_size; r.dst_size = dst_size; r.mode = mode;
    r.flags = flags; r.host = mem_kind != TSX_MEM_DEVICE; r.packed = packed; r.pooled = pooled;
    r.enc = mode != 2 && (flags & TSX_ENCRYPT); r.comp = mode != 2 && (flags & TSX_COMPRESS); r.rs = rs;
    r.fuse_stages = r.comp && !g_cfg.stages_separate;
    const bool service = mode == 0 && r.comp;
    c->key_wiped = false; c->key_staged = false;
    // every batch of ordinary kernels claims the reserved CUs for its duration (+ fetch_quiet_ms); a fused compressing batch queues none
    svc_foreground_scope fg(service && r.fuse_stages ? nullptr : c->dev);
    const int rc = service ? run_compress(r) : run_batch_inner(r);
    // Whatever happened: nothing of this call is still in flight when it returns (the copies reference the caller's buffers), and
    // the data key does not stay behind in a context that may serve another segment next (the native side zeroises its
    // copy; the round keys and H powers are as good as the key).
    if (service && r.fuse_stages) {
        // nothing of the key was uploaded (every wave took and wiped its own copy of the schedule); what is left is the pinned original,
        // and run_compress returns only when none of the batch's members can still be running
        if (r.enc) ctx_wipe_host_key(c);
        if (c->key_staged && !c->key_wiped) {
            // the GCM verifier had brought the schedule to the device and the batch failed before its wipe kernel was queued
            hipMemcpyAsync(c->d_key, c->dev->h_zeros, sizeof(tsx_gcm_key), hipMemcpyHostToDevice, c->st);
            hipStreamSynchronize(c->st);
        }
        if (rc != TSX_OK) (void)hipGetLastError();
        return rc;
    }
    ctx_sync_streams(c);
    if (r.enc) {
        ctx_wipe_host_key(c);                                           // (no kernel of the batch can still be reading the schedule)
        if (!c->key_wiped) {
            // the batch failed before its wipe kernel was queued: both device copies are cleared here, whichever of them it wrote
            hipMemcpyAsync(c->d_keyraw, c->dev->h_zeros, 128, hipMemcpyHostToDevice, c->st);
            hipMemcpyAsync(c->d_key, c->dev->h_zeros, sizeof(tsx_gcm_key), hipMemcpyHostToDevice, c->st);
            hipStreamSynchronize(c->st);
        }
    }
    if (rc != TSX_OK) (void)hipGetLastError();
    return rc;
}
