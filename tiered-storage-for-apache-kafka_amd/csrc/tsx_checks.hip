// The checks that run on the device before an uploaded chunk is reported to the caller (the pipelines that call them: tsx_batch.hip):
//   TSX_VERIFY            verify_piece           every Zstandard frame of a piece decodes to its source chunk
//   TSX_VERIFY_GCM        gcm_verify_piece       the delivered IV || C || TAG of a compressing piece (gcm_verify_in_stream: of an encrypt-only one)
//   TSX_VALIDATE_RECORDS  records_validate       the batch's source is a stream of valid Kafka record batches
// Each says one code per chunk - 0 (passed, or the chunk was not TSX_OK anyway), its error, or TSX_E_NOMEM for a chunk it could not look
// at (never "not looked at" as TSX_OK: every code starts from TSX_E_NOMEM) - and check_apply writes the codes into the descriptors.
// PRECEDENCE, as a caller sees it: a chunk keeps the first error it gets, and the pipelines apply in this order - (1) the stage's own
// error, (2) the Zstandard verifier, (3) the GCM verifier, which skips what (1) and (2) failed, (4) the record validator.  So a chunk
// behind a bad record batch that also fails a verifier is TSX_E_VERIFY.  The three share four parts: check_block, timed_wait, damage, check_apply.
#include <algorithm>
#include <mutex>
#include <new>
#include <string.h>

#include "tsx_ctx.h"
#include "zstd_dec_blocks.h"

// ---- the shared parts -------------------------------------------------------------------------------------------------------------------
void check_apply(tsx_chunk_desc* descs, const int32_t* code, uint32_t lo, uint32_t n) {
    for (uint32_t i = lo; i < lo + n; i++) if (code[i] && descs[i].status == TSX_OK) { descs[i].status = code[i]; descs[i].dst_len = 0; }
}

// The context's pinned result block, at least `need` bytes (created by the first checking batch; one check at a time uses it, and each
// has taken what it needs out of it before it returns).  TSX_E_NOMEM: the host has no memory for it - the caller leaves its chunks
// TSX_E_NOMEM and does not fail (said_per_chunk).
static int check_block(tsx_ctx* c, size_t need) {
    if (c->check_cap >= need) return TSX_OK;
    svc_free_host(c->dev, c->h_check); c->h_check = nullptr; c->hd_check = nullptr; c->check_cap = 0;
    const size_t cap = need + need / 4 + 256;
    if (hipHostMalloc((void**)&c->h_check, cap, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); c->h_check = nullptr; return TSX_E_NOMEM; }
    HIPCHK(hipHostGetDevicePointer((void**)&c->hd_check, c->h_check, 0));
    c->check_cap = cap;
    return TSX_OK;
}
static int said_per_chunk(int rc) { return rc == TSX_E_NOMEM ? TSX_OK : rc; }

// What launches() queues on the context's stream, waited for; its device time is added to *ms.  The kernels are ordinary kernels on a
// chip that compressor waves fill: they claim the reserved CUs like a fetch and are waited for with the fetch side's safety net.
template <class Launches>
static int timed_wait(tsx_ctx* c, float* ms, Launches launches) {
    svc_foreground_scope fg(c->dev);
    HIPCHK(hipEventRecord(c->ev[EV_CHECK_BEGIN], c->st));
    launches();
    HIPCHK(hipEventRecord(c->ev[EV_CHECK_END], c->st));
    HIPCHK(wait_event_watching(c, c->ev[EV_CHECK_END]));
    *ms += ev_ms(c->ev[EV_CHECK_BEGIN], c->ev[EV_CHECK_END]);
    return TSX_OK;
}

// test hooks verify_damage_*: one byte, one thread
__global__ void verify_damage_kernel(uint8_t* p) { *p ^= 1; }

// The byte a hook names - byte `off` of chunk `chunk` - if that is one of chunks [lo, lo + n) and has such a byte, else nullptr;
// where(chunk) -> {the chunk's first byte, how many it has}, asked only about a chunk of the range.
template <class Where>
static uint8_t* hooked_byte(long long chunk, long long off, uint32_t lo, uint32_t n, Where where) {
    if (chunk < lo || chunk >= (long long)lo + n || off < 0) return nullptr;
    const std::pair<uint8_t*, uint64_t> w = where((uint32_t)chunk);
    return (uint64_t)off < w.second ? w.first + off : nullptr;
}
// XOR 1 into it on st.  -> whether there was a byte to hit, i.e. a launch (the caller counts it)
static bool damage(hipStream_t st, uint8_t* p) {
    if (p) hipLaunchKernelGGL(verify_damage_kernel, dim3(1), dim3(1), 0, st, p);
    return p != nullptr;
}

// ---- TSX_VERIFY -------------------------------------------------------------------------------------------------------------------------
// ONE workspace per device (the literal and sequence arenas are ~21 MiB per 4 MiB chunk: too much per context with 32 callers in flight),
// created by the first verifying batch; a caller holds `mu` while a slice of its piece is verified in it.
struct tsx_verifier {
    std::mutex mu;
    uint8_t* work = nullptr; size_t work_cap = 0;  // [slice descriptors and status words][chunk headers][arenas]
    uint8_t* full = nullptr; size_t full_cap = 0;  // phase two: a chunk the block form did not take, restored in full
};
#define TSX_VERIFY_SLICE_BYTES ((size_t)3 << 29)   /* workspace budget of a slice: 1.5 GiB, ~73 chunks of 4 MiB (at least one chunk whatever its size) */
#define TSX_V_WANTED 3                             /* fourth word of a chunk's verdict (zstd_dec_blocks.h): the chunk was TSX_OK and is to be verified */

// What the verifier's kernels read, written on the device (the frame sizes exist only there): for chunk i of a slice, vdescs[i] describes
// its frame to the block form's kernels (zstd_gpu.h: tsx_launch_zstd_verify_blocks), fdescs[i] to the chunk-serial decoder of phase two
// (output at offset 0 of the verifier's buffer).  status == nullptr: the compressor waves own the status, in the descriptor itself.
// no_blocks (test hook verify_force_fallback): the block form is told to leave every chunk alone.
__global__ void verify_plan_kernel(const tsx_chunk_desc* __restrict__ descs, const int32_t* __restrict__ status, const uint32_t* __restrict__ zlen, uint32_t n,
                                   tsx_chunk_desc* __restrict__ vdescs, tsx_chunk_desc* __restrict__ fdescs, int32_t* __restrict__ vstatus, int32_t* __restrict__ fstatus,
                                   uint32_t* __restrict__ verdicts, int no_blocks) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const tsx_chunk_desc d = descs[i];
    const bool wanted = (status ? status[i] : d.status) == TSX_OK;
    tsx_chunk_desc v = d;
    v.src_off = 0; v.src_len = zlen[i] + 28; v.dst_cap = d.src_len; v.dst_len = 0; v.status = TSX_OK;
    v.dst_off = 0; fdescs[i] = v;
    v.dst_off = d.src_off; vdescs[i] = v;
    vstatus[i] = wanted && !no_blocks ? TSX_OK : TSX_E_INVAL;
    fstatus[i] = TSX_OK;
    verdicts[(size_t)i * ZB_VERDICT_WORDS + TSX_V_WANTED] = wanted ? 1u : 0u;
}
static_assert(ZB_VERDICT_WORDS == 4 && TSX_V_WANTED == 3, "a chunk's verdict: the verify kernel's three words and the plan kernel's");

// Phase two: the chunk restored in full by the chunk-serial decoder against its source.  V: the chunk's verdict words, zero on entry.
__global__ __launch_bounds__(256) void verify_compare_kernel(const uint8_t* __restrict__ restored, const uint8_t* __restrict__ orig, const tsx_chunk_desc* __restrict__ fdesc,
                                                             const int32_t* __restrict__ fstatus, uint32_t* __restrict__ V) {
    const uint32_t len = fdesc->dst_cap;
    bool diff = *fstatus != TSX_OK || fdesc->dst_len != len;          // (a frame the decoder rejects, or one of another size, restores nothing)
    if (!diff) for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < len; p += gridDim.x * 256) diff |= restored[p] != orig[p];
    if (diff) V[ZB_V_FAIL] = 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) V[ZB_V_SEEN] = 1;
}

static std::mutex g_verifier_mu;                    // creation of a device's verifier
static tsx_verifier* verifier_of(tsx_device* dev) {
    std::lock_guard<std::mutex> lk(g_verifier_mu);
    if (!dev->verifier) dev->verifier = new (std::nothrow) tsx_verifier;
    return dev->verifier;
}
void verifier_destroy(tsx_device& d) {
    if (d.verifier) { (void)hipFree(d.verifier->work); (void)hipFree(d.verifier->full); delete d.verifier; d.verifier = nullptr; }
}

// Chunks [sb.lo, sb.lo + sb.n) - a member that has just completed - before anything of them is reported: does the frame restore the chunk?
int verify_piece(tsx_run& r, const tsx_sub& sb, bool self_status, int32_t* code) {
    tsx_ctx* c = r.c;
    tsx_device* dev = c->dev;
    tsx_timing& t = c->timing;
    for (uint32_t i = 0; i < sb.n; i++) code[sb.lo + i] = TSX_E_NOMEM;
    tsx_verifier* const V = verifier_of(dev);
    if (!V) return TSX_OK;
    uint32_t max_len = 0;
    for (uint32_t i = sb.lo; i < sb.lo + sb.n; i++) if (r.descs[i].src_len > max_len) max_len = r.descs[i].src_len;
    const size_t per_chunk = tsx_zstd_verify_bytes(1, max_len) + 2 * sizeof(tsx_chunk_desc) + 8;
    uint32_t slice = g_cfg.verify_slice_chunks ? g_cfg.verify_slice_chunks : (uint32_t)std::min<size_t>(TSX_VERIFY_SLICE_BYTES / per_chunk, sb.n);
    if (slice < 1) slice = 1;
    if (slice > sb.n) slice = sb.n;
    int rc_ = check_block(c, (size_t)slice * ZB_VERDICT_WORDS * 4);
    if (rc_) return said_per_chunk(rc_);
    uint32_t* const words = (uint32_t*)c->h_check; uint32_t* const hd_words = (uint32_t*)c->hd_check;     // ZB_VERDICT_WORDS per chunk of a slice
    svc_foreground_scope fg(dev);                                       // (the piece's claim: taken before the workspace is waited for, held between its waits)
    std::lock_guard<std::mutex> lk(V->mu);
    const size_t head = ((size_t)slice * (2 * sizeof(tsx_chunk_desc) + 8) + 255) & ~(size_t)255;
    if (grow(dev, &V->work, &V->work_cap, head + tsx_zstd_verify_bytes(slice, max_len))) { (void)hipGetLastError(); return TSX_OK; }   // every chunk of the piece: TSX_E_NOMEM
    for (uint32_t lo = sb.lo; lo < sb.lo + sb.n; lo += slice) {
        const uint32_t n = std::min(slice, sb.lo + sb.n - lo);
        tsx_chunk_desc* const vdescs = (tsx_chunk_desc*)V->work; tsx_chunk_desc* const fdescs = vdescs + slice;
        int32_t* const vstatus = (int32_t*)(fdescs + slice); int32_t* const fstatus = vstatus + slice;
        const uint8_t* const frames = c->d_mid + (size_t)lo * c->mid_stride;
        // test hook verify_damage_src_*: a byte of the device copy of the source, put back behind the verification
        uint8_t* const src_hit = hooked_byte(g_cfg.verify_damage_src_chunk, g_cfg.verify_damage_src_off, lo, n, [&](uint32_t j) {
            return std::make_pair((uint8_t*)r.d_src + r.descs[j].src_off, (uint64_t)r.descs[j].src_len); });
        uint8_t* const frame_hit = hooked_byte(g_cfg.verify_damage_frame_chunk, g_cfg.verify_damage_frame_off, lo, n, [&](uint32_t j) {
            return std::make_pair(c->d_mid + (size_t)j * c->mid_stride, (uint64_t)c->mid_stride); });
        memset(words, 0, (size_t)n * ZB_VERDICT_WORDS * 4);
        rc_ = timed_wait(c, &t.unzstd_ms, [&] {
            t.unzstd_launches += damage(c->st, src_hit);
            t.unzstd_launches += damage(c->st, frame_hit);
            hipLaunchKernelGGL(verify_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, c->st, (const tsx_chunk_desc*)((self_status ? c->hd_descs : c->d_descs) + lo),
                               self_status ? (const int32_t*)nullptr : (const int32_t*)(c->d_status + lo), (const uint32_t*)(c->d_zlen + lo), n, vdescs, fdescs, vstatus, fstatus,
                               hd_words, g_cfg.verify_force_fallback ? 1 : 0);
            t.unzstd_launches += 1 + tsx_launch_zstd_verify_blocks(c->st, frames, (uint64_t)c->mid_stride, vdescs, vstatus, n, max_len, r.d_src, V->work + head, hd_words);
        });
        if (rc_) return rc_;
        // ---- phase two: what the block form did not take (above 16 MiB, more than 264 blocks, a frame it does not parse) is decoded in
        // full, chunk by chunk, by the register-only build of the chunk-serial decoder (uploads are running: nothing here may need
        // scratch), and compared byte for byte.  Rare, and allowed to synchronise.
        for (uint32_t i = 0; i < n; i++) {
            uint32_t* const W = words + (size_t)i * ZB_VERDICT_WORDS;
            const uint32_t j = lo + i;
            if (!W[TSX_V_WANTED]) { code[j] = TSX_OK; continue; }
            if (W[ZB_V_FAIL]) { code[j] = TSX_E_VERIFY; c->verify_block_form++; continue; }
            if (W[ZB_V_SEEN] && !W[ZB_V_NOT_TAKEN]) { code[j] = TSX_OK; c->verify_block_form++; continue; }
            c->verify_fallback++;
            if (grow(dev, &V->full, &V->full_cap, (size_t)r.descs[j].src_len + 64)) { (void)hipGetLastError(); continue; }     // code[j] stays TSX_E_NOMEM
            W[ZB_V_FAIL] = 0; W[ZB_V_NOT_TAKEN] = 0; W[ZB_V_SEEN] = 0;
            rc_ = timed_wait(c, &t.unzstd_ms, [&] {
                t.unzstd_launches += 1 + tsx_launch_zstd_decompress(c->st, c->d_mid + (size_t)j * c->mid_stride, 1, (uint64_t)c->mid_stride, fdescs + i, 1, V->full, fstatus + i,
                                                                    (uint8_t*)c->d_zwork + (size_t)j * tsx_zstd_workspace_bytes(1, 0), nullptr, 0, true);
                const uint32_t blocks = std::max(1u, std::min(1024u, r.descs[j].src_len / 4096u));
                hipLaunchKernelGGL(verify_compare_kernel, dim3(blocks), dim3(256), 0, c->st, (const uint8_t*)V->full, r.d_src + r.descs[j].src_off, (const tsx_chunk_desc*)(fdescs + i),
                                   (const int32_t*)(fstatus + i), hd_words + (size_t)i * ZB_VERDICT_WORDS);
            });
            if (rc_) return rc_;
            code[j] = W[ZB_V_FAIL] || !W[ZB_V_SEEN] ? TSX_E_VERIFY : TSX_OK;
        }
        if (damage(c->st, src_hit)) HIPCHK(hipStreamSynchronize(c->st));
    }
    HIPCHK(hipGetLastError());
    return TSX_OK;
}

// ---- TSX_VERIFY_GCM ---------------------------------------------------------------------------------------------------------------------
// The verifier's work items for chunks 0 .. n - 1 of a compressing piece, from the piece's descriptors in pinned memory as the host has
// left them (status, dst_off, dst_len, iv: the waves', or separate_finish's, with the Zstandard verifier's codes applied) and the frame
// sizes: reference = the chunk's frame in the staging buffer, delivered = the chunk's slot.  hd_key != nullptr (fused chain: the schedule
// exists in pinned memory only): the kernel brings it to the device as begin_batch_kernel does - a copy would be a blit that waits behind
// a chip full of compressor waves.
__global__ __launch_bounds__(256) void plan_gcm_verify_kernel(const tsx_chunk_desc* __restrict__ descs, const uint32_t* __restrict__ zlen, uint64_t mid_stride, uint32_t n,
                                                              tsx_gcm_chunk* __restrict__ g, const uint4* __restrict__ hd_key, uint4* __restrict__ d_key, uint32_t key_words16) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const tsx_chunk_desc d = descs[i];
        tsx_gcm_chunk c;
        c.in_off = (uint64_t)i * mid_stride; c.out_off = d.dst_off; c.len = zlen[i];
        for (int k = 0; k < 12; k++) c.iv[k] = d.iv[k];
        c.skip = d.status != TSX_OK ? 1 : d.dst_len != c.len + 28 ? 2 : 0;
        g[i] = c;
    }
    if (hd_key) for (uint32_t k = i; k < key_words16; k += gridDim.x * blockDim.x) d_key[k] = hd_key[k];
}

// Chunks [sb.lo, sb.lo + sb.n) of a compressing batch - a member whose GCM stage has run (in its waves, or in separate_finish) - before
// anything of them is reported or copied back: with the flag, do the delivered bytes decrypt to the frame and carry its tag?  The test
// hook verify_damage_out_* acts here, flag or no flag.
int gcm_verify_piece(tsx_run& r, const tsx_sub& sb, int32_t* code) {
    tsx_ctx* c = r.c;
    tsx_timing& t = c->timing;
    const bool verify = (r.flags & TSX_VERIFY_GCM) != 0;
    uint8_t* const out_hit = hooked_byte(g_cfg.verify_damage_out_chunk, g_cfg.verify_damage_out_off, sb.lo, sb.n, [&](uint32_t j) {
        return std::make_pair(r.d_dst + c->h_descs[j].dst_off, (uint64_t)(c->h_descs[j].status == TSX_OK ? c->h_descs[j].dst_len : 0)); });
    if (!verify && !out_hit) return TSX_OK;
    if (verify) {
        for (uint32_t i = 0; i < sb.n; i++) code[sb.lo + i] = c->h_descs[sb.lo + i].status == TSX_OK ? TSX_E_NOMEM : TSX_OK;
        const int brc = check_block(c, (size_t)sb.n * 4);
        if (brc) return said_per_chunk(brc);
        memset(c->h_check, 0, (size_t)sb.n * 4);
    }
    float ms = 0;
    const int rc = timed_wait(c, &ms, [&] {
        t.gcm_launches += damage(c->st, out_hit);
        if (!verify) return;
        const bool stage_key = r.fuse_stages;                           // (separate stages: separate_finish has uploaded it, run_batch wipes it)
        const uint32_t kw = (uint32_t)(sizeof(tsx_gcm_key) / 16);
        if (stage_key) { c->key_staged = true; c->key_wiped = false; }   // (run_batch clears d_key itself when the batch fails before this piece's wipe)
        hipLaunchKernelGGL(plan_gcm_verify_kernel, dim3(std::max((sb.n + 255u) / 256u, stage_key ? 6u : 1u)), dim3(256), 0, c->st, (const tsx_chunk_desc*)(c->hd_descs + sb.lo),
                           (const uint32_t*)(c->d_zlen + sb.lo), (uint64_t)c->mid_stride, sb.n, c->d_gchunks + sb.lo, stage_key ? (const uint4*)c->hd_key : (const uint4*)nullptr,
                           (uint4*)c->d_key, stage_key ? kw : 0u);
        tsx_launch_gcm_verify(c->st, c->dev->d_aes, c->d_key, c->d_gchunks + sb.lo, c->hd_descs + sb.lo, sb.n, (uint32_t)tsx_transformed_bound(r.max_len, TSX_COMPRESS),
                              c->d_mid + (size_t)sb.lo * c->mid_stride, r.d_dst, c->d_partials + (size_t)sb.lo * c->partials_per_chunk, (uint32_t*)c->hd_check, nullptr);
        t.gcm_launches += 3;
        if (stage_key) { launch_wipe_key(c, c->st); t.gcm_launches++; } // the schedule does not stay on the device between the pieces
    });
    if (rc) return rc;
    if (verify) {
        const uint32_t* const words = (const uint32_t*)c->h_check;      // one per chunk of the piece
        if (r.fuse_stages) c->key_wiped = true;
        t.gcm_ms += ms;
        for (uint32_t i = 0; i < sb.n; i++)                             // (a chunk that was TSX_OK and has no verdict has not been examined: not reported TSX_OK)
            if (c->h_descs[sb.lo + i].status == TSX_OK) code[sb.lo + i] = words[i] == TSX_GV_SEEN ? TSX_OK : TSX_E_VERIFY;
    }
    HIPCHK(hipGetLastError());
    return TSX_OK;
}

// The same of chunks [sb.lo, sb.lo + sb.n) of an encrypt-only batch, queued on st behind their GCM stage; nothing waits.  The hook: a
// chunk that fits its slot delivers src_len + 28 bytes.  The verifier works on the items plan_gcm_kernel has made (in: the source chunk
// on the device, out: where the chunk was delivered - with zero-copy output the caller's buffer); a chunk that fails is TSX_E_VERIFY in
// d_status before publish_status_kernel reports it: code and precedence are the device's to apply here.
void gcm_verify_in_stream(const tsx_run& r, const tsx_sub& sb, hipStream_t st) {
    tsx_ctx* c = r.c;
    c->timing.gcm_launches += damage(st, hooked_byte(g_cfg.verify_damage_out_chunk, g_cfg.verify_damage_out_off, sb.lo, sb.n, [&](uint32_t j) {
        const uint64_t len = (uint64_t)r.descs[j].src_len + 28;
        return std::make_pair(r.d_dst + r.descs[j].dst_off, len <= r.descs[j].dst_cap ? len : (uint64_t)0); }));
    if (!(r.flags & TSX_VERIFY_GCM)) return;
    tsx_launch_gcm_verify(st, c->dev->d_aes, c->d_key, c->d_gchunks + sb.lo, c->d_descs + sb.lo, sb.n, r.max_len, r.d_src, r.d_dst,
                          c->d_partials + (size_t)sb.lo * c->partials_per_chunk, nullptr, c->d_status + sb.lo);
    c->timing.gcm_launches += 2;
}

// ---- TSX_VALIDATE_RECORDS ---------------------------------------------------------------------------------------------------------------
// The source of the whole batch - every piece's input has landed behind `staged` (nullptr: it was on the device to begin with) - as ONE
// stream of Kafka record batches (records.hip): TSX_E_RECORDS from the chunk on in which the first invalid batch begins.  Two ordinary
// kernels on the context's stream, next to whatever the batch's own stages are doing (a compressing batch's waves have a second of work
// per chunk in front of them).  Everything the kernels say comes back through the context's pinned block (tsx_internal.h: tsx_rec_block).
// r.rs != nullptr (tsx_transform_batch_stream): the call's chunks continue the stream *r.rs describes - the host's working copy of the
// caller's state, every number of which has been checked - and *r.rs is the state behind this call when TSX_OK is returned; the entry
// point hands it to the caller only if the whole call succeeds.  There, a validator that cannot run fails the call (TSX_E_NOMEM): bytes
// it has not seen must not count as consumed.
bool tsx_records_state_ok(const tsx_rec_stream* s) {
    if (s->magic != TSX_REC_STATE_MAGIC || s->consumed > s->total || s->hdr_n > 60 || s->hdr_n > s->consumed || s->open > 1 || s->comp > 1) return false;
    if (s->first_bad_reason > TSX_REC_CRC || (s->first_bad_reason != 0) != (s->first_bad_pos != ~0ull) || (s->first_bad_reason && s->first_bad_pos > s->total)) return false;
    if (s->open && (s->hdr_n || s->open_end > s->total || s->open_end <= s->consumed || s->open_pos > s->consumed || s->consumed - s->open_pos < 61 ||
                    s->open_end - s->open_pos < 61 || s->open_end - s->open_pos > 12ull + 0x7FFFFFFFull)) return false;
    if (s->hdr_n && s->total - (s->consumed - s->hdr_n) < 61) return false;       // (fewer than 61 bytes left is a verdict, never a carry)
    return true;
}

int records_validate(tsx_run& r, hipEvent_t staged, int32_t* code) {
    tsx_ctx* c = r.c;
    tsx_rec_stream* const rs = r.rs;
    const int cannot = rs ? TSX_E_NOMEM : TSX_OK;
    for (uint32_t i = 0; i < r.n; i++) code[i] = TSX_E_NOMEM;
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < r.n; i++) bytes += r.descs[i].src_len;
    tsx_records_info& o = c->records;
    if (rs && bytes == 0) {                                             // a call without bytes changes nothing
        for (uint32_t i = 0; i < r.n; i++) code[i] = TSX_OK;
        o.batches = rs->batches; o.compressed_batches = rs->compressed; o.first_bad_pos = rs->first_bad_pos; o.first_bad_reason = rs->first_bad_reason;
        o.repaired_chunks = rs->repaired; o.ms = 0;
        return TSX_OK;
    }
    const bool frames = (r.flags & TSX_VALIDATE_FRAMES) != 0;           // (never on a stream: the entry point refuses it)
    const int rc = check_block(c, tsx_records_block_bytes(r.n, frames));
    if (rc) return rs ? rc : said_per_chunk(rc);
    // the view: position 0 is the first carried header byte - stream position `origin`
    const uint32_t hdr_n = rs ? rs->hdr_n : 0;
    const uint64_t origin = rs ? rs->consumed - hdr_n : 0;
    const uint64_t total = rs ? rs->total - origin : bytes;
    const uint64_t start = rs && rs->open ? rs->open_end - origin : 0;
    tsx_records_block_fill(c->h_check, r.descs, r.n, hdr_n, frames);
    const tsx_rec_block b = tsx_records_block_at(c->h_check, r.n, frames);
    if (rs) {
        tsx_rec_carry& in = b.head->in;
        in.open = rs->open; in.want = rs->want; in.reg = rs->reg; in.comp = rs->comp; in.hdr_n = hdr_n;
        memcpy(in.hdr, rs->hdr, hdr_n);
    }
    if (staged) HIPCHK(hipStreamWaitEvent(c->st, staged, 0));
    float ms = 0;
    const int wrc = timed_wait(c, &ms, [&] { tsx_launch_records(c->st, c->dev->d_crc, r.d_src, c->hd_check, r.n, total, start, frames); });
    if (wrc) return wrc;
    HIPCHK(hipGetLastError());
    if (!__atomic_load_n(&b.head->done, __ATOMIC_ACQUIRE)) return cannot;
    for (uint32_t i = 0; i < r.n; i++) code[i] = b.verdicts[i + 1];
    const tsx_rec_head& h = *b.head;
    if (rs) {
        // every number the device hands back is checked like the caller's: the state never holds what tsx_records_state_ok refuses
        tsx_rec_stream t = *rs;
        t.consumed += bytes; t.batches += h.batches; t.compressed += h.compressed; t.repaired += h.repaired; t.ms = ms;
        if (h.first_bad_reason) { t.first_bad_reason = h.first_bad_reason; t.first_bad_pos = h.bad_open ? rs->open_pos : origin + h.first_bad_pos; }
        t.hdr_n = 0; t.open = 0; t.open_pos = t.open_end = 0; t.want = t.reg = t.comp = 0; memset(t.hdr, 0, sizeof t.hdr);
        if (!h.first_bad_reason) {
            t.hdr_n = h.out.hdr_n;
            if (t.hdr_n <= 60) memcpy(t.hdr, h.out.hdr, t.hdr_n);
            const bool still = rs->open && start > bytes;               // the batch that was open on entry reaches beyond this call too
            if (h.out.open) { t.open = 1; t.open_pos = still ? rs->open_pos : origin + h.out.open_pos;
                              t.open_end = origin + h.out.open_end; t.want = h.out.want; t.reg = h.out.reg; t.comp = h.out.comp; }
        }
        if (!tsx_records_state_ok(&t)) return TSX_E_DEVICE;
        *rs = t;
        o.batches = t.batches; o.compressed_batches = t.compressed; o.first_bad_pos = t.first_bad_pos; o.first_bad_reason = t.first_bad_reason; o.repaired_chunks = t.repaired;
    } else {
        o.batches = h.batches; o.compressed_batches = h.compressed; o.first_bad_pos = h.first_bad_pos;
        o.first_bad_reason = h.first_bad_reason; o.repaired_chunks = h.repaired;
        o.records = frames && h.records <= 0xFFFFFFFFull ? (uint32_t)h.records : frames ? 0xFFFFFFFFu : 0u;
    }
    o.ms = ms;
    return TSX_OK;
}
