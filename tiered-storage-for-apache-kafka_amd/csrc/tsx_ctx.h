// What the front end's translation units share about a context and a batch (tsx_api.hip: lifecycle, contexts, the pool, entry points;
// tsx_batch.hip: the batch pipelines; tsx_checks.hip: the checks of an upload): the context record, the names of its events, what one
// batch carries through the pipelines, and the few functions the units call across.
#pragma once
#include "tsx_host.h"
#include "tsx_service.h"

#define TSX_MAX_SUBS 64                 /* sub-batches of one host-memory batch (staging pipeline) */

// tsx_ctx::ev[]: the events of a batch as a whole
enum {
    EV_BEGIN, EV_END,                   // on st: the batch's first and last kernel (tsx_timing.total_ms)
    EV_H2D_FIRST,                       // on the copy-in stream, in front of the first piece's input copy
    EV_D2H_LAST,                        // on the copy-out stream, behind the last piece's output copies
    EV_CHECK_BEGIN, EV_CHECK_END,       // on st: one timed wait of a check of an upload (tsx_checks.hip; the calling thread runs one at a time)
    EV_COUNT
};
// tsx_ctx::sub_ev[k][]: the events of piece k
enum {
    SUB_BEGUN,                          // on the piece's compute stream, behind begin_batch_kernel: descriptors (and key) are on the device
    SUB_STAGE1, SUB_STAGE2, SUB_STAGE3, // ... the stage boundaries (launch_stages; tsx_timing's per-stage times are the spans between them)
    SUB_DONE,                           // ... behind the piece's last kernel: its descriptors in pinned memory are filled in
    SUB_STAGED_IN,                      // on the copy-in stream: the piece's input has landed
    SUB_EV_COUNT
};

struct tsx_ctx {
    int dev_index = 0;
    tsx_device* dev = nullptr;
    hipStream_t st = nullptr;                      // kernels (+ descriptor copies)
    hipStream_t st_in = nullptr, st_out = nullptr; // H2D / D2H of the host-memory staging pipeline
    hipStream_t st_out2 = nullptr;                 // second D2H stream of a fetch cut into pieces (odd pieces; created on first use)
    hipStream_t st_pc[3] = {nullptr};              // compute streams of pieces 1.. of a block-form fetch cut into pieces (created on first use)
    hipEvent_t ev_key = nullptr;                   // key schedule ready (the piece streams wait for it)
    // device workspace (grown on demand)
    tsx_chunk_desc* d_descs = nullptr; size_t descs_cap = 0;
    tsx_chunk_desc* h_descs = nullptr;             // pinned mirror of the descriptors: no pageable copy ever sits in a stream
    tsx_chunk_desc* hd_descs = nullptr;            // ... as the device addresses it: compressor waves read and write it in place
    uint8_t* h_keyraw = nullptr;                   // pinned 128 bytes: key + aad on their way in (wiped after the batch)
    tsx_gcm_key* h_key = nullptr;                  // pinned: the key schedule built on the host (wiped after the batch)
    tsx_gcm_key* hd_key = nullptr;                 // ... as the device addresses it (every compressor wave takes its own copy, tsx_chain_fuse.key_on_host)
    uint32_t* d_segdone = nullptr;                 // per member of this context's batch: chunks that are done (device counters, self-resetting)
    uint32_t* h_segflag = nullptr;                 // ... and the words the last of them raise (pinned; hd_segflag = the device's address)
    uint32_t* hd_segflag = nullptr;
    tsx_gcm_chunk* d_gchunks = nullptr;
    int32_t* d_status = nullptr;
    uint32_t* d_zlen = nullptr;
    uint32_t* d_partials = nullptr; size_t partials_cap = 0; size_t partials_per_chunk = 0;   // (pieces that run side by side take their own slice)
    uint32_t last_max_out = 0;
    std::vector<std::pair<uint32_t, uint32_t>> blk_pieces;  // (first chunk, chunks) of every block-form decoder launch of the last batch
    tsx_gcm_key* d_key = nullptr;
    uint8_t* d_keyraw = nullptr;                 // 32 key + 64 aad
    uint8_t* d_in = nullptr; size_t in_cap = 0;    // staging for TSX_MEM_HOST
    uint8_t* d_out = nullptr; size_t out_cap = 0;
    uint8_t* d_mid = nullptr; size_t mid_cap = 0;  // compressed frames between the Zstd and GCM stages
    size_t mid_stride = 0;
    void* d_zwork = nullptr; size_t zwork_cap = 0; // Zstd per-chunk workspace
    void* d_bwork = nullptr; size_t bwork_cap = 0; // block-parallel frame decoder (small batches): chunk headers + literal / sequence arenas
    hipEvent_t ev[EV_COUNT] = {nullptr};
    hipEvent_t sub_ev[TSX_MAX_SUBS][SUB_EV_COUNT] = {{nullptr}};   // (row 0 is created with the context, the others by the first pipelined batch)
    tsx_timing timing{};
    bool pooled = false;
    bool last_used_blocks = false;                 // the last batch ran the block-parallel frame decoder (test hook)
    uint32_t last_members = 0;                     // members the last compressing batch went as (test hook)
    bool last_zero_copy = false;                   // ... and whether its waves wrote into the caller's buffer (test hook)
    bool key_wiped = false;                        // the batch's own wipe_key_kernel has cleared d_key / d_keyraw
    bool key_staged = false;                       // a fused compressing batch's GCM verifier has brought the key schedule to d_key (wiped behind every piece)
    // the checks of an upload (tsx_checks.hip): the block their kernels answer in, pinned, and as the device addresses it (created by the
    // first checking batch; one check at a time: the Zstandard verifier's four words per chunk of a slice, the GCM verifier's one word
    // per chunk of a piece, the record validator's tsx_rec_block)
    uint8_t* h_check = nullptr; uint8_t* hd_check = nullptr; size_t check_cap = 0;
    tsx_records_info records{};                    // what the last batch's record validator found
    uint32_t verify_block_form = 0, verify_fallback = 0;   // chunks of the last batch the block form judged / that were decoded in full (test hook)
};

struct tsx_sub { uint32_t lo, n; size_t in_lo, in_hi; };     // chunks [lo, lo + n), their input bytes [in_lo, in_hi) of src

struct tsx_run {                                              // what one batch needs everywhere in the pipelines
    tsx_ctx* c; const tsx_batch_params* params; tsx_chunk_desc* descs; uint32_t n; const void* src; void* dst; size_t src_size, dst_size;
    int mode; uint32_t flags, max_len, max_out; bool host, packed, enc, comp, fuse_stages, pooled;
    const uint8_t* d_src; uint8_t* d_dst;
    uint8_t* zc_dst;                                          // zero-copy output: the caller's buffer as the device addresses it (then d_dst), else nullptr
    tsx_rec_stream* rs;                                       // tsx_transform_batch_stream: the stream the call's chunks continue (records_validate), else nullptr
};

template <class T>
static int grow(tsx_device* dev, T** p, size_t* cap, size_t need) {
    if (need <= *cap && *p) return TSX_OK;
    if (*p) { svc_free_dev(dev, *p); *p = nullptr; *cap = 0; }
    size_t want = need + need / 8 + 256;
    hipError_t e = hipMalloc((void**)p, want * sizeof(T));
    if (e != hipSuccess) { tsx_set_err("hipMalloc(workspace)", e); return TSX_E_NOMEM; }
    *cap = want;
    return TSX_OK;
}

// Small detransform batches (a fetch: one chunk, a prefetch window) decode one workgroup per BLOCK instead of per chunk: the
// chunk-serial decoder needs 25-50 ms for a chunk however idle the chip is.  Up to 256 chunks (measured: 27.6 ms at 256 chunks against
// the chunk form's 33, profiles/r03_dec_latency_block_form.jsonl); the test hook dec_block_chunks moves the limit (0 = never).
static inline bool dec_use_blocks(uint32_t n, uint32_t max_out) { return n <= g_cfg.dec_block_chunks && tsx_zstd_blockmode_takes(max_out); }

// ---- tsx_api.hip, for the pipelines ----
// ctx_reserve; an allocation that fails drains the device's idle pooled contexts and is tried again
int reserve_or_drain(tsx_ctx* c, uint32_t n, uint32_t max_len, uint32_t max_out, uint32_t flags, bool host_mem, size_t in_bytes, size_t out_bytes);

// ---- tsx_batch.hip, for the entry points and the checks ----
int run_batch(tsx_ctx* c, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src, size_t src_size, void* dst,
              size_t dst_size, int mem_kind, int mode /*0 transform, 1 detransform, 2 crc only*/, bool pooled = false, tsx_rec_stream* rs = nullptr);
// the host ranges tsx_host_register has pinned (zero-copy output asks: device_alias_of_range); forget_all: tsx_shutdown
void registered_range_add(void* p, size_t bytes);
void registered_range_remove(void* p);
void registered_range_forget_all();
// wait for an event of a batch of ordinary kernels, with the safety net of svc_rotate; milliseconds between two events that have passed
hipError_t wait_event_watching(tsx_ctx* c, hipEvent_t ev);
float ev_ms(hipEvent_t a, hipEvent_t b);
// wipe_key_kernel on st: the key schedule and the raw key leave the device
void launch_wipe_key(tsx_ctx* c, hipStream_t st);

// ---- tsx_checks.hip, for the pipelines (and tsx_api.hip: verifier_destroy) ----
// One code per chunk into code[] (indexed like the batch: 0, the check's error, or TSX_E_NOMEM), waited for: the Zstandard verifier and
// the GCM verifier of chunks [sb.lo, sb.lo + sb.n) of a compressing batch, the record validator of a whole batch
int verify_piece(tsx_run& r, const tsx_sub& sb, bool self_status, int32_t* code);
int gcm_verify_piece(tsx_run& r, const tsx_sub& sb, int32_t* code);
int records_validate(tsx_run& r, hipEvent_t staged, int32_t* code);
// the GCM verifier of an encrypt-only piece: queued on st behind the piece's GCM stage, its codes go to d_status on the device
void gcm_verify_in_stream(const tsx_run& r, const tsx_sub& sb, hipStream_t st);
// code[lo .. lo + n) reach descs[lo .. lo + n): a chunk that already carries an error keeps it, one that takes a code delivers nothing
void check_apply(tsx_chunk_desc* descs, const int32_t* code, uint32_t lo, uint32_t n);
// the device's verify-on-upload workspace goes with the device (device current)
void verifier_destroy(tsx_device& d);
