// What the host-side translation units share (tsx_api.hip: devices, contexts, entry points; tsx_batch.hip: the batch pipelines;
// tsx_checks.hip: the checks of an upload; tsx_service.hip: the compressor service): the configuration, error reporting, the device
// record.  (Contexts and batches: tsx_ctx.h.)
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "tsx_internal.h"
#include "zstd_gpu.h"

void tsx_set_err(const char* what, hipError_t e);          // what tsx_strerror(TSX_E_DEVICE) says next, on this thread
void tsx_set_errmsg(const char* text);
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { tsx_set_err(#x, e_); return TSX_E_DEVICE; } } while (0)

// ---- configuration -----------------------------------------------------------------------------------------------------------------
// Read ONCE, in tsx_init: tsx_init_ex's tsx_config first, then the environment of the process for the few settings a deployment may
// want to change without touching code (INTEGRATION.md 5 lists them).  No entry point on a data path reads the environment.  The
// fields under "test hooks" have no environment variable: tests and measurement tools set them through tsx_debug_config().
struct tsx_cfg {
    uint32_t reserved_cus = 0xFFFFFFFFu;  // compute units the compressor service leaves to everything else (0xFFFFFFFF: one per shader engine); TSX_FETCH_RESERVED_CUS
    uint32_t svc_max_launch_ms = 60000;   // age limit of one launch of the service kernel (0 = none); TSX_SERVICE_MAX_LAUNCH_MS
    uint32_t svc_idle_exit_us = 2000;     // the service kernel ends when it has had nothing to do for this long (callers in a closed loop need ~1 ms to come back)
    uint32_t fetch_quiet_ms = 2000;       // tsx_config.fetch_quiet_ms: the reserved CUs work for the compressor too (guest waves) once no fetch has been seen for this long; 0 = never; TSX_FETCH_QUIET_MS
    uint32_t svc_keep_waves = 0;          // tsx_config.fetch_shared_cu_waves: compressor waves that stay on a reserved CU all the same; TSX_FETCH_SHARED_CU_WAVES
    long long pool_idle_bytes = -1;       // idle pooled workspace kept per device (-1: 4/9 of its memory); TSX_POOL_IDLE_BYTES
    uint32_t zstd_sched = 0;              // parser speculation schedule k0 | k1 << 8 (0 = the kernel's default; same bytes); TSX_ZSTD_SCHED
    bool debug = false;                   // TSX_DEBUG: HIP failures go to stderr as they happen
    bool allow_any_arch = false;          // TSX_ALLOW_ANY_ARCH: the CPU test harness
    // ---- test hooks (tsx_debug_config) ----
    uint32_t dec_block_chunks = 256;      // largest detransform batch that takes the block-parallel decoder form (0 = never)
    uint32_t comp_pieces = 4;             // members a compressing host-memory batch is cut into (input copy of piece k + 1 overlaps piece k's waves)
    long long sub_bytes = 0;              // input bytes per piece of the staging pipeline (0 = TSX_SUB_BYTES)
    bool stages_separate = false;         // one launch per stage instead of the whole chain in the compressor wave
    bool no_pipeline = false;             // host-memory batches in one piece
    bool no_zero_copy_out = false;        // never let the waves write into the caller's buffer
    bool zero_copy_packed = false;        // explicit contexts: packed output in place too
    bool gcm_setup_kernel = false;        // key schedule by gcm_setup_kernel instead of on the host
    bool no_dec_pieces = false;           // block-form fetches in one piece
    bool svc_normal_priority = false;     // the service's stream like any other (default: the device's LOWEST stream priority, a hardware queue of its own pool)
    bool trace = false;                   // timestamps of a batch's phases on stderr (tools/fetch_block_probe.py)
    // verify on upload (TSX_VERIFY): XOR 1 into byte `off` of chunk `chunk` of the batch (-1: none) - of the device copy of its source (put back
    // behind the verification), of its frame in the staging buffer - after the chunk's member has completed and before it is verified
    long long verify_damage_src_chunk = -1, verify_damage_src_off = 0, verify_damage_frame_chunk = -1, verify_damage_frame_off = 0;
    // verify on upload, GCM stage (TSX_VERIFY_GCM): XOR 1 into byte `off` of that chunk's delivered IV || C || TAG, through the device's view of the
    // destination, behind the GCM stage and in front of the GCM verifier - whether or not the flag is set (-1: none; an offset beyond dst_len: nothing)
    long long verify_damage_out_chunk = -1, verify_damage_out_off = 0;
    uint32_t verify_slice_chunks = 0;     // chunks per slice of the verifier's workspace (0 = as many as fit its byte budget)
    bool verify_force_fallback = false;   // every chunk is decoded in full and compared (phase two), none by the block form
};
extern tsx_cfg g_cfg;

// Every entry point that selects a device puts the calling thread's current device back on the way out: the caller may share
// the thread with another HIP user (a torch process, another JNI library) whose notion of "current device" is not ours to change.
struct tsx_device_scope {
    int prev = -1;
    tsx_device_scope() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~tsx_device_scope() { if (prev >= 0) (void)hipSetDevice(prev); }
    tsx_device_scope(const tsx_device_scope&) = delete;
    tsx_device_scope& operator=(const tsx_device_scope&) = delete;
};

struct tsx_ctx;
struct tsx_verifier;                                         // tsx_checks.hip: the device's verify-on-upload workspace
struct tsx_service;                                          // tsx_service.hip: nobody else looks inside
struct tsx_service_delete { void operator()(tsx_service* s) const; };

struct tsx_device {
    int hip_id = -1;
    tsx_crc_tables* d_crc = nullptr;
    tsx_aes_tables* d_aes = nullptr;
    tsx_zstd_consts* d_zc = nullptr;
    uint8_t* h_zeros = nullptr;                    // pinned sizeof(tsx_gcm_key) zero bytes: key material is wiped by COPYING zeros - a memset is a
                                                   // kernel, and a kernel waits for a slot on a chip full of compressor waves (measured: 52 ms on
                                                   // average, up to 489 ms, per wipe: profiles/r03_bench_rocprofv3_kernel_stats_before_zero_copy_wipes.csv)
    char name[256] = {0};
    char arch[256] = {0};
    // pooled contexts of the ctx-less calls: idle ones, how many are out, batches served (all under g_mu)
    std::vector<tsx_ctx*> idle;
    size_t idle_bytes = 0;
    size_t idle_cap = 0;                                     // most idle workspace kept (init_devices: a fraction of THIS device's memory)
    std::vector<std::pair<void*, size_t>> spare_bwork;       // block-form decoder workspaces that left their context (pool_release), for the next one
    std::unique_ptr<tsx_service, tsx_service_delete> svc;
    tsx_verifier* verifier = nullptr;                        // created by the first verifying batch (verifier_of), freed with the device
    // copy streams of the context-less compressing calls, shared by the callers: ONE of each.  With a stream per caller a segment's copies
    // stood behind other callers' in the engines' queues anyway, and more streams measured worse (profiles/r04_broker_shape_experiments.txt).
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    uint32_t in_use = 0;
    uint64_t batches = 0;
};

// Device `index` of tsx_init's list (nullptr: no such device).  The list does not change between tsx_init and tsx_shutdown.
tsx_device* tsx_device_at(int index);
