// C-ABI front end of libtsxform: configuration, init / shutdown, contexts and their pool, host registration, and the entry points
// (the batch pipelines they run: tsx_batch.hip; the compressor service's host side: tsx_service.hip).
// See include/tsxform.h for the contract and the reference call sites each entry point replaces.
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "tsx_ctx.h"

tsx_cfg g_cfg;

static thread_local char g_last_err[256];
void tsx_set_err(const char* what, hipError_t e) {
    snprintf(g_last_err, sizeof g_last_err, "%s failed: %s", what, hipGetErrorString(e));
    if (g_cfg.debug) fprintf(stderr, "[tsxform] %s\n", g_last_err);
}
void tsx_set_errmsg(const char* text) { snprintf(g_last_err, sizeof g_last_err, "%s", text); }

static void cfg_from_env(tsx_cfg& c) {
    if (const char* e = getenv("TSX_FETCH_RESERVED_CUS")) { const long v = atol(e); c.reserved_cus = (uint32_t)(v < 0 ? 0 : v > 128 ? 128 : v); }
    if (const char* e = getenv("TSX_FETCH_SHARED_CU_WAVES")) { const long v = atol(e); c.svc_keep_waves = (uint32_t)(v < 0 ? 0 : v > 8 ? 8 : v); }
    if (const char* e = getenv("TSX_FETCH_QUIET_MS")) { const long v = atol(e); if (v >= 0) c.fetch_quiet_ms = (uint32_t)v; }
    if (const char* e = getenv("TSX_SERVICE_MAX_LAUNCH_MS")) { const long v = atol(e); if (v >= 0) c.svc_max_launch_ms = (uint32_t)v; }
    if (const char* e = getenv("TSX_POOL_IDLE_BYTES")) { const long long v = atoll(e); if (v >= 0) c.pool_idle_bytes = v; }
    if (const char* e = getenv("TSX_ZSTD_SCHED")) { unsigned a = 0, b = 0; if (sscanf(e, "%u,%u", &a, &b) == 2 && a >= 1 && a <= 59 && b >= 1 && b <= 59) c.zstd_sched = a | b << 8; }
    c.debug = getenv("TSX_DEBUG") != nullptr;
    c.allow_any_arch = getenv("TSX_ALLOW_ANY_ARCH") != nullptr;
}

// Test / measurement hook (not part of the ABI in include/tsxform.h): set one configuration field, return its previous value
// (TSX_E_INVAL: no such field).  Takes effect for calls made afterwards; reserved_cus only for a tsx_init made afterwards.
extern "C" long long tsx_debug_config(const char* key, long long value) {
    if (!key) return TSX_E_INVAL;
#define CFG_FIELD(name, T) if (!strcmp(key, #name)) { const long long old = (long long)g_cfg.name; g_cfg.name = (T)value; return old; }
    CFG_FIELD(reserved_cus, uint32_t) CFG_FIELD(svc_max_launch_ms, uint32_t) CFG_FIELD(svc_idle_exit_us, uint32_t) CFG_FIELD(pool_idle_bytes, long long)
    CFG_FIELD(zstd_sched, uint32_t) CFG_FIELD(dec_block_chunks, uint32_t) CFG_FIELD(comp_pieces, uint32_t) CFG_FIELD(sub_bytes, long long)
    CFG_FIELD(stages_separate, bool) CFG_FIELD(no_pipeline, bool) CFG_FIELD(no_zero_copy_out, bool) CFG_FIELD(zero_copy_packed, bool)
    CFG_FIELD(gcm_setup_kernel, bool) CFG_FIELD(no_dec_pieces, bool) CFG_FIELD(debug, bool) CFG_FIELD(svc_normal_priority, bool) CFG_FIELD(svc_keep_waves, uint32_t) CFG_FIELD(fetch_quiet_ms, uint32_t) CFG_FIELD(trace, bool)
    CFG_FIELD(verify_damage_src_chunk, long long) CFG_FIELD(verify_damage_src_off, long long) CFG_FIELD(verify_damage_frame_chunk, long long)
    CFG_FIELD(verify_damage_frame_off, long long) CFG_FIELD(verify_damage_out_chunk, long long) CFG_FIELD(verify_damage_out_off, long long)
    CFG_FIELD(verify_slice_chunks, uint32_t) CFG_FIELD(verify_force_fallback, bool)
#undef CFG_FIELD
    return TSX_E_INVAL;
}

#define TSX_POOL_MAX_IDLE 32            /* idle pooled contexts kept per device (a broker: >= 10 RLM threads + read-ahead helpers + the fetch pool) ... */
// ... as long as their workspaces together stay under tsx_device.idle_cap = 4/9 of the device's memory (128 of the MI355X's 288 GB; a smaller
// device or several processes per GPU get their share: tsx_config.pool_idle_bytes); the rest are destroyed on release, and an
// allocation that fails drains the idle pool and is tried again (reserve_or_drain) - cached memory is never the reason for TSX_E_NOMEM.
#define TSX_POOL_MAX_IDLE_BWORK 4       /* idle contexts that keep their block-form decoder workspace (37 MiB per 4 MiB chunk: 9.4 GiB for a segment) */

static std::mutex g_mu;
static std::vector<tsx_device> g_devs;
static uint32_t g_rr = 0;
static thread_local int t_dev_hint = -1;
static const char kUninitVersion[] = "tsxform 0.5 (gfx950 HIP; uninitialised)";
static char g_version_buf[2][512];
static unsigned g_version_gen = 0;
static std::atomic<const char*> g_version{kUninitVersion};

tsx_device* tsx_device_at(int index) {
    std::lock_guard<std::mutex> lk(g_mu);
    return index < 0 || index >= (int)g_devs.size() ? nullptr : &g_devs[index];
}

extern "C" uint32_t tsx_abi_version(void) { return TSX_ABI_VERSION; }

// The string is composed in a buffer no reader can see yet and published with one pointer store at the end of a successful
// tsx_init: callers never observe a half-written string and need no lock.
extern "C" const char* tsx_version(void) { return g_version.load(std::memory_order_acquire); }

extern "C" const char* tsx_strerror(int code) {
    switch (code) {
        case TSX_OK: return "ok";
        case TSX_E_INVAL: return "invalid argument";
        case TSX_E_DEVICE: return g_last_err[0] ? g_last_err : "no usable gfx950 device / HIP failure";
        case TSX_E_NOMEM: return "out of memory";
        case TSX_E_DST_TOO_SMALL: return "destination slot too small";
        case TSX_E_TAG_MISMATCH: return "Tag mismatch";                                    // JCE AEADBadTagException text
        case TSX_E_BAD_FRAME: return "corrupt Zstd frame";
        case TSX_E_BAD_SIZE: return "Invalid decompressed size";                           // DecompressionChunkEnumeration.java:43
        case TSX_E_SHORT_CHUNK: return "encrypted chunk shorter than IV + tag";
        case TSX_E_UNSUPPORTED: return "unsupported parameter";
        case TSX_E_VERIFY: return "the frame written for this chunk does not restore it";
        case TSX_E_RECORDS: return "invalid record batch in the source at or before this chunk";
        default: return "unknown error";
    }
}

static void device_free_consts(tsx_device& d) {
    if (d.hip_id < 0) return;
    hipSetDevice(d.hip_id);
    svc_destroy(d);
    for (auto& b : d.spare_bwork) (void)hipFree(b.first);
    d.spare_bwork.clear();
    verifier_destroy(d);
    if (d.copy_in) hipStreamDestroy(d.copy_in);
    if (d.copy_out) hipStreamDestroy(d.copy_out);
    if (d.d_crc) hipFree(d.d_crc);
    if (d.d_aes) hipFree(d.d_aes);
    if (d.d_zc) hipFree(d.d_zc);
    if (d.h_zeros) hipHostFree(d.h_zeros);
    d.d_crc = nullptr; d.d_aes = nullptr; d.d_zc = nullptr; d.h_zeros = nullptr; d.copy_in = nullptr; d.copy_out = nullptr;
}

static int init_devices(std::vector<tsx_device>& devs, int want, const int* device_ids, const tsx_crc_tables* hc, const tsx_aes_tables* ha,
                        const tsx_zstd_consts* hz) {
    for (int i = 0; i < want; i++) {
        devs.emplace_back();
        tsx_device& d = devs.back();
        d.hip_id = device_ids ? device_ids[i] : i;
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, d.hip_id));
        snprintf(d.name, sizeof d.name, "%s", prop.name);
        snprintf(d.arch, sizeof d.arch, "%s", prop.gcnArchName);
        if (strncmp(d.arch, "gfx950", 6) != 0 && !g_cfg.allow_any_arch) {
            snprintf(g_last_err, sizeof g_last_err, "device %d is %s, this library is built for gfx950 only", d.hip_id, d.arch);
            return TSX_E_DEVICE;
        }
        HIPCHK(hipSetDevice(d.hip_id));
        {   size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !total_b) { (void)hipGetLastError(); total_b = prop.totalGlobalMem; }
            d.idle_cap = total_b / 9 * 4;
            if (g_cfg.pool_idle_bytes >= 0) d.idle_cap = (size_t)g_cfg.pool_idle_bytes;
        }
        HIPCHK(hipMalloc((void**)&d.d_crc, sizeof(tsx_crc_tables)));
        HIPCHK(hipMalloc((void**)&d.d_aes, sizeof(tsx_aes_tables)));
        HIPCHK(hipMalloc((void**)&d.d_zc, tsx_zstd_consts_bytes()));
        HIPCHK(hipHostMalloc((void**)&d.h_zeros, sizeof(tsx_gcm_key), hipHostMallocDefault));
        memset(d.h_zeros, 0, sizeof(tsx_gcm_key));
        HIPCHK(hipMemcpy(d.d_crc, hc, sizeof(tsx_crc_tables), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.d_aes, ha, sizeof(tsx_aes_tables), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.d_zc, hz, tsx_zstd_consts_bytes(), hipMemcpyHostToDevice));
        // the copy streams first, then the service's stream: whatever the runtime's stream -> hardware-queue assignment, the short copies and
        // their event markers are not the ones that end up behind the long-lived kernel
        HIPCHK(hipStreamCreateWithFlags(&d.copy_in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&d.copy_out, hipStreamNonBlocking));
        const int rc = svc_create(d, prop.multiProcessorCount);
        if (rc) return rc;
    }
    return TSX_OK;
}

extern "C" int tsx_init_ex(int device_count, const int* device_ids, const tsx_config* cfg) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_devs.empty()) return (int)g_devs.size();
    tsx_device_scope keep;
    {   // what the process has (defaults, or what tsx_debug_config set), then the caller's structure, then the environment - a deployment's last word
        tsx_cfg c = g_cfg;
        if (cfg && cfg->struct_size >= offsetof(tsx_config, fetch_quiet_ms)) {      // (the struct as it was before fetch_quiet_ms is accepted too)
            if (cfg->fetch_reserved_cus != TSX_CFG_DEFAULT) c.reserved_cus = cfg->fetch_reserved_cus > 128 ? 128 : cfg->fetch_reserved_cus;
            if (cfg->service_max_launch_ms != TSX_CFG_DEFAULT) c.svc_max_launch_ms = cfg->service_max_launch_ms;
            if (cfg->fetch_shared_cu_waves != TSX_CFG_DEFAULT) c.svc_keep_waves = cfg->fetch_shared_cu_waves > 8 ? 8 : cfg->fetch_shared_cu_waves;
            if (cfg->struct_size >= offsetof(tsx_config, fetch_quiet_ms) + 4 && cfg->fetch_quiet_ms != TSX_CFG_DEFAULT) c.fetch_quiet_ms = cfg->fetch_quiet_ms;
            if (cfg->pool_idle_bytes != TSX_CFG_DEFAULT64) c.pool_idle_bytes = (long long)cfg->pool_idle_bytes;
        } else if (cfg) return TSX_E_INVAL;
        cfg_from_env(c);
        g_cfg = c;
    }
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) {
        snprintf(g_last_err, sizeof g_last_err, "no HIP device visible");
        return TSX_E_DEVICE;
    }
    int want = device_count <= 0 ? visible : device_count;
    if (device_ids) { for (int i = 0; i < want; i++) if (device_ids[i] < 0 || device_ids[i] >= visible) return TSX_E_INVAL; }
    else if (want > visible) return TSX_E_INVAL;
    tsx_crc_tables* hc = new (std::nothrow) tsx_crc_tables;
    tsx_aes_tables* ha = new (std::nothrow) tsx_aes_tables;
    tsx_zstd_consts* hz = (tsx_zstd_consts*)malloc(tsx_zstd_consts_bytes());
    int rc = TSX_E_NOMEM;
    std::vector<tsx_device> devs;
    devs.reserve((size_t)want);
    if (hc && ha && hz) {
        tsx_crc_build_tables(hc);
        tsx_aes_build_tables(ha);
        tsx_zstd_build_consts(hz);
        rc = init_devices(devs, want, device_ids, hc, ha, hz);
    }
    delete hc; delete ha; free(hz);
    if (rc != TSX_OK) { for (auto& d : devs) device_free_consts(d); return rc; }   // nothing of a failed init stays allocated
    g_devs.swap(devs);
    char* vb = g_version_buf[g_version_gen++ & 1];
    const svc_geometry sg = svc_geometry_of(g_devs[0]);
    snprintf(vb, sizeof g_version_buf[0],
             "tsxform 0.5 (gfx950 HIP; CRC32C, AES-256-GCM, Zstd frames of levels 1-3; zstd parity target libzstd 1.5.7 / 1.5.6 profile, device profile; %d device(s): %s; "
             "compressor service: %u waves, %u of %u CUs reserved for fetches)",
             (int)g_devs.size(), g_devs[0].name, sg.waves, sg.cus_reserved, sg.cus);
    g_version.store(vb, std::memory_order_release);
    return (int)g_devs.size();
}

extern "C" int tsx_init(int device_count, const int* device_ids) { return tsx_init_ex(device_count, device_ids, nullptr); }

extern "C" int tsx_device_count(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return (int)g_devs.size();
}

static void ctx_free_device_mem(tsx_ctx* c) {
    hipSetDevice(c->dev->hip_id);
    // the key schedule and the raw key never outlive the context in readable form (copies of zeros, not kernels)
    if (c->st && c->d_key) { hipMemcpyAsync(c->d_key, c->dev->h_zeros, sizeof(tsx_gcm_key), hipMemcpyHostToDevice, c->st); }
    if (c->st && c->d_keyraw) { hipMemcpyAsync(c->d_keyraw, c->dev->h_zeros, 128, hipMemcpyHostToDevice, c->st); }
    if (c->st) hipStreamSynchronize(c->st);
    void* ptrs[] = {c->d_descs, c->d_gchunks, c->d_status, c->d_zlen, c->d_partials, c->d_key, c->d_keyraw, c->d_in, c->d_out, c->d_mid, c->d_zwork, c->d_bwork, c->d_segdone};
    for (void* p : ptrs) svc_free_dev(c->dev, p);
    svc_free_host(c->dev, c->h_segflag);
    svc_free_host(c->dev, c->h_descs);
    svc_free_host(c->dev, c->h_check);
    if (c->h_keyraw) { memset(c->h_keyraw, 0, 128); svc_free_host(c->dev, c->h_keyraw); }
    if (c->h_key) { memset(c->h_key, 0, sizeof(tsx_gcm_key)); svc_free_host(c->dev, c->h_key); }
    for (auto& e : c->ev) if (e) hipEventDestroy(e);
    for (auto& row : c->sub_ev) for (auto& e : row) if (e) hipEventDestroy(e);
    if (c->st) hipStreamDestroy(c->st);
    if (c->st_in) hipStreamDestroy(c->st_in);
    if (c->st_out) hipStreamDestroy(c->st_out);
    if (c->st_out2) hipStreamDestroy(c->st_out2);
    for (auto& q : c->st_pc) if (q) hipStreamDestroy(q);
    if (c->ev_key) hipEventDestroy(c->ev_key);
}

extern "C" void tsx_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    tsx_device_scope keep;
    for (auto& d : g_devs) {
        for (tsx_ctx* c : d.idle) { ctx_free_device_mem(c); delete c; }
        d.idle.clear(); d.idle_bytes = 0;
        device_free_consts(d);
    }
    g_devs.clear();
    registered_range_forget_all();
    g_version.store(kUninitVersion, std::memory_order_release);
}

// max_out: largest output slot of the batch (detransform: the CRC of the restored bytes runs over dst_cap-sized slots)
static int ctx_reserve(tsx_ctx* c, uint32_t n, uint32_t max_len, uint32_t max_out, uint32_t flags, bool host_mem, size_t in_bytes, size_t out_bytes) {
    HIPCHK(hipSetDevice(c->dev->hip_id));
    if (n > c->descs_cap || !c->d_descs) {
        void* olds[] = {c->d_descs, c->d_gchunks, c->d_status, c->d_zlen};
        for (void* p : olds) svc_free_dev(c->dev, p);
        svc_free_host(c->dev, c->h_descs);
        c->d_descs = nullptr; c->d_gchunks = nullptr; c->d_status = nullptr; c->d_zlen = nullptr; c->h_descs = nullptr; c->hd_descs = nullptr;
        c->descs_cap = 0;                                    // a failure below leaves a context that reallocates, not one with holes
        size_t cap = (size_t)n + n / 4 + 16;
        HIPCHK(hipMalloc((void**)&c->d_descs, cap * sizeof(tsx_chunk_desc)));
        HIPCHK(hipHostMalloc((void**)&c->h_descs, cap * sizeof(tsx_chunk_desc), hipHostMallocMapped | hipHostMallocPortable));
        HIPCHK(hipHostGetDevicePointer((void**)&c->hd_descs, c->h_descs, 0));
        HIPCHK(hipMalloc((void**)&c->d_gchunks, cap * sizeof(tsx_gcm_chunk)));
        HIPCHK(hipMalloc((void**)&c->d_status, cap * sizeof(int32_t)));
        HIPCHK(hipMalloc((void**)&c->d_zlen, cap * sizeof(uint32_t)));
        c->descs_cap = cap;
    }
    // partials: GCM needs 4 u32 per 64 KiB sub-block of the (possibly expanded) stage input, CRC 1 per 256 KiB of the
    // bytes it runs over - the source chunks on the way in, the dst_cap-sized output slots on the way back
    size_t bound = tsx_transformed_bound(max_len, flags & TSX_COMPRESS) + 64;
    size_t subs = (bound + TSX_GCM_SUB_BYTES - 1) / TSX_GCM_SUB_BYTES + 1;
    size_t crc_subs = ((size_t)(max_out > max_len ? max_out : max_len) + TSX_CRC_SUB_BYTES - 1) / TSX_CRC_SUB_BYTES + 1;
    const size_t gcm_words = (flags & TSX_VERIFY_GCM) ? 5 : 4;        // (the GCM verifier keeps a mismatch word per sub-block behind the partial values)
    size_t per_chunk = subs * gcm_words > crc_subs ? subs * gcm_words : crc_subs;
    int rc = grow(c->dev, &c->d_partials, &c->partials_cap, (size_t)n * per_chunk);
    if (rc) return rc;
    c->partials_per_chunk = per_chunk;
    if (host_mem) {
        if ((rc = grow(c->dev, &c->d_in, &c->in_cap, in_bytes + 64))) return rc;
        if ((rc = grow(c->dev, &c->d_out, &c->out_cap, out_bytes + 64))) return rc;
    }
    if (flags & TSX_COMPRESS) {
        size_t stride = (tsx_transformed_bound(max_len, TSX_COMPRESS) + 63) & ~(size_t)63;
        if ((rc = grow(c->dev, &c->d_mid, &c->mid_cap, stride * n))) return rc;
        c->mid_stride = stride;
        size_t zw = tsx_zstd_workspace_bytes(n, max_len);
        uint8_t* zp = (uint8_t*)c->d_zwork;
        rc = grow(c->dev, &zp, &c->zwork_cap, zw);
        c->d_zwork = zp;                                     // also when grow failed: it has freed the old block
        if (rc) return rc;
        if (max_out && dec_use_blocks(n, max_out)) {         // inverse chain, small batch
            const size_t need = tsx_zstd_blockmode_bytes(n, max_out);
            if (!c->d_bwork || c->bwork_cap < need) {
                // a workspace another context left behind (pool_release) before a fresh allocation
                std::lock_guard<std::mutex> lk(g_mu);
                auto& sp = c->dev->spare_bwork;
                for (size_t k = 0; k < sp.size(); k++) if (sp[k].second >= need) {
                    if (c->d_bwork) sp.push_back({c->d_bwork, c->bwork_cap});
                    c->d_bwork = sp[k].first; c->bwork_cap = sp[k].second;
                    sp.erase(sp.begin() + (long)k);
                    break;
                }
            }
            uint8_t* bp = (uint8_t*)c->d_bwork;
            rc = grow(c->dev, &bp, &c->bwork_cap, need);
            c->d_bwork = bp;
            if (rc) { c->d_bwork = nullptr; c->bwork_cap = 0; (void)hipGetLastError(); }   // no room for the fast path: the chunk form decodes the batch
        }
    }
    return TSX_OK;
}

static int ctx_init_device_objects(tsx_ctx* c) {
    HIPCHK(hipSetDevice(c->dev->hip_id));
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->st_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->st_out, hipStreamNonBlocking));
    for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreate(&c->ev_key));
    for (auto& e : c->sub_ev[0]) HIPCHK(hipEventCreate(&e));      // the other rows are created by the first pipelined batch
    HIPCHK(hipMalloc((void**)&c->d_key, sizeof(tsx_gcm_key)));
    HIPCHK(hipMalloc((void**)&c->d_keyraw, 128));
    HIPCHK(hipMalloc((void**)&c->d_segdone, 64));
    // Nothing an allocator left behind: what tsx_debug_key_residue reads, and the completion counters, start from zero.  Copies of pinned
    // zeros on the context's OWN stream - it is non-blocking (a memset on the null stream could land behind the first batch's key copy: seen
    // on the device), and a memset would be a kernel, which waits for a wave slot on a chip full of compressor waves.
    HIPCHK(hipMemcpyAsync(c->d_key, c->dev->h_zeros, sizeof(tsx_gcm_key), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->d_keyraw, c->dev->h_zeros, 128, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->d_segdone, c->dev->h_zeros, 64, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipHostMalloc((void**)&c->h_keyraw, 128, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void**)&c->h_key, sizeof(tsx_gcm_key), hipHostMallocMapped | hipHostMallocPortable));
    HIPCHK(hipHostGetDevicePointer((void**)&c->hd_key, c->h_key, 0));
    HIPCHK(hipHostMalloc((void**)&c->h_segflag, 64, hipHostMallocMapped | hipHostMallocPortable));
    HIPCHK(hipHostGetDevicePointer((void**)&c->hd_segflag, c->h_segflag, 0));
    memset(c->h_segflag, 0, 64);
    HIPCHK(hipStreamSynchronize(c->st));                                // (the counters are zero before a wave of the service can touch them)
    return TSX_OK;
}

extern "C" int tsx_ctx_create(int device_index, uint32_t max_chunks, uint32_t max_chunk_size, tsx_ctx** out) {
    if (!out) return TSX_E_INVAL;
    tsx_device* dev;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (g_devs.empty()) { snprintf(g_last_err, sizeof g_last_err, "tsx_init has not succeeded"); return TSX_E_DEVICE; }
        if (device_index < 0 || device_index >= (int)g_devs.size()) return TSX_E_INVAL;
        dev = &g_devs[device_index];
    }
    tsx_ctx* c = new (std::nothrow) tsx_ctx;
    if (!c) return TSX_E_NOMEM;
    tsx_device_scope keep;
    c->dev_index = device_index; c->dev = dev;
    // a new context zeroes a few device words with small copies (blit kernels of the runtime): like a fetch, it asks guest waves for room
    svc_foreground_begin(dev);
    int rc = ctx_init_device_objects(c);
    svc_foreground_end(dev, false);
    if (rc == TSX_OK && max_chunks && max_chunk_size) rc = ctx_reserve(c, max_chunks, max_chunk_size, max_chunk_size, 0, false, 0, 0);
    if (rc) { ctx_free_device_mem(c); delete c; return rc; }     // a half-built context leaves nothing behind
    *out = c;
    return TSX_OK;
}

extern "C" void tsx_ctx_destroy(tsx_ctx* c) {
    if (!c) return;
    tsx_device_scope keep;
    ctx_free_device_mem(c);
    delete c;
}

extern "C" int tsx_ctx_timing(const tsx_ctx* c, tsx_timing* out) {
    if (!c || !out) return TSX_E_INVAL;
    *out = c->timing;
    return TSX_OK;
}

extern "C" int tsx_ctx_records(const tsx_ctx* c, tsx_records_info* out) {
    if (!c || !out) return TSX_E_INVAL;
    *out = c->records;
    return TSX_OK;
}

extern "C" int tsx_ctx_device(const tsx_ctx* c) { return c ? c->dev_index : TSX_E_INVAL; }

// ---- ctx-less calls: which device, which pooled context ---------------------------------------------
// One JVM per broker drives ALL GPUs of the node from >= 10 RLM threads plus the ChunkCache pool (README.md:218-222,
// RemoteStorageManager.java:212): a ctx-less call goes to the device its thread asked for (tsx_set_thread_device: the JVM side
// passes segment hash % devices, SURVEY 8e "segment s -> GPU s mod N"), otherwise to the device with the fewest batches in
// flight (ties broken round-robin).
extern "C" int tsx_set_thread_device(int device_index) {
    if (device_index >= 0) {
        std::lock_guard<std::mutex> lk(g_mu);
        if (device_index >= (int)g_devs.size()) return TSX_E_INVAL;
    }
    t_dev_hint = device_index < 0 ? -1 : device_index;
    return TSX_OK;
}

extern "C" int tsx_pool_stats(int device_index, uint32_t* idle, uint32_t* in_use, uint64_t* batches) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (device_index < 0 || device_index >= (int)g_devs.size()) return TSX_E_INVAL;
    if (idle) *idle = (uint32_t)g_devs[device_index].idle.size();
    if (in_use) *in_use = g_devs[device_index].in_use;
    if (batches) *batches = g_devs[device_index].batches;
    return TSX_OK;
}

static size_t ctx_workspace_bytes(const tsx_ctx* c) {
    return c->descs_cap * (sizeof(tsx_chunk_desc) + sizeof(tsx_gcm_chunk) + 8) + c->partials_cap * 4 + c->in_cap + c->out_cap + c->mid_cap + c->zwork_cap + c->bwork_cap;
}

static tsx_ctx* pool_acquire(int* rc) {
    int di = -1;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const int nd = (int)g_devs.size();
        if (nd == 0) { snprintf(g_last_err, sizeof g_last_err, "tsx_init has not succeeded"); *rc = TSX_E_DEVICE; return nullptr; }
        if (t_dev_hint >= 0 && t_dev_hint < nd) di = t_dev_hint;
        else {
            const int first = (int)(g_rr++ % (uint32_t)nd);
            di = first;
            for (int k = 1; k < nd; k++) { const int j = (first + k) % nd; if (g_devs[j].in_use < g_devs[di].in_use) di = j; }
        }
        tsx_device& d = g_devs[di];
        d.in_use++; d.batches++;
        if (!d.idle.empty()) { tsx_ctx* c = d.idle.back(); d.idle.pop_back(); d.idle_bytes -= ctx_workspace_bytes(c); return c; }
    }
    tsx_ctx* c = nullptr;
    *rc = tsx_ctx_create(di, 0, 0, &c);
    if (*rc) { std::lock_guard<std::mutex> lk(g_mu); g_devs[di].in_use--; return nullptr; }
    c->pooled = true;
    return c;
}
// Idle pooled contexts of a device give their memory back (an allocation has just failed: what is cached must not be the reason).  The
// service is paused meanwhile: a free only happens with its kernel gone.
static bool pool_drain(tsx_device* dev) {
    std::vector<tsx_ctx*> dead;
    std::vector<std::pair<void*, size_t>> spare;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        dead.swap(dev->idle); dev->idle_bytes = 0;
        spare.swap(dev->spare_bwork);
    }
    if (dead.empty() && spare.empty()) return false;
    tsx_device_scope keep;
    svc_pause(dev);
    for (tsx_ctx* c : dead) { ctx_free_device_mem(c); delete c; }
    for (auto& b : spare) { hipSetDevice(dev->hip_id); (void)hipFree(b.first); }
    svc_resume(dev);
    return true;
}
int reserve_or_drain(tsx_ctx* c, uint32_t n, uint32_t max_len, uint32_t max_out, uint32_t flags, bool host_mem, size_t in_bytes, size_t out_bytes) {
    int rc = ctx_reserve(c, n, max_len, max_out, flags, host_mem, in_bytes, out_bytes);
    if (rc != TSX_E_NOMEM) return rc;
    (void)hipGetLastError();
    if (!pool_drain(c->dev)) return rc;                                 // nothing was cached: the device really is full
    return ctx_reserve(c, n, max_len, max_out, flags, host_mem, in_bytes, out_bytes);
}
static void pool_release(tsx_ctx* c) {
    void* surplus = nullptr;
    tsx_device* const dev = c->dev;
    {
        std::unique_lock<std::mutex> lk(g_mu);
        tsx_device& d = *c->dev;
        d.in_use--;
        if (c->d_bwork) {
            // the fetch side's ForkJoinPool issues from dozens of threads (ChunkCache.java:140): without a bound every idle context would
            // park a block-form workspace.  Beyond a few, the workspace leaves its context for the device's spare list - the next small fetch
            // on a context without one takes it from there (ctx_reserve).  Never a hipFree here: that call waits for every stream of the
            // device, i.e. for second-long compressor waves, on the path of a fetch.
            uint32_t with = 0;
            for (const tsx_ctx* o : d.idle) if (o->d_bwork) with++;
            if (with >= TSX_POOL_MAX_IDLE_BWORK) {
                if (d.spare_bwork.size() < TSX_POOL_MAX_IDLE_BWORK) d.spare_bwork.push_back({c->d_bwork, c->bwork_cap});
                else surplus = c->d_bwork;                               // freed when the service kernel is gone (svc_free_dev), not here
                c->d_bwork = nullptr; c->bwork_cap = 0;
            }
        }
        const size_t b = ctx_workspace_bytes(c);
        if (d.idle.size() < TSX_POOL_MAX_IDLE && (d.idle.empty() || d.idle_bytes + b <= d.idle_cap)) { d.idle.push_back(c); d.idle_bytes += b; c = nullptr; }
    }
    tsx_device_scope keep;
    if (surplus) { hipSetDevice(dev->hip_id); svc_free_dev(dev, surplus); }
    if (!c) return;
    ctx_free_device_mem(c);                                            // a burst of callers does not pin its workspaces forever
    delete c;
}

// ZSTD_compressBound(n) = n + (n >> 8) + (n < 128 KiB ? ((128 KiB - n) >> 11) : 0)
extern "C" size_t tsx_transformed_bound(size_t n, uint32_t flags) {
    size_t m = n;
    if (flags & TSX_COMPRESS) m = n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
    if (flags & TSX_ENCRYPT) m += 28;
    return m;
}

static int with_ctx(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src, size_t src_size, void* dst,
                    size_t dst_size, int mem_kind, int mode, tsx_rec_stream* rs = nullptr) {
    if (ctx) return run_batch(ctx, params, descs, n, src, src_size, dst, dst_size, mem_kind, mode, false, rs);
    int rc = TSX_OK;
    tsx_ctx* c = pool_acquire(&rc);
    if (!c) return rc;
    rc = run_batch(c, params, descs, n, src, src_size, dst, dst_size, mem_kind, mode, true, rs);
    pool_release(c);
    return rc;
}

extern "C" int tsx_transform_batch(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src,
                                   size_t src_size, void* dst, size_t dst_size, int mem_kind) {
    return with_ctx(ctx, params, descs, n, src, src_size, dst, dst_size, mem_kind, 0);
}

// ---- TSX_VALIDATE_RECORDS over several calls.  The state is the caller's memory: it is copied in, every number of it checked, worked on,
// and copied back only when the whole call has succeeded - a negative return leaves it bit for bit as it was.
extern "C" int tsx_records_begin(tsx_records_state* st, uint64_t stream_bytes) {
    if (!st) return TSX_E_INVAL;
    tsx_rec_stream s;
    memset(&s, 0, sizeof s);
    s.magic = TSX_REC_STATE_MAGIC; s.total = stream_bytes; s.first_bad_pos = ~0ull;
    memcpy(st, &s, sizeof s);
    return TSX_OK;
}

extern "C" int tsx_transform_batch_stream(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src,
                                          size_t src_size, void* dst, size_t dst_size, int mem_kind, tsx_records_state* st) {
    if (!st) return TSX_E_INVAL;
    // the records of a batch that is open across two calls cannot be walked without keeping the batch: not built.  Refused before a
    // context, the state or a descriptor is looked at.
    if (params && (params->flags & TSX_VALIDATE_FRAMES)) return TSX_E_UNSUPPORTED;
    tsx_rec_stream s;
    memcpy(&s, st, sizeof s);
    if (!tsx_records_state_ok(&s)) return TSX_E_INVAL;
    const int rc = with_ctx(ctx, params, descs, n, src, src_size, dst, dst_size, mem_kind, 0, &s);
    if (rc >= 0) memcpy(st, &s, sizeof s);
    return rc;
}

extern "C" int tsx_records_result(const tsx_records_state* st, tsx_records_info* out) {
    if (!st || !out) return TSX_E_INVAL;
    tsx_rec_stream s;
    memcpy(&s, st, sizeof s);
    if (!tsx_records_state_ok(&s)) return TSX_E_INVAL;
    memset(out, 0, sizeof *out);
    out->batches = s.batches; out->compressed_batches = s.compressed; out->first_bad_pos = s.first_bad_pos; out->first_bad_reason = s.first_bad_reason;
    out->repaired_chunks = s.repaired; out->ms = s.ms;
    return s.consumed == s.total ? 1 : 0;
}

extern "C" int tsx_detransform_batch(tsx_ctx* ctx, const tsx_batch_params* params, tsx_chunk_desc* descs, uint32_t n, const void* src,
                                     size_t src_size, void* dst, size_t dst_size, int mem_kind) {
    return with_ctx(ctx, params, descs, n, src, src_size, dst, dst_size, mem_kind, 1);
}

extern "C" int tsx_crc32c_batch(tsx_ctx* ctx, tsx_chunk_desc* descs, uint32_t n, const void* src, size_t src_size, int mem_kind) {
    return with_ctx(ctx, nullptr, descs, n, src, src_size, nullptr, 0, mem_kind, 2);
}

// Test hook (not part of the ABI in include/tsxform.h): OR of every byte of the context's key material on the device - 0 after
// any batch, whatever its outcome.
extern "C" int tsx_debug_key_residue(tsx_ctx* c) {
    if (!c) return TSX_E_INVAL;
    tsx_device_scope keep;
    if (hipSetDevice(c->dev->hip_id) != hipSuccess) return TSX_E_DEVICE;
    std::vector<uint8_t> h(sizeof(tsx_gcm_key) + 128);
    if (hipMemcpy(h.data(), c->d_key, sizeof(tsx_gcm_key), hipMemcpyDeviceToHost) != hipSuccess) return TSX_E_DEVICE;
    if (hipMemcpy(h.data() + sizeof(tsx_gcm_key), c->d_keyraw, 128, hipMemcpyDeviceToHost) != hipSuccess) return TSX_E_DEVICE;
    int acc = 0;
    for (uint8_t b : h) acc |= b;
    for (size_t i = 0; i < sizeof(tsx_gcm_key); i++) acc |= ((const uint8_t*)c->h_key)[i];
    return acc;
}

// Test hooks (not part of the ABI): members the context's last compressing batch went as; whether its waves wrote into the caller's buffer.
extern "C" int tsx_debug_last_members(tsx_ctx* c) { return c ? (int)c->last_members : TSX_E_INVAL; }
extern "C" int tsx_debug_last_zero_copy(tsx_ctx* c) { return c ? (int)c->last_zero_copy : TSX_E_INVAL; }
// Test hook (not part of the ABI): which way the chunks of the context's last verifying batch were verified - judged by the block form
// (passed or failed there), or decoded in full (phase two)
extern "C" int tsx_debug_verify_counts(tsx_ctx* c, uint32_t* block_form, uint32_t* fallback) {
    if (!c) return TSX_E_INVAL;
    if (block_form) *block_form = c->verify_block_form;
    if (fallback) *fallback = c->verify_fallback;
    return TSX_OK;
}

// Test hook (not part of the ABI): how many of the first n chunks of the context's LAST detransform batch were decoded by the
// block-parallel form (the rest went through the chunk-serial kernel); -1 when that batch did not use the form at all.
// test hook: how many idle pooled contexts of a device hold a block-form decoder workspace (bounded by TSX_POOL_MAX_IDLE_BWORK)
extern "C" int tsx_debug_pool_bwork(int device_index) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (device_index < 0 || device_index >= (int)g_devs.size()) return TSX_E_INVAL;
    int k = 0;
    for (const tsx_ctx* c : g_devs[device_index].idle) if (c->d_bwork) k++;
    return k;
}
// test hook: block-form decoder launches of the context's last batch (> 1: the batch was cut into co-resident pieces)
extern "C" int tsx_debug_blockmode_pieces(tsx_ctx* c) { return c ? (int)c->blk_pieces.size() : TSX_E_INVAL; }
extern "C" int tsx_debug_blockmode_chunks(tsx_ctx* c, uint32_t n) {
    if (!c) return TSX_E_INVAL;
    if (!c->d_bwork || !c->last_used_blocks) return -1;
    tsx_device_scope keep;
    if (hipSetDevice(c->dev->hip_id) != hipSuccess) return TSX_E_DEVICE;
    int cnt = 0;
    for (const auto& pc : c->blk_pieces) {                              // every launch of the batch laid its chunks' headers out for itself
        uint32_t stride = 0;
        const uint32_t* skip = tsx_zstd_blockmode_skip((const uint8_t*)c->d_bwork + tsx_zstd_blockmode_bytes(pc.first, c->last_max_out), &stride);
        for (uint32_t i = 0; i < pc.second && pc.first + i < n; i++) {
            uint32_t w = 0;
            if (hipMemcpy(&w, skip + (size_t)i * stride, 4, hipMemcpyDeviceToHost) != hipSuccess) return TSX_E_DEVICE;
            cnt += w == 1;
        }
    }
    return cnt;
}

// Pins a caller buffer that will be used for TSX_MEM_HOST / TSX_MEM_HOST_PACKED batches again and again (the JVM side registers its
// per-thread direct ByteBuffers once): copies from / to it go by DMA and overlap fully instead of being staged by the runtime, and
// compressing batches write their output straight into it (zero-copy output: the registered extent is what the device may touch).
// Portable: the pinning holds for every device of the node, whichever one the pool picks for a batch.
extern "C" int tsx_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return TSX_E_INVAL;
    { std::lock_guard<std::mutex> lk(g_mu); if (g_devs.empty()) return TSX_E_DEVICE; }
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) { tsx_set_err("hipHostRegister", e); (void)hipGetLastError(); return TSX_E_DEVICE; }
    registered_range_add(p, bytes);
    return TSX_OK;
}
extern "C" int tsx_host_unregister(void* p) {
    if (!p) return TSX_E_INVAL;
    registered_range_remove(p);
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { tsx_set_err("hipHostUnregister", e); (void)hipGetLastError(); return TSX_E_DEVICE; }
    return TSX_OK;
}

// ---- device memory helpers -------------------------------------------------------------------------
static int set_dev(int device_index, tsx_device** dev = nullptr) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (device_index < 0 || device_index >= (int)g_devs.size()) return TSX_E_INVAL;
    if (dev) *dev = &g_devs[device_index];
    return hipSetDevice(g_devs[device_index].hip_id) == hipSuccess ? TSX_OK : TSX_E_DEVICE;
}
extern "C" int tsx_device_malloc(int device_index, size_t bytes, void** out) {
    if (!out) return TSX_E_INVAL;
    tsx_device_scope keep;
    int rc = set_dev(device_index); if (rc) return rc;
    return hipMalloc(out, bytes) == hipSuccess ? TSX_OK : TSX_E_NOMEM;
}
extern "C" int tsx_device_free(int device_index, void* p) {
    tsx_device_scope keep;
    tsx_device* dev = nullptr;
    int rc = set_dev(device_index, &dev); if (rc) return rc;
    svc_free_dev(dev, p);                                               // (given back when the compressor service's kernel is gone: a free waits for every stream)
    return TSX_OK;
}
// (copies of pageable memory and small copies run as kernels of the runtime: guest waves make room for them as for a fetch)
extern "C" int tsx_memcpy_h2d(int device_index, void* d, const void* s, size_t bytes) {
    tsx_device_scope keep;
    tsx_device* dev = nullptr;
    int rc = set_dev(device_index, &dev); if (rc) return rc;
    svc_foreground_begin(dev);
    const hipError_t e = hipMemcpy(d, s, bytes, hipMemcpyHostToDevice);
    svc_foreground_end(dev, false);
    return e == hipSuccess ? TSX_OK : TSX_E_DEVICE;
}
extern "C" int tsx_memcpy_d2h(int device_index, void* d, const void* s, size_t bytes) {
    tsx_device_scope keep;
    tsx_device* dev = nullptr;
    int rc = set_dev(device_index, &dev); if (rc) return rc;
    svc_foreground_begin(dev);
    const hipError_t e = hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost);
    svc_foreground_end(dev, false);
    return e == hipSuccess ? TSX_OK : TSX_E_DEVICE;
}
