// The compressor service, host side (device side: svc_dev.h and zstd_service_kernel in zstd_enc.hip; layout: tsx_internal.h).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <thread>
#include <stdio.h>
#include <string.h>

#include "tsx_service.h"

// Rounds 2-4 launched one compressor kernel per batch (or per group of callers: the "launch combiner") and let the hardware's
// dispatcher hand workgroups to freed wave slots.  Two things followed from a launch being the unit of work: the chip ran in
// generations (a batch's stragglers held its hardware queue while slots sat empty; 18.0 GiB/s in a timed region against 18.7-20.4
// continuously fed), and everything that is not a compressor wave starved - a freed 6.7 KB slot is refilled by the dispatcher before a
// decoder workgroup finds three neighbouring ones: a fetch under upload load took 1-65 s (profiles/r04_mixed_load.txt).  Now a
// compressing batch is a MEMBER of its device's queue: tickets in pinned memory, persistent waves that pull them, per-member completion
// flags.  One kernel, on one stream that carries nothing else; it is (re)started by whoever publishes work and finds it gone, and by
// the waiting callers' watchdog (a launch that ended - idle, age limit, every wave on a reserved CU - with tickets still unserved).
struct tsx_svc_member { uint64_t id; uint32_t first, n; uint16_t slot; bool done; const uint32_t* h_flag; };
struct tsx_service {
    std::mutex mu; std::condition_variable cv;
    tsx_svc_host* h = nullptr; tsx_svc_host* hd = nullptr;          // the queue in pinned host memory: host view, device alias
    tsx_svc_dev* d = nullptr;
    uint32_t* h_zero = nullptr;                                      // pinned zero word (resets of device words travel as copies, not kernels)
    hipStream_t st = nullptr;                                        // the service kernel's stream: launches only - no events, no copies while it runs
    uint32_t launch_id = 0;                                          // id of the last launch made
    bool launched = false;                                           // a launch is out whose end this side has not seen yet
    bool stop_dirty = false;                                         // the device's stop word must be cleared in front of the next launch
    uint32_t paused = 0;                                             // > 0: no launches (memory management in progress)
    uint32_t grid = 0, cu_keys = 0, cus = 0, cus_reserved = 0, waves_per_cu = 0, resident = 0, engines = 0;
    uint32_t published = 0;
    uint64_t next_id = 1;
    std::deque<tsx_svc_member> out;                                  // members published and not yet retired, oldest first
    std::vector<uint16_t> free_slots; uint16_t slot_gen[TSX_SVC_MEMBERS] = {0};
    uint64_t launches = 0, watchdog_launches = 0, members = 0, chunks = 0, rotations = 0; double kernel_ms = 0;
    bool rotating = false;                                           // a waiting fetch has asked the running launch to end (svc_rotate)
    // The reservation follows the traffic.  "Foreground" = every batch that runs ordinary kernels (fetches above all): while one is in flight,
    // and for fetch_quiet_ms after the last one, tsx_svc_host.yield is raised - guest waves on the reserved CUs hand their chunks back and
    // leave (<= one block of their chunk later, ~30 ms), launches made meanwhile leave the reserved CUs alone.  A device that only uploads
    // compresses on every CU.
    std::atomic<uint32_t> fg_inflight{0};
    std::atomic<int64_t> fg_last_ns{INT64_MIN / 2};                  // steady clock at the end of the last foreground batch
    uint64_t guest_launches = 0;
    // Guests come in launches of their own, next to the launch they help (tsx_svc_launch.guest_launch): on a second stream of the lowest priority
    hipStream_t st_g = nullptr;
    uint32_t g_launch_id = 0; bool g_launched = false; int64_t g_last_ns = INT64_MIN / 2;
    int64_t launch_ns = 0;                                           // steady clock at the last launch of the service kernel itself
    std::vector<void*> deferred_dev, deferred_host;                  // frees that wait for the kernel to be gone (svc_free_*)
};
void tsx_service_delete::operator()(tsx_service* s) const { delete s; }

// ---- the service's time constants (device ticks are 10 ns: the 100 MHz clock every CU shares) ---------------------------------------------
// (the rotation's 200 ms are SVC_ROTATE_AFTER_MS, tsx_service.h; the 50 ms a calibration wave stays at most are SVC_CALIBRATE_CAP_TICKS, svc_dev.h;
//  svc_idle_exit_us and svc_max_launch_ms are configuration, tsx_host.h)
static const uint32_t kPollTicks = 500;                  // one look at the host's words per 5 us, device-wide
static const uint32_t kGuestIdleTicks = 1000000;         // 10 ms: a guest that has found the queue dry for this long leaves (callers that resubmit at once leave it dry for 2 - 3 ms)
static const int64_t kGuestDelayNs = 3000000;            // guests not before the launch they are to help has arrived: its workgroups take a moment to be placed (~0.5 ms on a cold
                                                         // chip), and a guest that finds a free slot anywhere but on a reserved CU takes it - and leaves (measured: guests launched 1 ms
                                                         // behind their launch, 41 of 768 stayed)
static const int64_t kGuestRetryNs = 20000000;           // a guest launch whose workgroups all left at once is tried again 20 ms later
#ifdef HIPEMU
static const uint32_t kCalibrateTicks = 50000;           // (the CPU harness runs the workgroups one after the other: each waits its window out)
#else
static const uint32_t kCalibrateTicks = 200000;          // calibration waves leave when nobody has arrived for 2 ms (svc_create says why not less)
#endif

// ---- service: whose turn the reserved CUs are ----------------------------------------------------------------------------------------
static int64_t steady_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// A batch of ordinary kernels begins / is over (no lock: this is the fetch path).  The counter first, the word second - svc_launch_locked
// clears the word first and looks at the counter second, so one of the two always sees the other.
void svc_foreground_begin(tsx_device* dev) {
    if (!dev->svc) return;
    dev->svc->fg_inflight.fetch_add(1, std::memory_order_seq_cst);
    __atomic_store_n(&dev->svc->h->yield, 1u, __ATOMIC_SEQ_CST);
}
// traffic = false: something that only needed room while it ran (a new context's first small copies, a helper copy) - it does not count as
// a fetch having been seen: the next member published finds the device as quiet as it was before (svc_note_quiet_locked)
void svc_foreground_end(tsx_device* dev, bool traffic) {
    if (!dev->svc) return;
    if (traffic) dev->svc->fg_last_ns.store(steady_ns(), std::memory_order_seq_cst);
    dev->svc->fg_inflight.fetch_sub(1, std::memory_order_seq_cst);
}
static bool svc_quiet(const tsx_service& s) {
    return g_cfg.fetch_quiet_ms != 0 && s.fg_inflight.load(std::memory_order_seq_cst) == 0 &&
           steady_ns() - s.fg_last_ns.load(std::memory_order_seq_cst) > (int64_t)g_cfg.fetch_quiet_ms * 1000000;
}

// A member is about to be published (mu held): the yield word follows the device's quietness - down when no fetch has been seen for fetch_quiet_ms
// (word first, counter second: svc_foreground_begin does it the other way round, one of the two sees the other), up otherwise.  Guests read it, and
// so does a wave of the launch itself that the hardware's scheduler has restored onto a reserved CU: on a quiet device it finishes its chunk there.
static void svc_note_quiet_locked(tsx_service& s) {
    if (!s.cus_reserved) return;
    if (svc_quiet(s)) {
        if (__atomic_load_n(&s.h->yield, __ATOMIC_SEQ_CST) == 0u) return;
        __atomic_store_n(&s.h->yield, 0u, __ATOMIC_SEQ_CST);
        if (s.fg_inflight.load(std::memory_order_seq_cst) != 0) __atomic_store_n(&s.h->yield, 1u, __ATOMIC_SEQ_CST);
    } else if (__atomic_load_n(&s.h->yield, __ATOMIC_SEQ_CST) == 0u) __atomic_store_n(&s.h->yield, 1u, __ATOMIC_SEQ_CST);      // (fetch_quiet_ms was changed under a lowered word)
}

// ---- service: lifetime ------------------------------------------------------------------------------------------------------------------
// Which kernels of the service are still out - the launch, its guests?  (mu held.)  When an end is seen for the first time, the launch's
// duration joins the statistics, and once nothing is alive what waited for that is freed: hipFree / hipHostFree wait for EVERY stream of
// the device, i.e. for a kernel that lives as long as uploads go on - nothing in this library frees device or pinned memory while that
// kernel may be running (svc_free_*).  The launch's last wave says so itself (tsx_svc_host.ended_launch): nothing is queued behind the
// kernel that could be asked.
// .main: whoever starts, rotates or watches the launch.  .any(): what must not free memory, or must wait for the device to be the caller's alone.
struct svc_out { bool main, guests; bool any() const { return main || guests; } };
static svc_out svc_harvest_locked(tsx_service& s) {
    if (s.launched && __atomic_load_n(&s.h->ended_launch, __ATOMIC_ACQUIRE) == s.launch_id) {
        s.kernel_ms += (double)(s.h->t_last - s.h->t_first) / 1e5;       // 100 MHz ticks
        s.launched = false;
        // a rotation is over with the launch it asked to end - also when a pause overlapped that end (the flag must not survive into the next
        // launch: svc_rotate would stay switched off for its whole life); only the host's stop word stays up while paused
        if (s.rotating) { s.rotating = false; if (!s.paused) __atomic_store_n(&s.h->stop, 0u, __ATOMIC_RELEASE); }   // (the device's copy of the word is cleared in front of the next launch)
    }
    if (s.g_launched && __atomic_load_n(&s.h->g_ended_launch, __ATOMIC_ACQUIRE) == s.g_launch_id) s.g_launched = false;
    if (!s.launched && !s.g_launched) {                                  // (nothing of the service is alive)
        for (void* p : s.deferred_dev) (void)hipFree(p);
        for (void* p : s.deferred_host) (void)hipHostFree(p);
        s.deferred_dev.clear(); s.deferred_host.clear();
    }
    return {s.launched, s.g_launched};
}

// The arguments of a launch of the service kernel itself, or of a launch of guests next to it (mu held).
static tsx_svc_launch svc_launch_args(const tsx_service& s, bool guest_launch) {
    const uint32_t gwaves = s.cus_reserved * s.waves_per_cu;
    tsx_svc_launch a{};
    a.launch_id = (guest_launch ? s.g_launch_id : s.launch_id) + 1;
    a.sched = g_cfg.zstd_sched;
    a.poll_ticks = kPollTicks; a.idle_exit_ticks = g_cfg.svc_idle_exit_us * 100u; a.guest_idle_ticks = kGuestIdleTicks;
#ifdef HIPEMU
    a.poll_ticks = 0; a.idle_exit_ticks = 0; a.guest_idle_ticks = 0;     // blocks run one after the other: nobody to wait for
#endif
    const uint64_t age = (uint64_t)g_cfg.svc_max_launch_ms * 100000ull;
    a.max_age_ticks_lo = (uint32_t)age; a.max_age_ticks_hi = (uint32_t)(age >> 32);
    if (guest_launch) {
        a.guest_launch = 1; a.guests = 1;
        a.spread_cus = 0;                                                // (guests exist because everybody else is busy: nothing to spread)
        a.main_waves = s.grid > gwaves ? s.grid - gwaves : s.grid;
    } else {
        a.keep_waves = g_cfg.svc_keep_waves;
        a.spread_cus = s.cus > s.cus_reserved ? s.cus - s.cus_reserved : s.cus;
    }
    return a;
}

// Start the service kernel (mu held, kernel known to be gone, device current).
static int svc_launch_locked(tsx_service& s) {
    if (s.paused) return TSX_OK;                                        // whoever paused the service starts it again (svc_resume)
    if (s.stop_dirty) {
        HIPCHK(hipMemcpyAsync(&s.d->stop, s.h_zero, 4, hipMemcpyHostToDevice, s.st));
        s.stop_dirty = false;
    }
    tsx_svc_launch a = svc_launch_args(s, false);
#ifdef HIPEMU
    // (the CPU harness runs one kernel at a time, its blocks one after the other: guests are part of the launch there, which is how its tests reach
    //  the guests' code; on the device they come in launches of their own - svc_try_guests_locked)
    if (s.cus_reserved && svc_quiet(s)) {
        __atomic_store_n(&s.h->yield, 0u, __ATOMIC_SEQ_CST);             // word first, counter second (svc_foreground_begin)
        if (s.fg_inflight.load(std::memory_order_seq_cst) != 0) __atomic_store_n(&s.h->yield, 1u, __ATOMIC_SEQ_CST);
        else a.guests = 1;
    }
#endif
    (void)hipGetLastError();
    tsx_launch_zstd_service(s.st, s.hd, s.d, s.grid, a);
    if (hipGetLastError() != hipSuccess) { tsx_set_errmsg("launch of the compressor service kernel failed"); return TSX_E_DEVICE; }
    s.launch_id = a.launch_id;
    s.launched = true; s.launches++; s.guest_launches += a.guests ? 1u : 0u;
    s.launch_ns = steady_ns();
    return TSX_OK;
}

// Guests (mu held, device current): a launch of as many one-wave workgroups as the reserved CUs hold, made when the running launch has more chunks
// queued than waves, no fetch has been seen for fetch_quiet_ms and no guests are out.  With every other slot of the chip taken the workgroups land
// on the reserved CUs; one that lands elsewhere (the main launch is still arriving, or the chip is not full after all) leaves at once, and so does
// every guest that finds the queue dry for ten milliseconds (callers that resubmit as soon as their batches complete leave the queue dry for 2 - 3 ms between
// two rounds: the guests stay through that) - so guests are there exactly while the chip is full AND busy, the one regime in which a
// chip without a free slot works well (profiles/r06_full_chip_with_idle_waves.txt).  The next fetch raises the yield word: they hand their chunks
// back and leave (tsx_svc_host.yield).
static void svc_try_guests_locked(tsx_service& s) {
#ifndef HIPEMU
    if (!s.cus_reserved || !g_cfg.fetch_quiet_ms || s.paused || s.rotating || !s.launched || !s.st_g) return;
    if (svc_harvest_locked(s).guests || !svc_quiet(s)) return;
    const int64_t now = steady_ns();
    if (now - s.g_last_ns < kGuestRetryNs || now - s.launch_ns < kGuestDelayNs) return;
    uint64_t outstanding = 0;
    for (const auto& m : s.out) if (!m.done && !__atomic_load_n(m.h_flag, __ATOMIC_ACQUIRE)) outstanding += m.n;
    const uint32_t gwaves = s.cus_reserved * s.waves_per_cu;
    if (outstanding <= (uint64_t)(s.grid > gwaves ? s.grid - gwaves : s.grid)) return;     // every queued chunk has a wave of the launch itself
    s.g_last_ns = now;
    __atomic_store_n(&s.h->yield, 0u, __ATOMIC_SEQ_CST);                 // word first, counter second (svc_foreground_begin)
    if (s.fg_inflight.load(std::memory_order_seq_cst) != 0) { __atomic_store_n(&s.h->yield, 1u, __ATOMIC_SEQ_CST); return; }
    const tsx_svc_launch a = svc_launch_args(s, true);
    (void)hipGetLastError();
    tsx_launch_zstd_service(s.st_g, s.hd, s.d, gwaves, a);
    if (hipGetLastError() != hipSuccess) return;                         // (no guests this time)
    s.g_launch_id = a.launch_id; s.g_launched = true; s.guest_launches++;
#else
    (void)s;
#endif
}

void svc_destroy(tsx_device& d) {
    if (!d.svc) return;
    tsx_service& s = *d.svc;
    if (s.h) __atomic_store_n(&s.h->stop, 1u, __ATOMIC_RELEASE);
    if (s.st) { (void)hipStreamSynchronize(s.st); (void)hipStreamDestroy(s.st); }
    if (s.st_g) { (void)hipStreamSynchronize(s.st_g); (void)hipStreamDestroy(s.st_g); }
    for (void* p : s.deferred_dev) (void)hipFree(p);
    for (void* p : s.deferred_host) (void)hipHostFree(p);
    if (s.h) (void)hipHostFree(s.h);
    if (s.h_zero) (void)hipHostFree(s.h_zero);
    if (s.d) (void)hipFree(s.d);
    d.svc.reset();
}

// The queue, the device words and - from a probe launch that covers the chip - the CU keys that exist and the ones the compressor leaves alone.
int svc_create(tsx_device& d, int cus) {
    d.svc.reset(new (std::nothrow) tsx_service);
    if (!d.svc) return TSX_E_NOMEM;
    tsx_service& s = *d.svc;
    HIPCHK(hipHostMalloc((void**)&s.h, sizeof(tsx_svc_host), hipHostMallocMapped | hipHostMallocPortable));
    memset(s.h, 0, sizeof(tsx_svc_host));
    s.h->yield = 1;                                                      // (cleared when a member is published on a quiet device: svc_note_quiet_locked)
    HIPCHK(hipHostGetDevicePointer((void**)&s.hd, s.h, 0));
    HIPCHK(hipHostMalloc((void**)&s.h_zero, 64, hipHostMallocDefault));
    memset(s.h_zero, 0, 64);
    HIPCHK(hipMalloc((void**)&s.d, sizeof(tsx_svc_dev)));
    HIPCHK(hipMemset(s.d, 0, sizeof(tsx_svc_dev)));
    // The service's stream gets the LOWEST stream priority of the device.  Two reasons: the runtime keeps a pool of hardware queues per
    // priority and multiplexes a process's streams onto them - a stream that shared the service's hardware queue would sit behind a kernel
    // that lives as long as uploads go on, and nothing else in this library (or, normally, in the process) creates low-priority streams;
    // and between a compressor wave and a fetch's workgroup that could both be placed, the fetch's goes first.
    {
        int least = 0, greatest = 0;
        if (g_cfg.svc_normal_priority || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest ||
            hipStreamCreateWithPriority(&s.st, hipStreamNonBlocking, least) != hipSuccess) {
            (void)hipGetLastError();
            s.st = nullptr;
            HIPCHK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
        }
    }
    {   // ... and the guests' stream, of the same (lowest) priority: a hardware queue of its own in that pool (a second stream of normal priority would
        // share hardware queues with the fetch side's streams - and a kernel that lives for seconds blocks whatever is queued behind it)
        int least = 0, greatest = 0;
        if (g_cfg.svc_normal_priority || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest ||
            hipStreamCreateWithPriority(&s.st_g, hipStreamNonBlocking, least) != hipSuccess) { (void)hipGetLastError(); s.st_g = nullptr; }     // (no guests then)
    }
    for (uint32_t i = TSX_SVC_MEMBERS; i-- > 0;) s.free_slots.push_back((uint16_t)i);
    // which compute units are there?  (HIP promises nothing about placement: a launch of three 48 KiB workgroups per CU that stay ~30 us each
    // has to spread over all of them; twice, in case the first one met a chip that was busy)
    std::vector<uint32_t> seen(128, 0);
    for (int pass = 0; pass < 2; pass++) {
        (void)hipGetLastError();
        tsx_launch_cu_probe(s.st, s.d, (uint32_t)cus * 3u * 2u);
        HIPCHK(hipStreamSynchronize(s.st));
        HIPCHK(hipMemcpy(seen.data(), s.d->seen, 512, hipMemcpyDeviceToHost));
        uint32_t k = 0; for (uint32_t w : seen) k += (uint32_t)__builtin_popcount(w);
        s.cu_keys = k;
        if ((int)k >= cus) break;
    }
    s.cus = (uint32_t)cus;
    // The reservation: ONE CU OF EVERY SHADER ENGINE first.  The hardware hands a kernel's workgroups to the shader engines in a fixed
    // rotation and a workgroup waits for room in ITS engine: next to waves that stay for seconds, a fetch kernel's workgroup that falls to
    // an engine without a free CU waits until the compressor launch ends (measured: kernels of a fetch each stuck for exactly one service
    // launch, with 8 reserved CUs as well as with a CU mask that kept the service off 8 CUs - profiles/r05_kernel_trace_blocked_fetch.csv.gz,
    // r05_cu_mask_variant_phases.txt).  A key's upper bits name the engine: xcc_id | se_id | sh_id (key >> 4).  Round r takes the r-th
    // highest CU of every engine: the default (0xFFFFFFFF = "one per engine") stops after round 0; a number asked for is spread the same way.
    // Never more than a quarter of the chip, and nothing at all when the probe did not find one key per CU (a key that stood for two CUs
    // would take both).
    std::vector<uint32_t> res(128, 0);
    uint32_t engines = 0;
    for (uint32_t g = 0; g < 256; g++) { bool any = false; for (uint32_t c = 0; c < 16; c++) { const uint32_t key = g << 4 | c; any |= ((seen[key >> 5] >> (key & 31)) & 1) != 0; } engines += any; }
    s.engines = engines;
    uint32_t want = g_cfg.reserved_cus == 0xFFFFFFFFu ? engines : g_cfg.reserved_cus;
    if (want > s.cus / 4) want = s.cus / 4;
    if (s.cu_keys != s.cus) {
        if (g_cfg.debug || want) fprintf(stderr, "[tsxform] device %d: %u CU keys seen for %u compute units - no CU reservation\n", d.hip_id, s.cu_keys, s.cus);
        want = 0;
    }
    uint32_t taken = 0;
    for (uint32_t round = 0; taken < want && round < 16; round++)
        for (uint32_t g = 0; g < 256 && taken < want; g++) {
            uint32_t nth = 0;
            for (int c = 15; c >= 0; c--) {
                const uint32_t key = g << 4 | (uint32_t)c;
                if (!((seen[key >> 5] >> (key & 31)) & 1)) continue;
                if (nth++ == round) { res[key >> 5] |= 1u << (key & 31); taken++; break; }
            }
        }
    s.cus_reserved = taken;
    HIPCHK(hipMemcpy(s.d->reserved, res.data(), 512, hipMemcpyHostToDevice));
    // A launch covers the chip exactly once - never more workgroups than are resident at the same time.  The waves stay for as long as there
    // is work, so workgroups that did not fit would stay PENDING for as long, and a dispatch that is still in progress holds its hardware
    // pipe: the first command of every stream whose queue sat on that pipe did not start until the launch was over.  Measured (gpurun
    // r05a-r05n, profiles/r05_service_resident_waves_and_pending_workgroups.txt): launches of 256 x 24 against the 256 x 21 that fit (the
    // kernel's 6704 bytes of LDS are allocated as 7680) kept 768 workgroups pending, and a fetch issued meanwhile came back when the launch
    // ended - up to its age limit later.
    // How many fit is MEASURED: a launch of 32 workgroups per CU whose waves stay until no workgroup has ARRIVED for 2 ms counts the most that
    // were ever resident at once (registers, LDS with its allocation granularity, scratch slots - whatever limits it; the runtime's occupancy
    // query said 24 where 21 fit).  The window was 500 us for most of round 6: the last few dozen workgroups of such a launch can arrive later
    // than that behind the others (6094 - 6133 resident "measured" on a chip that holds 6144), the division below rounded that down to 23 per
    // CU, and the service ran with 5888 waves instead of 6144 in most processes of some boxes - the "boxes that hold 23": they do not.  With
    // 2 ms every pass sees 6137 - 6144 and the best of the passes is 6144 (four processes of four).  Up to four passes, until the best is a
    // whole number of workgroups per CU twice in a row or at all after the second pass.  tsx_init runs on a device this process is not using yet.
    for (int pass = 0; pass < 4; pass++) {
        // (twice at least: the first launch of a process also loads the code object)
        tsx_svc_launch c{}; c.launch_id = ++s.launch_id; c.calibrate_ticks = kCalibrateTicks;
        (void)hipGetLastError();
        tsx_launch_zstd_service(s.st, s.hd, s.d, s.cus * 32u, c);
        HIPCHK(hipStreamSynchronize(s.st));
        uint32_t lm[2] = {0, 0};
        HIPCHK(hipMemcpy(lm, &s.d->live, 8, hipMemcpyDeviceToHost));
        const uint32_t before = s.resident;
        if (lm[1] > s.resident) s.resident = lm[1];
        HIPCHK(hipMemcpy(&s.d->live_max, s.h_zero, 4, hipMemcpyHostToDevice));
        if (g_cfg.debug) fprintf(stderr, "[tsxform] device %d: calibration launch %d: %u workgroups resident at once\n", d.hip_id, pass, lm[1]);
        if (pass >= 1 && (lm[1] == before || s.resident % s.cus == 0)) break;
    }
    uint32_t per_cu = s.resident / s.cus;
    if (per_cu == 0 || per_cu > 32) per_cu = 16;                        // (a measurement that cannot be: stay on the safe side)
    s.waves_per_cu = per_cu;
    s.grid = s.cus * per_cu;
    return TSX_OK;
}
svc_geometry svc_geometry_of(const tsx_device& d) { return {d.svc->grid, d.svc->cus_reserved, d.svc->cus}; }

// Frees that must not wait for the service kernel: freed at once when it is known to be gone (mu held meanwhile: no launch can begin),
// otherwise when its end is seen (svc_harvest_locked) or at shutdown.
void svc_free_dev(tsx_device* dev, void* p) {
    if (!p) return;
    if (!dev->svc) { (void)hipFree(p); return; }
    std::lock_guard<std::mutex> lk(dev->svc->mu);
    if (svc_harvest_locked(*dev->svc).any()) dev->svc->deferred_dev.push_back(p); else (void)hipFree(p);
}
void svc_free_host(tsx_device* dev, void* p) {
    if (!p) return;
    if (!dev->svc) { (void)hipHostFree(p); return; }
    std::lock_guard<std::mutex> lk(dev->svc->mu);
    if (svc_harvest_locked(*dev->svc).any()) dev->svc->deferred_host.push_back(p); else (void)hipHostFree(p);
}

// Memory management that needs the memory BACK (an allocation has failed): no launches until svc_resume, the running kernel is told to
// stop (its waves leave after their current chunk, <= ~1.3 s), deferred frees happen.  Members that wait meanwhile just wait.
void svc_pause(tsx_device* dev) {
    if (!dev->svc) return;
    tsx_service& s = *dev->svc;
    std::unique_lock<std::mutex> lk(s.mu);
    s.paused++;
    __atomic_store_n(&s.h->stop, 1u, __ATOMIC_RELEASE);
    s.stop_dirty = true;
    while (svc_harvest_locked(s).any()) { lk.unlock(); std::this_thread::sleep_for(std::chrono::microseconds(200)); lk.lock(); }
}
// The safety net of the fetch side.  One CU of every shader engine is kept free for it, and a fetch next to saturating uploads takes its
// ~2 ms - but once in a few hundred fetches (measured: 1 of 271, 2 of 12, 0 of 218 + 218 in four runs) a kernel of a fetch did not start
// until the compressor launch next to it ended, for a reason that was not found.  A batch that has waited for its own kernels for 200 ms
// while the service kernel is alive asks that launch to end: its waves leave after their current chunk (<= ~1.3 s), the waiting callers'
// watchdog starts the next one, and the fetch gets the chip in between.  Cost: one chunk time of a half-empty chip, only when it happens.
void svc_rotate(tsx_device* dev) {
    if (!dev->svc) return;
    tsx_service& s = *dev->svc;
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.rotating || s.paused || !svc_harvest_locked(s).main) return;
    s.rotating = true; s.rotations++;
    __atomic_store_n(&s.h->stop, 1u, __ATOMIC_RELEASE);
    s.stop_dirty = true;
}
void svc_resume(tsx_device* dev) {
    if (!dev->svc) return;
    tsx_service& s = *dev->svc;
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.paused && --s.paused == 0) {
        __atomic_store_n(&s.h->stop, 0u, __ATOMIC_RELEASE);
        if (!s.out.empty() && !svc_harvest_locked(s).main) (void)svc_launch_locked(s);     // (a failure shows up in the waiting members' watchdog)
    }
}

bool svc_busy(tsx_device* dev) {
    tsx_service& s = *dev->svc;
    std::lock_guard<std::mutex> lk(s.mu);
    return svc_harvest_locked(s).main || !s.out.empty();
}

// ---- service: members ---------------------------------------------------------------------------------------------------------------
// Publish one member: `proto` names its buffers (n, done and flag included); its n chunks become the next n tickets.  Returns the member's
// id (for svc_retire) through *id.  Blocks while the ticket ring or the member slots are full (members retire one by one).
int svc_submit(tsx_device* dev, const tsx_zseg& proto, const uint32_t* h_flag, uint64_t* id) {
    tsx_service& s = *dev->svc;
    const uint32_t n = proto.n;
    if (!n || n > TSX_SVC_MEMBER_MAX) return TSX_E_INVAL;
    std::unique_lock<std::mutex> lk(s.mu);
    // room: a ticket record is reused TSX_SVC_TICKETS tickets later - by then every member up to it must be complete ON THE DEVICE (its flag
    // raised; whether its caller has come back for it yet does not matter: a caller that publishes its pieces one after the other must
    // never wait here for a piece of its own that only it can retire)
    for (;;) {
        uint32_t oldest = s.published; bool any = false;
        for (const auto& m : s.out) if (!m.done && !__atomic_load_n(m.h_flag, __ATOMIC_ACQUIRE)) { oldest = m.first; any = true; break; }
        if (!s.free_slots.empty() && (!any || (uint32_t)(s.published + n - oldest) <= TSX_SVC_TICKETS)) break;
        // whoever waits for room is also the service's watchdog (as svc_wait is): the kernel may have ended - idle, age limit, a rotation -
        // with the members that hold the room still unserved, and their callers may all be in here
        if (!s.paused && !s.out.empty() && !svc_harvest_locked(s).main) { s.watchdog_launches++; (void)svc_launch_locked(s); }
        s.cv.wait_for(lk, std::chrono::milliseconds(1));
    }
    svc_note_quiet_locked(s);
    const uint16_t slot = s.free_slots.back(); s.free_slots.pop_back();
    const uint16_t gen = ++s.slot_gen[slot];
    tsx_zseg e = proto;
    e.gen = gen;
    s.h->member[slot] = e;
    const uint32_t first = s.published;
    for (uint32_t i = 0; i < n; i++) { tsx_svc_ticket& t = s.h->ticket[(first + i) & (TSX_SVC_TICKETS - 1)]; t.member_gen = (uint32_t)gen << 16 | slot; t.chunk = i; }
    s.published = first + n;
    __atomic_store_n(&s.h->published, s.published, __ATOMIC_RELEASE);   // the waves' poll picks it up (a few microseconds)
    *id = s.next_id++;
    s.out.push_back({*id, first, n, slot, false, h_flag});
    s.members++;
    if (!svc_harvest_locked(s).main) { const int rc = svc_launch_locked(s); if (rc == TSX_OK) svc_try_guests_locked(s); return rc; }     // (on failure the caller abandons the member: svc_retire)
    svc_try_guests_locked(s);                                           // the queue has just grown: deeper than the launch has waves?  (and quiet?)
    return TSX_OK;
}

// The member is over - completed, or abandoned (`abandon`: its tickets, should a later launch ever reach them, name a stale generation).
void svc_retire(tsx_device* dev, uint64_t id, bool abandon) {
    tsx_service& s = *dev->svc;
    std::lock_guard<std::mutex> lk(s.mu);
    for (auto& m : s.out) if (m.id == id) {
        m.done = true;
        if (abandon) { s.slot_gen[m.slot]++; __atomic_store_n(&s.h->member[m.slot].gen, (uint32_t)s.slot_gen[m.slot], __ATOMIC_RELEASE); }
        else s.chunks += m.n;
        break;
    }
    while (!s.out.empty() && s.out.front().done) { s.free_slots.push_back(s.out.front().slot); s.out.pop_front(); }
    s.cv.notify_all();
}

// Wait for a member's flag.  A chunk takes about a second: short sleeps only while the member is young (tests, tiny chunks), a
// millisecond between looks afterwards - dozens of callers must not burn the cores next to the GPU's NUMA node.  Every look that follows
// a real sleep is also the service's watchdog: a kernel that has ended with this member unfinished is started again.
int svc_wait(tsx_device* dev, uint32_t* h_flag) {
    tsx_service& s = *dev->svc;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t failures = 0;
    for (uint32_t look = 0;; look++) {
        if (__atomic_load_n(h_flag, __ATOMIC_ACQUIRE)) return TSX_OK;
        const auto age = std::chrono::steady_clock::now() - t0;
        const bool young = age < std::chrono::milliseconds(2);
        if (!young || (look & 7) == 7) {
            std::lock_guard<std::mutex> lk(s.mu);
            if (!s.paused && !svc_harvest_locked(s).main) {
                if (__atomic_load_n(h_flag, __ATOMIC_ACQUIRE)) return TSX_OK;
                s.watchdog_launches++;
                if (svc_launch_locked(s) != TSX_OK && ++failures >= 3) return TSX_E_DEVICE;
            } else if (!young) svc_try_guests_locked(s);                // (the callers may all be in here: whoever waits also asks whether guests are due)
        }
        std::this_thread::sleep_for(young ? std::chrono::microseconds(20) : age < std::chrono::milliseconds(50) ? std::chrono::microseconds(250) : std::chrono::microseconds(1000));
    }
}

// Returns when the device's service kernel has ended (its waves leave a moment after the last chunk): measurement tools bracket a timed
// region with it so that the region's chunks and the kernel launches that did them can be set against each other (tsx_service_stats).
extern "C" int tsx_service_quiesce(int device_index) {
    tsx_device* const dev = tsx_device_at(device_index);
    if (!dev) return TSX_E_INVAL;
    tsx_service& s = *dev->svc;
    for (;;) {
        { std::lock_guard<std::mutex> lk(s.mu); if (!svc_harvest_locked(s).any()) return TSX_OK; }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// device words the host copies several of at a time
static_assert(offsetof(tsx_svc_dev, pub) == offsetof(tsx_svc_dev, next) + 4, "next, pub");
static_assert(offsetof(tsx_svc_dev, avail) == offsetof(tsx_svc_dev, fin) + 4, "fin, avail");
static_assert(offsetof(tsx_svc_dev, stat_skipped) == offsetof(tsx_svc_dev, stat_chunks) + 12 && offsetof(tsx_svc_dev, stat_wave_starts) == offsetof(tsx_svc_dev, stat_chunks) + 4 &&
              offsetof(tsx_svc_dev, stat_reserved_exits) == offsetof(tsx_svc_dev, stat_chunks) + 8, "stat_chunks, stat_wave_starts, stat_reserved_exits, stat_skipped");
static_assert(offsetof(tsx_svc_dev, live_max) == offsetof(tsx_svc_dev, live) + 4, "live, live_max");
static_assert(offsetof(tsx_svc_dev, stat_returned) == offsetof(tsx_svc_dev, stat_yields) + 4, "stat_yields, stat_returned");
static_assert(sizeof(tsx_service_info) == 112, "relocated_waves took the struct's tail padding: callers compiled before it hand in 112 bytes too");
extern "C" int tsx_service_stats(int device_index, tsx_service_info* out) {
    if (!out) return TSX_E_INVAL;
    tsx_device* const dev = tsx_device_at(device_index);
    if (!dev) return TSX_E_INVAL;
    tsx_service& s = *dev->svc;
    tsx_device_scope keep;
    if (hipSetDevice(dev->hip_id) != hipSuccess) return TSX_E_DEVICE;
    std::lock_guard<std::mutex> lk(s.mu);
    const bool running = svc_harvest_locked(s).main;
    memset(out, 0, sizeof *out);
    out->launches = s.launches; out->watchdog_launches = s.watchdog_launches; out->rotations = (uint32_t)s.rotations; out->members = s.members; out->chunks = s.chunks;
    out->kernel_ms = s.kernel_ms; out->running = running ? 1u : 0u;
    out->waves = s.grid; out->compute_units = s.cus; out->cu_keys_seen = s.cu_keys; out->reserved_cus = s.cus_reserved; out->shader_engines = s.engines;
    out->guest_launches = (uint32_t)s.guest_launches;      // (readmissions: no launch is asked to end for that any more - 0)
    if (running) {
        // the launch is alive: the words its waves mirror into pinned memory (a copy out of device memory is a blit kernel for sizes like
        // these and, next to guest waves, waits for the launch to end - tsx_internal.h, tsx_svc_host.m_*)
        out->device_chunks = __atomic_load_n(&s.h->m_chunks, __ATOMIC_RELAXED); out->live_waves = __atomic_load_n(&s.h->m_live, __ATOMIC_RELAXED);
        out->live_waves_max = __atomic_load_n(&s.h->m_live_max, __ATOMIC_RELAXED); out->wave_starts = __atomic_load_n(&s.h->m_wave_starts, __ATOMIC_RELAXED);
        out->reserved_exits = __atomic_load_n(&s.h->m_reserved_exits, __ATOMIC_RELAXED); out->skipped_tickets = __atomic_load_n(&s.h->m_skipped, __ATOMIC_RELAXED);
        out->yielded_waves = __atomic_load_n(&s.h->m_yields, __ATOMIC_RELAXED); out->returned_chunks = __atomic_load_n(&s.h->m_returned, __ATOMIC_RELAXED);
        out->relocated_waves = __atomic_load_n(&s.h->m_relocated, __ATOMIC_RELAXED);
        return TSX_OK;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    if (hipMemcpy(w, &s.d->stat_yields, 8, hipMemcpyDeviceToHost) == hipSuccess) { out->yielded_waves = w[0]; out->returned_chunks = w[1]; } else (void)hipGetLastError();
    if (hipMemcpy(w, &s.d->stat_chunks, sizeof w, hipMemcpyDeviceToHost) == hipSuccess) {
        out->device_chunks = w[0]; out->wave_starts = w[1]; out->reserved_exits = w[2]; out->skipped_tickets = w[3];
    } else (void)hipGetLastError();
    if (hipMemcpy(w, &s.d->live, 8, hipMemcpyDeviceToHost) == hipSuccess) { out->live_waves = w[0]; out->live_waves_max = w[1]; } else (void)hipGetLastError();
    if (hipMemcpy(w, &s.d->stat_relocated, 4, hipMemcpyDeviceToHost) == hipSuccess) out->relocated_waves = w[0]; else (void)hipGetLastError();
    return TSX_OK;
}

// Test hook (not part of the ABI): put the device's ticket counters at `published` (an idle service only) - the wrap-around of the 32-bit
// counters is ten days of full-rate compression away otherwise.
extern "C" int tsx_debug_service_seed(int device_index, uint32_t published) {
    tsx_device* const dev = tsx_device_at(device_index);
    if (!dev) return TSX_E_INVAL;
    tsx_service& s = *dev->svc;
    tsx_device_scope keep;
    if (hipSetDevice(dev->hip_id) != hipSuccess) return TSX_E_DEVICE;
    std::lock_guard<std::mutex> lk(s.mu);
    if (svc_harvest_locked(s).any() || !s.out.empty()) return TSX_E_INVAL;
    const uint32_t w[2] = {published, published};
    if (hipMemcpy(&s.d->next, w, 8, hipMemcpyHostToDevice) != hipSuccess) return TSX_E_DEVICE;      // next, pub
    const uint32_t fa[2] = {published, 0};
    if (hipMemcpy(&s.d->fin, fa, 8, hipMemcpyHostToDevice) != hipSuccess) return TSX_E_DEVICE;      // fin, avail (nothing outstanding: no right to a ticket)
    s.published = published;
    __atomic_store_n(&s.h->published, published, __ATOMIC_RELEASE);
    return TSX_OK;
}
