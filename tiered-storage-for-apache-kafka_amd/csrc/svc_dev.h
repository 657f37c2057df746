// The compressor service, device side: the protocol between the persistent waves of zstd_service_kernel, and between them and the
// host (layout and description: tsx_internal.h, tsx_svc_host / tsx_svc_dev / tsx_svc_launch; host side: tsx_service.hip).  Every access
// to a word of tsx_svc_dev, and to the protocol words of tsx_svc_host, is in this header; the kernel itself (zstd_enc.hip) reads the
// ticket records and member entries and compresses.  Nothing here knows the codec.
#pragma once
#include "tsx_internal.h"

#define SVC_NOINLINE __attribute__((noinline))      /* cold and register-hungry: kept out of the codec's loops */

// Words the host (or another wave) rewrites while this kernel lives are never read through a cache: member slots and ticket
// records are reused, and a persistent wave gets no kernel-boundary invalidate.
#ifdef HIPEMU
#define SVC_LD_SYS(p) __atomic_load_n((p), __ATOMIC_ACQUIRE)
#define SVC_LD_DEV(p) __atomic_load_n((p), __ATOMIC_ACQUIRE)
#define SVC_ST_DEV(p, v) __atomic_store_n((p), (v), __ATOMIC_RELEASE)
#define SVC_ST_SYS(p, v) __atomic_store_n((p), (v), __ATOMIC_RELEASE)
#define SVC_ST_MIRROR(p, v) __atomic_store_n((p), (v), __ATOMIC_RELAXED)
__device__ static inline uint64_t svc_now() { return hipemu_clock_100mhz(); }
__device__ static inline uint32_t svc_cu_key() { return hipemu_cu_key(); }
__device__ static inline void svc_nap(uint32_t) {}
__device__ static inline void svc_acquire_chunk() {}
__device__ static inline void svc_release_system() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }   // (the harness's __threadfence_system is a wave rendezvous: lane 0 is alone here)
__device__ static inline void svc_fence_device() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
__device__ static inline uint32_t zs_yield_asked(const uint32_t* p) { return hipemu_yield_probe(p); }
#else
#define SVC_LD_SYS(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
#define SVC_LD_DEV(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SVC_ST_DEV(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SVC_ST_SYS(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM)
#define SVC_ST_MIRROR(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)   /* statistics mirrors: no ordering wanted */
__device__ static inline uint64_t svc_now() { return wall_clock64(); }                       // 100 MHz, the same on every CU
// Which compute unit is this wave on?  HW_ID[15:8] = CU_ID | SH_ID | SE_ID, XCC_ID[3:0] = the XCD: a 12-bit key, unique per CU
// (tsx_launch_cu_probe counts the keys of a launch that covers the chip; the front end checks the count against the CU count).
__device__ static inline uint32_t svc_cu_key() {
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);              // hwreg(HW_REG_HW_ID, 0, 32)
    const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);             // hwreg(HW_REG_XCC_ID, 0, 4)
    return ((xcc & 15u) << 8) | ((hw >> 8) & 255u);
}
__device__ static inline void svc_nap(uint32_t n) { for (uint32_t i = 0; i < n; i++) __builtin_amdgcn_s_sleep(127); }     // ~3.5 us each
// What this wave reads next (a source chunk the copy engine has just written, descriptors the host has just rewritten) must not come
// from this CU's vector L1 or the scalar cache: both survive from the wave's previous chunk.
__device__ static inline void svc_acquire_chunk() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_dcache_inv\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
}
__device__ static inline void svc_release_system() { __threadfence_system(); }
__device__ static inline void svc_fence_device() { __threadfence(); }
// A look at the host's yield word (tsx_svc_host.yield, pinned memory: one PCIe read)
__device__ static inline uint32_t zs_yield_asked(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
#endif

// ---- whose compute unit is this? ----------------------------------------------------------------------------------------------------
__device__ static inline bool svc_cu_reserved(const uint32_t* reserved, uint32_t key) { return ((reserved[key >> 5] >> (key & 31)) & 1u) != 0; }

// What decides whether a wave must give up its CU.  Either part may be absent:
// `reserved` != nullptr (a wave of the launch itself on an ordinary CU): the bitmap of reserved compute units - the wave asks the hardware
// where it IS.  A wave does not move by itself, but the hardware's scheduler may save a queue's waves and restore them later, anywhere
// (compute wave save / restore, when another queue's dispatch has waited long enough): after that, compressor waves sat on the reserved
// CUs for the rest of their launch and a fetch found no room - the "kernel of a fetch that does not start, once in a few hundred fetches"
// of round 5 (profiles/r06_stuck_fetch_trace.txt).
// `yield` != nullptr: the host's yield word - a wave on a reserved CU (a guest, or one restored there) works on while it is down.
// Neither (a wave kept on a reserved CU, tsx_svc_launch.keep_waves): it stays whatever happens.
struct svc_handback { const uint32_t* reserved; const uint32_t* yield; };
__device__ static inline bool svc_is_guest(const svc_handback hb) { return !hb.reserved && hb.yield; }

// Lane 0: must this wave give up its CU now?  With a bitmap the hardware position first (*key, *moved: where the wave is, and whether that
// is a reserved CU), the yield word - over PCIe - only on a reserved CU; without a bitmap the word.
__device__ static inline bool svc_must_yield(const svc_handback hb, uint32_t* key = nullptr, bool* moved = nullptr) {
    if (!hb.reserved) return hb.yield && zs_yield_asked(hb.yield);
    const uint32_t k = svc_cu_key();
    const bool on = svc_cu_reserved(hb.reserved, k);
    if (key) *key = k;
    if (moved) *moved = on;
    return on && (!hb.yield || zs_yield_asked(hb.yield));
}

// ---- bookkeeping that several phases share (lane 0) ---------------------------------------------------------------------------------
// One more of a statistic, and its new value to the host's mirror (tsx_svc_host.m_*)
__device__ static inline void svc_count(uint32_t* stat, uint32_t* mirror) { SVC_ST_MIRROR(mirror, atomicAdd(stat, 1u) + 1u); }
// This wave no longer holds a chunk on CU key_busy
__device__ static inline void svc_drop_chunk(tsx_svc_dev* D, uint32_t key_busy) { atomicSub(&D->cu_busy[key_busy], 1u); atomicSub(&D->busy, 1u); }

// ---- the queue --------------------------------------------------------------------------------------------------------------------------
// The return list's lock
__device__ static inline void svc_ret_lock(tsx_svc_dev* D) { while (atomicCAS(&D->ret_lock, 0u, 1u) != 0u) svc_nap(1); svc_fence_device(); }
__device__ static inline void svc_ret_unlock(tsx_svc_dev* D) { svc_fence_device(); atomicExch(&D->ret_lock, 0u); }
// A guest hands its chunk back (lane 0, after the wave's last access to the chunk's workspace).
__device__ SVC_NOINLINE static void svc_return_chunk(tsx_svc_dev* D, uint32_t member_gen, uint32_t chunk) {
    svc_ret_lock(D);
    const uint32_t n = SVC_LD_DEV(&D->ret_n);
    if (n < TSX_SVC_RETURNED_MAX) { SVC_ST_DEV(&D->ret[n].member_gen, member_gen); SVC_ST_DEV(&D->ret[n].chunk, chunk); SVC_ST_DEV(&D->ret_n, n + 1u); }
    svc_ret_unlock(D);
    atomicAdd(&D->stat_returned, 1u);
}
// Lane 0 of an idle wave: the next ticket (1), or leave (2).  A wave leaves when the device is told to stop, when its launch has
// reached its age limit, or when the queue has been dry AND no wave has held a ticket for idle_exit_ticks - as long as anyone is
// still compressing, the idle waves stay (napping): the next member finds the whole supply of waves, not the stragglers' kernel.
// (3): a chunk that a guest handed back, in *ticket / *chunk_out (member slot | generation, chunk index) - taken before any fresh ticket.
// `yield` != nullptr: this wave is a guest and leaves (2) as soon as the word is raised.
// `moved`: a wave of the launch itself that sits on a reserved CU (restored there) - a guest for as long as nobody wants the CU.
__device__ SVC_NOINLINE static uint32_t svc_take(const tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a, const uint64_t t_start, const uint32_t* yield,
                                                const uint32_t key, uint32_t* ticket, uint32_t* chunk_out, const bool moved) {
    const uint64_t max_age = ((uint64_t)a.max_age_ticks_hi << 32) | a.max_age_ticks_lo;
    uint64_t quiet_since = 0, dry_since = 0;
    uint32_t nap = 1, looks = 0, turned_away = 1;
    for (;;) {
        const uint64_t now = svc_now();
        if (SVC_LD_DEV(&D->stop)) return 2;
        if (max_age && now - t_start > max_age) return 2;
        if (yield && (a.guests || moved) && (looks++ & 7u) == 0u && zs_yield_asked(yield)) return 2;     // (an idle guest: one PCIe read per eight looks, <= 2 ms apart)
        if (SVC_LD_DEV(&D->ret_n)) {
            atomicAdd(&D->busy, 1u);
            svc_ret_lock(D);
            const uint32_t n = SVC_LD_DEV(&D->ret_n);
            if (n) { *ticket = SVC_LD_DEV(&D->ret[n - 1u].member_gen); *chunk_out = SVC_LD_DEV(&D->ret[n - 1u].chunk); SVC_ST_DEV(&D->ret_n, n - 1u); }
            svc_ret_unlock(D);
            if (n) { atomicAdd(&D->cu_busy[key], 1u); return 3; }
            atomicSub(&D->busy, 1u);
        }
        if (SVC_LD_DEV(&D->draining)) return 2;                          // the launch is ending (below): no more tickets for it - the host starts the next one
        // one wave per poll_ticks asks the host - whether or not the mirror is dry: the host's stop word (pause, rotation, shutdown) must not wait
        // for a queue of thousands of tickets to be consumed first
        const uint32_t ps = SVC_LD_DEV(&D->poll_stamp);
        if ((uint32_t)now - ps >= a.poll_ticks && atomicCAS(&D->poll_stamp, ps, (uint32_t)now) == ps) {
            const uint32_t p = SVC_LD_SYS(&H->published);
            if (SVC_LD_SYS(&H->stop)) { SVC_ST_DEV(&D->stop, 1u); return 2; }
            uint32_t old = SVC_LD_DEV(&D->pub);
            while ((int32_t)(p - old) > 0) { const uint32_t prev = atomicCAS(&D->pub, old, p); if (prev == old) { atomicAdd(&D->avail, p - old); break; } old = prev; }   // (as many rights as tickets)
        }
        const uint32_t nx = SVC_LD_DEV(&D->next), pb = SVC_LD_DEV(&D->pub);
        if ((int32_t)(pb - nx) > 0) {
            // Tickets are waiting.  Two things decide whether this wave gets one:
            // - its CU's share (tsx_svc_dev.cu_busy): a partial load is spread evenly over the compressor's CUs - no CU runs more chunks than the
            //   outstanding ones (queued + in progress) divided by the CUs, rounded up, plus one.  The slot on the CU is reserved first (an atomic on
            //   the CU's own word), so that the waves of one CU cannot all pass the check at once;
            // - the semaphore tsx_svc_dev.avail: a right to one ticket is an atomic decrement that found it positive, and only then is `next`
            //   advanced - by a fetch-add that cannot fail.  (Until round 6 the ticket was a compare-and-swap on `next`: with 5000 idle waves going
            //   for a fresh batch's 2048 tickets almost every attempt lost - its value of `next` was stale by the time the atomic was served - and
            //   the tickets left at 20 per millisecond: the last chunk of a lone batch began 105 ms after the first, profiles/r06_ticket_storm.txt.)
            // A wave that is turned away looks again after a nap that doubles (3.5 - 56 us).
            const uint32_t limit = a.spread_cus ? ((pb - SVC_LD_DEV(&D->fin)) + a.spread_cus - 1u) / a.spread_cus + 1u : 0xFFFFFFFFu;     // (published - finished = outstanding)
            // Look before the read-modify-write, both times: a wave that decrements a spent semaphore holds it one lower until it has put the right
            // back, and with thousands of idle waves doing that around the clock a SMALL member's rights (7 tickets against ~170 waves inside that
            // window at any moment) never showed as positive to anybody - the host tests' 7-chunk batches stood still on the device (the CPU
            // harness runs one workgroup at a time and cannot see it; tests/test_zzzz_gpu_service.py::test_small_members_next_to_thousands_of_idle_waves).
            // Waves that only LOAD a spent semaphore leave it alone: it shows its true value as soon as the last loser has put its right back.
            if (SVC_LD_DEV(&D->cu_busy[key]) < limit && (int32_t)SVC_LD_DEV(&D->avail) > 0) {
                if (atomicAdd(&D->cu_busy[key], 1u) < limit) {
                    if ((int32_t)atomicSub(&D->avail, 1u) > 0) {
                        atomicAdd(&D->busy, 1u);                         // before `next` moves: whoever finds the queue dry finds busy != 0 (the idle exit looks at both)
                        svc_fence_device();
                        *ticket = atomicAdd(&D->next, 1u);
                        return 1;
                    }
                    atomicAdd(&D->avail, 1u);
                }
                atomicSub(&D->cu_busy[key], 1u);
            }
            svc_nap(turned_away); if (turned_away < 16u) turned_away *= 2u;
            continue;
        }
        // A guest does not wait for work.  With EVERY wave slot of the chip held and most of the waves idle, the busy ones crawl: a lone
        // 2048-chunk batch took 1.1 - 9.8 s instead of 1.1 s, whether the idle waves were guests, waves kept on the reserved CUs or ordinary
        // waves of a launch without any reservation; with as little as a third of one CU per shader engine free it is 1.1 s every time
        // (profiles/r06_full_chip_with_idle_waves.txt).  A chip that is full AND busy is fine (that is the saturated regime guests exist for).
        // So a guest that has found nothing to do for guest_idle_ticks (10 ms: the gap between two rounds of callers that resubmit at once is 2 - 3 ms)
        // leaves its slot; the next launch - which begins when work arrives after a dry spell - has guests again.
        // While more than half of the launch they help is busy the chip is not "mostly idle": the queue of callers that resubmit as their batches
        // complete runs dry for milliseconds at a time, a guest that leaves then is not replaced before all guests have left (one guest launch at a
        // time), and a saturated run went on with 291 of 768 guests (profiles/r06_ticket_storm.txt 6).  Then a guest waits 50 times as long.
        if (yield) {
            if (dry_since == 0) dry_since = now;
            else if (now - dry_since >= a.guest_idle_ticks && (SVC_LD_DEV(&D->busy) * 2u < a.main_waves || now - dry_since >= 50ull * a.guest_idle_ticks)) return 2;
        }
        if (a.guest_launch) { svc_nap(nap); if (nap < 64) nap *= 2; continue; }      // (when the launch they help ends is not for its guests to say)
        if (SVC_LD_DEV(&D->busy) != 0 || quiet_since == 0) quiet_since = now;
        if (now - quiet_since >= a.idle_exit_ticks && SVC_LD_DEV(&D->busy) == 0) { atomicExch(&D->draining, 1u); return 2; }
        svc_nap(nap);
        if (nap < 64) nap *= 2;
    }
}

// A wave leaves: the last one of the launch tells the host (pinned memory) that the launch is over, and when it began and ended.
__device__ SVC_NOINLINE static void svc_wave_exit(tsx_svc_host* H, tsx_svc_dev* D, uint32_t launch_id, uint32_t guest_launch) {
    SVC_ST_MIRROR(&H->m_live, atomicSub(&D->live, 1u) - 1u);
    if (guest_launch) {                                                  // a guest launch counts, and reports its end, apart
        if (atomicAdd(&D->g_exited, 1u) + 1u != gridDim.x) return;
        SVC_ST_DEV(&D->g_exited, 0u);
        svc_release_system();
        SVC_ST_SYS(&H->g_ended_launch, launch_id);
        return;
    }
    if (atomicAdd(&D->exited, 1u) + 1u != gridDim.x) return;
    // the last wave: the other statistics words as they stand (tsx_svc_host.m_*)
    SVC_ST_MIRROR(&H->m_live_max, SVC_LD_DEV(&D->live_max)); SVC_ST_MIRROR(&H->m_wave_starts, SVC_LD_DEV(&D->stat_wave_starts));
    SVC_ST_MIRROR(&H->m_reserved_exits, SVC_LD_DEV(&D->stat_reserved_exits)); SVC_ST_MIRROR(&H->m_skipped, SVC_LD_DEV(&D->stat_skipped));
    SVC_ST_MIRROR(&H->m_yields, SVC_LD_DEV(&D->stat_yields)); SVC_ST_MIRROR(&H->m_returned, SVC_LD_DEV(&D->stat_returned));
    SVC_ST_MIRROR(&H->m_chunks, SVC_LD_DEV(&D->stat_chunks));
    const uint64_t now = svc_now();
    const uint64_t first = ((uint64_t)SVC_LD_DEV(&D->t_first_hi) << 32) | SVC_LD_DEV(&D->t_first_lo);
    SVC_ST_DEV(&D->entered, 0u); SVC_ST_DEV(&D->exited, 0u);            // the next launch counts from zero (it is only started once this one is seen ended)
    SVC_ST_DEV(&D->draining, 0u);
    for (uint32_t g = 0; g < 256u; g++) if (SVC_LD_DEV(&D->kept[g])) SVC_ST_DEV(&D->kept[g], 0u);
    SVC_ST_MIRROR(&H->t_first, first); SVC_ST_MIRROR(&H->t_last, now);
    svc_release_system();
    SVC_ST_SYS(&H->ended_launch, launch_id);
}

// ---- the phases of a wave's life (zstd_service_kernel; lane 0 unless it says otherwise) ------------------------------------------------
// A wave has started: it counts itself (the first one of a launch stamps the launch's begin)
__device__ static inline void svc_wave_enter(tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a, const uint64_t t_start) {
    if (!a.guest_launch && atomicAdd(&D->entered, 1u) == 0u) { SVC_ST_DEV(&D->t_first_lo, (uint32_t)t_start); SVC_ST_DEV(&D->t_first_hi, (uint32_t)(t_start >> 32)); }
    const uint32_t lv = atomicAdd(&D->live, 1u) + 1u;
    atomicMax(&D->live_max, lv);
    SVC_ST_MIRROR(&H->m_live, lv);
}

// A calibration launch (tsx_svc_launch.calibrate_ticks: how many of these workgroups does the chip hold at once?)
// Every wave stays until no wave has ARRIVED for calibrate_ticks: live_max is then what fits at once, however slowly the dispatcher fills a
// cold chip.  (Until round 6 a wave stayed a fixed 300 us from its own start: on a box whose first launch placed one wave per ~20 us and CU
// the first waves had left before the sixteenth arrived - 15 per CU "measured", a grid of 3840 instead of 6144 for the life of the process.)
#define SVC_CALIBRATE_CAP_TICKS 5000000u              /* ... and never longer than 50 ms, whatever happens */
__device__ static inline void svc_calibrate(tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a, const uint64_t t_start) {
    SVC_ST_DEV(&D->poll_stamp, (uint32_t)t_start);
    while ((uint32_t)svc_now() - SVC_LD_DEV(&D->poll_stamp) < a.calibrate_ticks && svc_now() - t_start < SVC_CALIBRATE_CAP_TICKS) svc_nap(1);
    svc_wave_exit(H, D, a.launch_id, 0u);
}

// The probe launch (cu_probe_kernel): this compute unit exists
__device__ static inline void svc_note_cu(tsx_svc_dev* D, uint32_t key) { atomicOr(&D->seen[key >> 5], 1u << (key & 31)); }

// Admission: what is this wave, which has started on CU `key`, to its launch?
enum : uint32_t {
    SVC_LEAVES = 0,      // nothing: it has left (svc_wave_exit is done)
    SVC_ORDINARY = 1,    // a wave of the launch on an ordinary CU: it leaves when it finds itself on a reserved one that is wanted
    SVC_KEPT = 2,        // one of the first keep_waves on a reserved CU: it stays for good
    SVC_GUEST = 3,       // a guest on a reserved CU: it works while no fetch is about
};
__device__ static inline uint32_t svc_admit(tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a, const uint32_t key) {
    const bool on_reserved = svc_cu_reserved(D->reserved, key);
    uint32_t role = SVC_LEAVES;
    if (a.guest_launch) {                                                // a launch of guests only: the reserved CUs are where it is meant to land
        // (A guest that lands anywhere else leaves at once.  Slots that the launch itself had not filled swallow guest after guest that way - each is free
        //  again the moment its guest has left - and of 736 - 768 guests 288 - 767 stay, by run.  Letting them stay wherever they land was tried: every slot
        //  of the chip is held then, the hardware's scheduler saved and restored the waves in two runs of four, and those runs lost 10 % - for 224 waves
        //  more that the saturated regime, bound by its line requests, has no use for: profiles/r06_ticket_storm.txt 6.)
        if (on_reserved && !zs_yield_asked(&H->yield)) role = SVC_GUEST;
    } else if (!on_reserved) role = SVC_ORDINARY;
    // a reserved CU (see tsx_internal.h): the first keep_waves to arrive stay for good, the others work as guests while no fetch is about
    // (a.guests: the CPU harness; on the device guests come in launches of their own), or leave at once
    else if (a.keep_waves && atomicAdd(&D->kept[key >> 4], 1u) < a.keep_waves) role = SVC_KEPT;
    else if (a.guests && !zs_yield_asked(&H->yield)) role = SVC_GUEST;
    else atomicAdd(&D->stat_reserved_exits, 1u);
    if (role == SVC_LEAVES) svc_wave_exit(H, D, a.launch_id, a.guest_launch);
    else atomicAdd(&D->stat_wave_starts, 1u);
    return role;
}
// (any lane) ... and what makes a wave of that role give up its CU
__device__ static inline svc_handback svc_handback_of(const tsx_svc_host* H, const tsx_svc_dev* D, const uint32_t role) {
    svc_handback hb;
    hb.reserved = role == SVC_ORDINARY ? D->reserved : nullptr;
    hb.yield = role == SVC_KEPT ? nullptr : &H->yield;
    return hb;
}

// Between two chunks: where is this wave now?  Restored onto a reserved CU, it leaves before it takes another ticket - when the CU is
// wanted.  On a quiet device (yield word down) it works on like a guest: every restore used to cost the launch those waves for the rest of
// its life - a saturated run seen going from 6143 to 4153 live waves in 12 s, profiles/r06_ticket_storm.txt 6.  Then svc_take; *key_busy is
// the CU a chunk taken (1, 3) is counted on.
__device__ static inline uint32_t svc_next(tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a, const uint64_t t_start, const svc_handback hb,
                                           uint32_t* ticket, uint32_t* chunk, uint32_t* key_busy) {
    uint32_t k = 0, got = 2; bool moved = false;
    if (!hb.reserved) k = svc_cu_key();                                  // (nowhere it must keep off: a guest's looks at the yield word while idle are svc_take's)
    if (!hb.reserved || !svc_must_yield(hb, &k, &moved)) got = svc_take(H, D, a, t_start, moved || svc_is_guest(hb) ? hb.yield : nullptr, k, ticket, chunk, moved);
    if (moved && got == 2) svc_count(&D->stat_relocated, &H->m_relocated);
    if (got == 1 || got == 3) *key_busy = k;                             // (svc_take has counted the chunk on this CU)
    return got;
}

// The ticket named an abandoned member: nothing to do for it
__device__ static inline void svc_chunk_skipped(tsx_svc_dev* D, const uint32_t key_busy) {
    atomicAdd(&D->stat_skipped, 1u); atomicAdd(&D->fin, 1u);
    svc_drop_chunk(D, key_busy);
}

// A fetch has arrived (or the wave was moved onto a reserved CU): the chunk goes back to the queue - every lane's stores into its workspace
// are complete (the caller's barrier) and released here (as at the end of a finished chunk: the next wave may sit on another XCD, behind
// another L2) before another wave can start it again - and this wave leaves its CU to the fetch's kernels
__device__ static inline void svc_chunk_handed_back(tsx_svc_host* H, tsx_svc_dev* D, const uint32_t key_busy, const uint32_t member_gen, const uint32_t chunk, const bool guest) {
    svc_release_system(); svc_return_chunk(D, member_gen, chunk);
    if (guest) svc_count(&D->stat_yields, &H->m_yields);
    else svc_count(&D->stat_relocated, &H->m_relocated);                 // (not a guest: it was moved onto a reserved CU)
    svc_drop_chunk(D, key_busy);
}

// This chunk is done: tell its member's caller when it was the member's last one (of n; tsx_zseg.done / flag).
// The kernel goes on, so nothing here may rely on an end-of-kernel release: every lane's stores (ciphertext in device memory, which
// the caller's copy engine reads next, or in the caller's registered buffer; descriptor in pinned host memory) are complete at the
// caller's barrier, lane 0 releases them to system scope, and only then counts the chunk.
__device__ static inline void svc_chunk_finished(tsx_svc_host* H, tsx_svc_dev* D, const uint32_t key_busy, const uint32_t n, uint32_t* done, uint32_t* flag) {
    svc_release_system();
    svc_count(&D->stat_chunks, &H->m_chunks);
    atomicAdd(&D->fin, 1u);
    if (atomicAdd(done, 1u) + 1u == n) {
        atomicExch(done, 0u);                                            // ready for the context's next member (ordered before it by the flag)
        svc_release_system();
        // a plain system-scope store, not an atomic read-modify-write: the flag lives in HOST memory, and an atomic there would need
        // PCIe AtomicOps routed all the way to the root complex - not every server does that
        SVC_ST_SYS(flag, 1u);
    }
    svc_drop_chunk(D, key_busy);
}
