// XXH64 (seed 0) of a byte range by ONE wave: the hash behind a Zstandard frame's content checksum (RFC 8878 3.1.1: the low four
// bytes of XXH64 of the original content).  Included by the compressor (zstd_enc.hip: the checksum it appends on request) and by
// both decoder forms (zstd_dec.hip, zstd_dec_blocks.hip: every checksummed frame is verified).
//
// The hash is four accumulators, each a serial chain over its own 8 bytes of every 32-byte stripe:
//     acc = rotl(acc + x * P2, 31) * P1
// so only lanes 0-3 carry state.  What does not depend on the chain is done by all 64 lanes ahead of it: one step loads 512 bytes
// (16 stripes, 8 bytes per lane; the next step's load is issued before this step's chain starts) and forms the 64 products
// x * P2 at once; the chain then takes 16 rounds, each fetching its product from lane 4 * stripe + accumulator.  Lanes 4-63 run
// the same rounds on values nobody reads.  The tail (fewer than 32 bytes) and the avalanche are the same in every lane.
// Every lane of the wave must call with the same arguments; ptr needs no alignment; no byte outside [ptr, ptr + len) is read.
#pragma once
#include <stdint.h>

#define XXH_P1 0x9E3779B185EBCA87ULL
#define XXH_P2 0xC2B2AE3D27D4EB4FULL
#define XXH_P3 0x165667B19E3779F9ULL
#define XXH_P4 0x85EBCA77C2B2AE63ULL
#define XXH_P5 0x27D4EB2F165667C5ULL

__device__ static inline uint64_t xxh_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64 - r)); }
__device__ static inline uint64_t xxh_ld64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ static inline uint32_t xxh_ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ static inline uint64_t xxh_round(uint64_t acc, uint64_t prod) { return xxh_rotl(acc + prod, 31) * XXH_P1; }      // prod = x * P2
__device__ static inline uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v * XXH_P2)) * XXH_P1 + XXH_P4; }
__device__ static inline uint64_t xxh_lane64(uint64_t v, int src) { return (uint64_t)__shfl((unsigned long long)v, src); }

// XXH_WAVE_ATTR: the decoders inline it (they end with it); the compressor keeps it out of line (its kernel is shaped for residency)
#ifndef XXH_WAVE_ATTR
#define XXH_WAVE_ATTR __forceinline__
#endif
__device__ static XXH_WAVE_ATTR uint64_t xxh64_wave(const uint8_t* ptr, uint32_t len, uint32_t lane) {
    uint64_t h = XXH_P5;                                                // (seed 0) the start of an input without a whole stripe
    const uint32_t stripeBytes = len & ~31u;
    if (stripeBytes) {
        const uint32_t a = lane & 3;
        uint64_t acc = a == 0 ? XXH_P1 + XXH_P2 : a == 1 ? XXH_P2 : a == 2 ? 0 : 0 - XXH_P1;
        const uint8_t* q = ptr + 8 * lane;                              // this lane's 8 bytes of the step at hand
        uint32_t rem = stripeBytes;                                     // stripe bytes from the step at hand on
        uint64_t nxt = 8 * lane + 8 <= rem ? xxh_ld64(q) : 0;
        while (rem) {
            const uint64_t prod = nxt * XXH_P2;
            const uint32_t ns = rem >= 512 ? 16 : rem >> 5;             // stripes of this step
            q += 512;
            nxt = rem > 512 && 8 * lane + 8 <= rem - 512 ? xxh_ld64(q) : 0;
            if (ns == 16) {
#pragma unroll
                for (int s = 0; s < 16; s++) acc = xxh_round(acc, xxh_lane64(prod, 4 * s + (int)a));
            } else {
                for (uint32_t s = 0; s < ns; s++) acc = xxh_round(acc, xxh_lane64(prod, (int)(4 * s + a)));
            }
            rem -= ns * 32;
        }
        const uint64_t v1 = xxh_lane64(acc, 0), v2 = xxh_lane64(acc, 1), v3 = xxh_lane64(acc, 2), v4 = xxh_lane64(acc, 3);
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        h = xxh_merge(h, v1); h = xxh_merge(h, v2); h = xxh_merge(h, v3); h = xxh_merge(h, v4);
    }
    h += len;
    const uint8_t* t = ptr + stripeBytes;
    uint32_t r = len & 31;
    for (; r >= 8; r -= 8, t += 8) h = xxh_rotl(h ^ xxh_round(0, xxh_ld64(t) * XXH_P2), 27) * XXH_P1 + XXH_P4;
    if (r >= 4) { h = xxh_rotl(h ^ ((uint64_t)xxh_ld32(t) * XXH_P1), 23) * XXH_P2 + XXH_P3; t += 4; r -= 4; }
    for (; r; r--, t++) h = xxh_rotl(h ^ ((uint64_t)*t * XXH_P5), 11) * XXH_P1;
    h ^= h >> 33; h *= XXH_P2;
    h ^= h >> 29; h *= XXH_P3;
    h ^= h >> 32;
    return h;
}
