/* TEST HARNESS ONLY: well-framed v2 record batches for the C and C++ harnesses of TSX_VALIDATE_FRAMES (tests/jni/jni_records_frames_harness.c,
 * tests/host/host_records_frames.cpp). */
#pragma once
#include <stdint.h>
#include <string.h>

#include "harness_util.h"

static inline uint32_t frames_varint(uint8_t* p, int32_t v) {          /* zigzag; returns the bytes written */
    uint32_t z = ((uint32_t)v << 1) ^ (uint32_t)(v >> 31), n = 0;
    while (z >= 0x80u) { p[n++] = (uint8_t)(z | 0x80u); z >>= 7; }
    p[n++] = (uint8_t)z;
    return n;
}
static inline void frames_seal(uint8_t* p, uint32_t total) { harness_be32(p + 17, harness_crc32c(p + 21, total - 21)); }
/* one batch at p: baseOffset `base`, nrec < 64 records (null key, a value of vlen bytes of `text`, no headers), offset deltas 0 .. nrec - 1.
 * Returns its size: 61 + nrec * (6 + the bytes of vlen's and the length's varints + vlen). */
static inline uint32_t frames_batch(uint8_t* p, uint32_t base, uint32_t nrec, uint32_t vlen, const char* text) {
    const uint32_t m = (uint32_t)strlen(text);
    uint8_t tmp[5];
    memset(p, 0, 61);
    harness_be32(p + 4, base); p[16] = 2; harness_be32(p + 23, nrec - 1); harness_be32(p + 57, nrec);
    uint32_t at = 61;
    for (uint32_t i = 0; i < nrec; i++) {
        const uint32_t body = 1 + 1 + 1 + 1 + frames_varint(tmp, (int32_t)vlen) + vlen + 1;
        at += frames_varint(p + at, (int32_t)body);
        p[at++] = 0;                                                    /* attributes */
        p[at++] = 0;                                                    /* timestampDelta */
        at += frames_varint(p + at, (int32_t)i);                        /* offsetDelta (one byte) */
        p[at++] = 1;                                                    /* keyLength -1 */
        at += frames_varint(p + at, (int32_t)vlen);
        for (uint32_t k = 0; k < vlen; k++) p[at++] = (uint8_t)text[(k * 7 + i + base) % m];
        p[at++] = 0;                                                    /* headersCount */
    }
    harness_be32(p + 8, at - 12);
    frames_seal(p, at);
    return at;
}
