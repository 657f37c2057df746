// Shared definitions of the Zstandard stages (encoder + decoder): format constants and the per-chunk
// device workspace layout.
#pragma once
#include "tsx_internal.h"
#include "zstd_gpu.h"

#define ZS_BLOCK_MAX (128u << 10)
#define ZS_MAX_SEQ 32768u            /* 128 KiB / minMatch 4 */
#define ZS_MaxLL 35
#define ZS_MaxML 52
#define ZS_MaxOff 31
#define ZS_DefaultMaxOff 28
#define ZS_LLFSELog 9
#define ZS_MLFSELog 9
#define ZS_OffFSELog 8
#define ZS_LitHufLog 11
#define ZS_HUF_TABLELOG_MAX 12

struct tsx_zstd_consts { uint32_t abi; uint32_t pad[3]; };

struct zs_seq { uint32_t offBase, litLength, mlBase, litPos; };   /* litPos: chunk offset of the literal run (encoder) */

// ---- per-chunk workspace (global memory) --------------------------------------------------------------
#define ZS_WS_HASHLONG 0u                                             /* u32[1 << 17]                       */
#define ZS_WS_HASHSMALL (ZS_WS_HASHLONG + (4u << 17))                 /* u32[1 << 16]                       */
#define ZS_WS_SEQS (ZS_WS_HASHSMALL + (4u << 16))                     /* zs_seq[ZS_MAX_SEQ + 64]            */
#define ZS_WS_LIT (ZS_WS_SEQS + 16u * (ZS_MAX_SEQ + 64))              /* literals of the current block      */
#define ZS_WS_CODES (ZS_WS_LIT + ZS_BLOCK_MAX + 256)                  /* llCode | ofCode | mlCode           */
#define ZS_WS_CODE_STRIDE (ZS_MAX_SEQ + 64)
#define ZS_WS_STBITS (ZS_WS_CODES + 3u * ZS_WS_CODE_STRIDE)           /* u16[3][stride]: FSE state bits per sequence (LL|OF|ML) */
#define ZS_WS_BLOCKOUT (ZS_WS_STBITS + 6u * ZS_WS_CODE_STRIDE)        /* compressed block being built       */
#define ZS_BLOCKOUT_CAP (384u << 10)
#define ZS_WS_HUFSAVE (ZS_WS_BLOCKOUT + ZS_BLOCKOUT_CAP + 256)        /* the two Huffman tables of the literal stage, between blocks */
#define ZS_WS_KEYCOPY (ZS_WS_HUFSAVE + 2048)                           /* the wave's own copy of the batch key schedule (tsx_gcm_key), wiped by the wave */
#define ZS_WS_KEYCOPY_BYTES 21504u
#define ZS_WS_BYTES ((size_t)(ZS_WS_KEYCOPY + ZS_WS_KEYCOPY_BYTES))
#define ZS_WS_HASH_BYTES (ZS_WS_SEQS)                                 /* prefix that must be zero at start  */

struct zs_cparams { uint32_t windowLog, chainLog, hashLog, minMatch; };

// ZSTD_defaultCParameters[*][3] + ZSTD_adjustCParams_internal (libzstd 1.5.x), level 3 = dfast everywhere.
__host__ __device__ static inline zs_cparams zs_level3_cparams(uint32_t srcSize) {
    zs_cparams c;
    if (srcSize <= (16u << 10)) { c.windowLog = 14; c.chainLog = 14; c.hashLog = 15; c.minMatch = 4; }
    else if (srcSize <= (128u << 10)) { c.windowLog = 17; c.chainLog = 15; c.hashLog = 16; c.minMatch = 5; }
    else if (srcSize <= (256u << 10)) { c.windowLog = 18; c.chainLog = 16; c.hashLog = 16; c.minMatch = 4; }
    else { c.windowLog = 21; c.chainLog = 16; c.hashLog = 17; c.minMatch = 5; }
    uint32_t srcLog = 6;
    if (srcSize >= 64) { uint32_t v = srcSize - 1; srcLog = 0; while (v) { srcLog++; v >>= 1; } }
    if (c.windowLog > srcLog) c.windowLog = srcLog;
    if (c.hashLog > c.windowLog + 1) c.hashLog = c.windowLog + 1;
    if (c.chainLog > c.windowLog) c.chainLog = c.windowLog;
    if (c.windowLog < 10) c.windowLog = 10;
    return c;
}

// Levels 1 - 3 as ZSTD_getCParams(level, srcSize, 0) of libzstd 1.5.7 returns them: the row of ZSTD_defaultCParameters for the
// source size, then ZSTD_adjustCParams_internal.  srcSize 0 = unknown (no adjustment, the > 256 KiB row), as in the library.
// strategy: 1 = fast, 2 = dfast.  Level 2 is dfast for sources in (128 KiB, 256 KiB].  (zs_level3_cparams stays what the level-3
// compressor has always used; it agrees with this one for every known size.)
#define ZS_STRAT_FAST 1u
#define ZS_STRAT_DFAST 2u
struct zs_level_params { uint32_t windowLog, chainLog, hashLog, searchLog, minMatch, targetLength, strategy; };
__host__ __device__ static inline zs_level_params zs_level_cparams(int level, uint64_t srcSize) {
    //                                      wlog clog hlog slog mml tlen strategy           (levels 1, 2, 3)
    static const uint8_t kRows[4][3][7] = {{{19, 13, 14, 1, 7, 0, 1}, {20, 15, 16, 1, 6, 0, 1}, {21, 16, 17, 1, 5, 0, 2}},   // > 256 KiB
                                           {{18, 13, 14, 1, 6, 0, 1}, {18, 14, 14, 1, 5, 0, 2}, {18, 16, 16, 1, 4, 0, 2}},   // <= 256 KiB
                                           {{17, 12, 13, 1, 6, 0, 1}, {17, 13, 15, 1, 5, 0, 1}, {17, 15, 16, 2, 5, 0, 2}},   // <= 128 KiB
                                           {{14, 14, 15, 1, 5, 0, 1}, {14, 14, 15, 1, 4, 0, 1}, {14, 14, 15, 2, 4, 0, 2}}};  // <= 16 KiB
    const uint32_t li = level <= 1 ? 0u : level == 2 ? 1u : 2u;
    const uint32_t table = srcSize == 0 ? 0u : (srcSize <= (256u << 10)) + (srcSize <= (128u << 10)) + (srcSize <= (16u << 10));
    const uint8_t* r = kRows[table][li];
    zs_level_params c;
    c.windowLog = r[0]; c.chainLog = r[1]; c.hashLog = r[2]; c.searchLog = r[3]; c.minMatch = r[4]; c.targetLength = r[5]; c.strategy = r[6];
    if (srcSize != 0 && srcSize <= (1ull << 30)) {
        uint32_t srcLog = 6;
        if (srcSize >= 64) { uint64_t v = srcSize - 1; srcLog = 0; while (v) { srcLog++; v >>= 1; } }
        if (c.windowLog > srcLog) c.windowLog = srcLog;
    }
    if (srcSize != 0) {
        if (c.hashLog > c.windowLog + 1) c.hashLog = c.windowLog + 1;
        if (c.chainLog > c.windowLog) c.chainLog = c.windowLog;            // (cycleLog = chainLog below btlazy2)
    }
    if (c.windowLog < 10) c.windowLog = 10;
    return c;
}
