// Per-chunk bookkeeping of the block-parallel frame decoder (zstd_dec_blocks.hip): written by its index kernel, completed by its
// decode kernel, read by its execute kernel.  Lives in the context's block-mode workspace, one header per chunk, reset by the index kernel.
#pragma once
#include <stdint.h>

#define ZB_MAX_BLOCKS 264u                       /* blocks of one chunk this form takes: 2 x (16 MiB / 128 KiB) + slack; more -> fallback */
#define ZB_MAX_CHUNK (16u << 20)                 /* largest chunk (dst_cap) this form takes */

struct ZbBlock {
    uint32_t off, bsize;                         // block content in the frame: offset, Block_Size
    uint8_t btype, last, ltype, modes;           // block type, last-block bit, literals type, Symbol_Compression_Modes
    uint32_t litSize, q;                         // regenerated size of the literals, offset of the sequences section in the block
    uint32_t nbSeq;
    uint32_t litAt, seqAt;                       // this block's place in the literal arena (bytes) / the sequence arenas (entries)
    uint16_t hufSrc, tblSrc[3];                  // block whose bytes hold the Huffman tree / the LL, OF, ML table in force here
    uint32_t tOff[3], streamOff;                 // offsets in the block: description of each table defined here, start of the bit stream
    uint32_t regen;                              // bytes this block regenerates (raw / RLE: Block_Size; compressed: after decoding)
    uint32_t endHist[3];                         // repeat-offset history behind the block: offsets, or references into the incoming history
    uint32_t ok;                                 // decode kernel: sequences decoded and consistent
};
struct ZbChunk {
    uint32_t mode;                               // 1: the block form is decoding this chunk; 0: left to (or handed back to) zstd_decompress_kernel
    uint32_t nblocks, contentSize;
    uint32_t emitDone;                           // workgroups of zb_emit_kernel that have written their bytes (counted only when the frame has a checksum)
    uint32_t live[32];                           // jump round r left unresolved words in this chunk (round r + 1 returns at once when not)
    uint32_t hasCksum, cksum;                    // the frame declares a content checksum / its four bytes
    ZbBlock blk[ZB_MAX_BLOCKS];
};
#define ZB_CHUNK_HDR_BYTES ((sizeof(ZbChunk) + 255u) & ~(size_t)255u)

// zb_verify_kernel's words per chunk (zero before the launch): see the kernel
#define ZB_VERDICT_WORDS 4u
#define ZB_V_FAIL 0
#define ZB_V_NOT_TAKEN 1
#define ZB_V_SEEN 2
