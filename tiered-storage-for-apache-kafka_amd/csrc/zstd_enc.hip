// Zstandard frame compressor (levels 1 - 3) — gfx950, one 64-lane wavefront per chunk, up to 24 chunks resident per CU.
// Levels 1 and 2 take the fast parse (fast_block) - but level 2 for sources in (128 KiB, 256 KiB], which libzstd makes dfast; the rest
// of this header describes level 3's double-fast parse.
//
// Replaces zstd-jni's  new ZstdCompressCtx(); setPledgedSrcSize(n); setContentSize(true); compress(chunk)
//   core/src/main/java/io/aiven/kafka/tieredstorage/transform/CompressionChunkEnumeration.java:50-63
// and must emit, byte for byte, the frame libzstd emits for the same chunk (one-shot compression call, level 3:
// strategy dfast, windowLog <= 21, 128 KiB blocks, Huffman literals + FSE sequences; profile 1.5.7 adds that
// release's pre-block splitter).  The serial statement of the algorithm, pinned against the real library, is
// oracle/zstd_l3.c; this file is its wave-parallel form (DESIGN.md §5 has the measurements behind each choice):
//
//  * Match finding is an inherently serial greedy parse (every decision updates two hash tables and the repcode
//    history), so parallelism inside a chunk is SPECULATION: the wave evaluates K consecutive search positions at once
//    (K = 4 after a match, then 32, then 59 while nothing matches) - each lane hashes its position and probes both tables
//    (global memory: 512 KiB + 256 KiB per chunk cannot shrink into LDS without changing the output); a step whose lanes
//    share a bucket is cut in front of the second one (LDS scoreboard), a ballot picks the first lane with a match -
//    everything before it is exactly what the serial loop would have done - its table inserts are committed and the match
//    is verified and extended with one wave-wide 64-byte compare.
//  * A dependent global round trip costs a wave 1300-2000 cycles here, so the parser never reads global memory for bytes
//    near ip (LDS ring of the chunk around ip), never reads a candidate that cannot match (tags in the table entries),
//    verifies a far candidate and runs both extensions in one round trip, and keeps its state in SGPRs.
//  * Chunks are independent (fresh context per chunk in the reference); the kernel is latency bound per chunk and
//    HBM-random-access bound in aggregate, so it is shaped for residency: 80 VGPRs, 6.5 KiB LDS (parse-stage and
//    entropy-stage LDS alias), and callers keep several batches in flight.
//  * The entropy stage of each block: histograms, Huffman bit packing, literal gathering and the FSE sequence bit stream
//    run on all lanes (the three FSE state machines on three lanes, then prefix-summed bit packing); only the table
//    constructions (Huffman tree, FSE normalisation: a few thousand dependent steps per block) stay on lane 0.
//  * The wave also runs the stages either side of the compression when the batch asks for them (tsx_chain_fuse): CRC32C of
//    the source chunk before parsing it (crc_dev.h), AES-256-GCM over the finished frame (gcm_dev.h) - one launch per
//    batch; separate CRC / GCM launches starve for LDS on a chip full of compressor waves.
// This is byte-stream work: no MFMA.  Algorithmic traffic per chunk: N bytes read + transformed bytes written.
//
// One translation unit, cut along its stages, each header included here once in dependency order: zstd_enc_dev.h (what every stage
// uses), zstd_enc_parse.h (source window, match_block, fast_block), zstd_enc_devparse.h (device_block: the lane-parallel parse of
// TSX_ZSTD_PROFILE_DEVICE), zstd_enc_huf.h (huf_buildCTable), zstd_enc_entropy.h (FSE coder, bit
// packer, literal and sequence stages).  This file keeps the pre-splitters, the frame loop, the GCM / CRC fusion, the kernels, the host side.
#include "zstd_common.h"
#include "gcm_dev.h"
#include "crc_dev.h"
#include "svc_dev.h"
#define XXH_WAVE_ATTR __attribute__((noinline))     /* out of line, like the other cold stages: the service kernel keeps its registers */
#include "xxh64_dev.h"
#include "zstd_enc_dev.h"
#include "zstd_enc_parse.h"
#include "zstd_enc_devparse.h"
#include "zstd_enc_huf.h"
#include "zstd_enc_entropy.h"

// ---------------------------------------------------------------------------------------------------
// libzstd 1.5.7 pre-block splitter (ZSTD_splitBlock_byChunks level 0): byte histogram of every 43rd byte of
// each 8 KiB chunk, compared with the accumulated past.
// ---------------------------------------------------------------------------------------------------
__device__ ZS_NOINLINE static uint32_t split_block_1_5_7(const uint8_t* __restrict__ p, EncLds& L, uint32_t lane) {
    uint32_t* past = L.hist; uint32_t* cur = L.hist2;
    uint32_t pastN = 0; int penalty = 3;
    for (uint32_t i = lane; i < 256; i += LANES) past[i] = 0;
    __syncthreads();
    for (uint32_t n = lane * 43; n < 8191; n += LANES * 43) atomicAdd(&past[p[n]], 1u);
    pastN = 8191 / 43;
    __syncthreads();
    for (uint32_t pos = 8192; pos <= ZS_BLOCK_MAX - 8192; pos += 8192) {
        for (uint32_t i = lane; i < 256; i += LANES) cur[i] = 0;
        __syncthreads();
        for (uint32_t n = lane * 43; n < 8191; n += LANES * 43) atomicAdd(&cur[p[pos + n]], 1u);
        const uint32_t curN = 8191 / 43;
        __syncthreads();
        uint64_t dev = 0;
        for (uint32_t i = lane; i < 256; i += LANES) {
            const int64_t d = (int64_t)past[i] * (int64_t)curN - (int64_t)cur[i] * (int64_t)pastN;
            dev += (uint64_t)(d < 0 ? -d : d);
        }
        for (int o = 32; o; o >>= 1) dev += __shfl_xor(dev, o);
        const uint64_t p50 = (uint64_t)pastN * (uint64_t)curN;
        const uint64_t threshold = p50 * (uint64_t)(14 + penalty) / 16;
        if (dev >= threshold) return pos;
        for (uint32_t i = lane; i < 256; i += LANES) past[i] += cur[i];
        pastN += curN;
        if (penalty > 0) penalty--;
        __syncthreads();
    }
    return ZS_BLOCK_MAX;
}

// libzstd 1.5.7 pre-block splitter of strategy fast (ZSTD_splitBlock_fromBorders): byte histograms of the first and the last 512 bytes
// of the 128 KiB block; when they differ, the histogram of the middle 512 bytes decides between 32, 64 and 96 KiB.
__device__ ZS_NOINLINE static uint32_t split_block_fast_1_5_7(const uint8_t* __restrict__ p, EncLds& L, uint32_t lane) {
    uint32_t* h0 = L.hist; uint32_t* h1 = L.hist2;
    for (uint32_t i = lane; i < 256; i += LANES) { h0[i] = 0; h1[i] = 0; }
    __syncthreads();
    for (uint32_t n = lane; n < 512; n += LANES) { atomicAdd(&h0[p[n]], 1u); atomicAdd(&h1[p[ZS_BLOCK_MAX - 512 + n]], 1u); }
    __syncthreads();
    uint32_t past[4], fresh[4];
    uint64_t dev = 0;
    for (uint32_t k = 0; k < 4; k++) {
        past[k] = h0[lane + k * LANES]; fresh[k] = h1[lane + k * LANES];
        const int64_t d = (int64_t)past[k] * 512 - (int64_t)fresh[k] * 512;
        dev += (uint64_t)(d < 0 ? -d : d);
    }
    for (int o = 32; o; o >>= 1) dev += __shfl_xor(dev, o);
    if (dev < (uint64_t)512 * 512 * 14 / 16) return ZS_BLOCK_MAX;     // compareFingerprints(penalty 0): not "too different"
    __syncthreads();
    for (uint32_t i = lane; i < 256; i += LANES) h0[i] = 0;
    __syncthreads();
    for (uint32_t n = lane; n < 512; n += LANES) atomicAdd(&h0[p[ZS_BLOCK_MAX / 2 - 256 + n]], 1u);
    __syncthreads();
    uint64_t dB = 0, dE = 0;
    for (uint32_t k = 0; k < 4; k++) {
        const int64_t m = (int64_t)h0[lane + k * LANES] * 512;
        const int64_t x = (int64_t)past[k] * 512 - m, y = (int64_t)fresh[k] * 512 - m;
        dB += (uint64_t)(x < 0 ? -x : x); dE += (uint64_t)(y < 0 ? -y : y);
    }
    for (int o = 32; o; o >>= 1) { dB += __shfl_xor(dB, o); dE += __shfl_xor(dE, o); }
    __syncthreads();
    const int64_t diff = (int64_t)dB - (int64_t)dE;
    if ((diff < 0 ? -diff : diff) < 512 * 512 / 3) return 64u << 10;
    return dB > dE ? 32u << 10 : 96u << 10;
}

__device__ static bool wave_is_rle(const uint8_t* __restrict__ p, uint32_t n, uint32_t lane) {
    const uint8_t b0 = p[0];
    bool bad = false;
    for (uint32_t i = lane; i < n && !bad; i += LANES) bad = p[i] != b0;
    return !__any(bad);
}

// ---------------------------------------------------------------------------------------------------
// the kernel: one wave per chunk
// ---------------------------------------------------------------------------------------------------
// The frame is complete: publish its size and, when the batch is also encrypted, run GCM over it in this same wave.  A separate
// GCM launch would need 40 KiB of LDS per workgroup on CUs whose LDS and VGPRs are held by compressor waves of the batches in
// flight, and sat hundreds of ms in the queue for 20 ms of work; here it costs the wave a few ms of its second-long life.
__device__ static ZS_NOINLINE void finish_frame(tsx_chunk_desc* __restrict__ descs, uint32_t chunk, const uint8_t* frame, uint32_t flen,
                                    uint32_t* __restrict__ zlen, int32_t* __restrict__ status, const tsx_chain_fuse fuse, uint8_t* keyLocal, EncLds& L, uint32_t lane) {
    if (lane == 0) zlen[chunk] = flen;
    if (!fuse.key && !fuse.out) return;                                 // the frame stays in the staging buffer (stages as separate launches)
    stage_sync();
    const uint64_t dstOff = descs[chunk].dst_off;
    const uint64_t needed = (uint64_t)flen + (fuse.key ? 28 : 0);      // encrypted: 12 bytes of IV in front, 16 bytes of tag behind
    if (needed > descs[chunk].dst_cap) {
        if (lane == 0) { status[chunk] = TSX_E_DST_TOO_SMALL; descs[chunk].dst_len = 0; if (fuse.self_status) descs[chunk].status = TSX_E_DST_TOO_SMALL; }
        return;
    }
    if (!fuse.key) {
        // compression without encryption: the frame goes to the caller's slot as it is (16 bytes per lane: slots are 16-byte aligned)
        uint8_t* const o = fuse.out + dstOff;
        const uint32_t q = flen >> 4;
        for (uint32_t i = lane; i < q; i += LANES) reinterpret_cast<uint4*>(o)[i] = reinterpret_cast<const uint4*>(frame)[i];
        for (uint32_t i = (q << 4) + lane; i < flen; i += LANES) o[i] = frame[i];
    } else {
        const tsx_gcm_key* key = fuse.key;
        if (fuse.key_on_host) {
            // the key schedule waits in the caller's pinned memory: 21 KB over PCIe once per chunk, into this chunk's workspace
            static_assert(sizeof(tsx_gcm_key) <= ZS_WS_KEYCOPY_BYTES && sizeof(tsx_gcm_key) % 16 == 0, "key copy fits its workspace region");
            const uint4* s_ = reinterpret_cast<const uint4*>(fuse.key); uint4* d_ = reinterpret_cast<uint4*>(keyLocal);
            for (uint32_t i = lane; i < sizeof(tsx_gcm_key) / 16; i += LANES) d_[i] = s_[i];
            stage_sync();
            key = reinterpret_cast<const tsx_gcm_key*>(keyLocal);
        }
        uint8_t iv[12];
        { const uint8_t* p_ = descs[chunk].iv; for (int i = 0; i < 12; i++) iv[i] = p_[i]; }
        gcm_encrypt_wave(fuse.aes, key, iv, frame, flen, fuse.out + dstOff, L.g.t0, L.g.tab, lane);
        if (fuse.key_on_host) {
            stage_sync();
            uint4 z; z.x = z.y = z.z = z.w = 0;
            uint4* d_ = reinterpret_cast<uint4*>(keyLocal);
            for (uint32_t i = lane; i < sizeof(tsx_gcm_key) / 16; i += LANES) d_[i] = z;      // the copy does not outlive the chunk
        }
    }
    if (lane == 0) { descs[chunk].dst_len = (uint32_t)needed; if (fuse.self_status) descs[chunk].status = TSX_OK; }
}

// The content checksum behind the last block (ZSTD_c_checksumFlag): the low 32 bits of XXH64 of the chunk, little endian.  The hash
// is taken here, at the chunk's end and from its source bytes, by whichever wave finishes the chunk: one that starts a handed-back
// chunk again gets here on its own.  Returns the frame's new end.
__device__ static ZS_NOINLINE uint8_t* append_checksum(uint8_t* op, const uint8_t* __restrict__ src, uint32_t srcSize, uint32_t lane) {
    const uint32_t h = (uint32_t)xxh64_wave(src, srcSize, lane);
    if (lane == 0) put_le(op, h, 4);
    return op + 4;
}

// Block_Header: last-block bit, type, then the block's size (raw, RLE: regenerated; compressed: what follows) - 3 bytes, little endian
enum { ZS_BLOCK_RAW = 0, ZS_BLOCK_RLE = 1, ZS_BLOCK_COMPRESSED = 2 };
__device__ __forceinline__ static void put_block_header(uint8_t* op, uint32_t lastBlock, uint32_t type, uint32_t size) { put_le(op, lastBlock + (type << 1) + (size << 3), 3); }

// Between two blocks, and while the sequences of a block are coded, the two Huffman tables wait in the chunk's workspace (ZS_WS_HUFSAVE):
// the LL table has their bytes in LDS (EncLds).  Both directions end with the hand-off to the next stage.
__device__ __forceinline__ static void huf_to_workspace(uint32_t* __restrict__ hufSave, const EncLds& L, uint32_t lane) {
    for (uint32_t i = lane; i < sizeof(L.huf) / 4; i += LANES) hufSave[i] = reinterpret_cast<const uint32_t*>(&L.huf[0])[i];
    stage_sync();
}
__device__ __forceinline__ static void huf_from_workspace(EncLds& L, const uint32_t* __restrict__ hufSave, uint32_t lane) {
    for (uint32_t i = lane; i < sizeof(L.huf) / 4; i += LANES) reinterpret_cast<uint32_t*>(&L.huf[0])[i] = hufSave[i];
    stage_sync();
}

// One chunk, start to finish, in the calling wave: CRC32C head, frame, GCM tail (or the copy into the caller's slot), descriptor.
// Every argument is the same in all lanes (the service kernel hands them over in SGPRs).
// `hb` (svc_dev.h: what makes this wave give up its CU) is asked before every block; when it says so, true is returned with the chunk
// unfinished.  Nothing the caller can see has been written by then but the chunk's CRC32C and TSX_OK in status[] (both the same again
// next time); hash tables, frame and entropy state live in the chunk's own workspace and are set up afresh by whoever starts the chunk again.
__device__ __forceinline__ static bool zstd_compress_chunk(EncLds& L, const uint8_t* __restrict__ src_base, tsx_chunk_desc* __restrict__ descs,
                                                           uint8_t* __restrict__ mid, uint64_t mid_stride, uint32_t* __restrict__ zlen,
                                                           int32_t* __restrict__ status, uint8_t* __restrict__ work, uint32_t profile, uint32_t level_word, uint32_t sched,
                                                           const tsx_chain_fuse fuse, const uint32_t chunk, const svc_handback hb ZS_PROF_PARAM) {
    const uint32_t lane = threadIdx.x;
    const uint32_t level = level_word & ~TSX_ZSEG_CHECKSUM;
    const bool checksum = (level_word & TSX_ZSEG_CHECKSUM) != 0;
#ifdef TSX_PROF
    if (lane == 0) { for (int i = 0; i < 24; i++) g_prof[i] = 0; g_prof[22] = g_prof[23] = (unsigned long long)clock64(); g_prof[2] = wall_clock64(); }
    __syncthreads();
#endif
    const uint8_t* __restrict__ src = src_base + descs[chunk].src_off;
    const uint32_t srcSize = descs[chunk].src_len;
    uint8_t* const frame = mid + (uint64_t)chunk * mid_stride;
    uint8_t* const ws = work + (size_t)chunk * ZS_WS_BYTES;
    uint32_t* const hashLong = (uint32_t*)(ws + ZS_WS_HASHLONG);
    uint32_t* const hashSmall = (uint32_t*)(ws + ZS_WS_HASHSMALL);
    zs_seq* const seqs = (zs_seq*)(ws + ZS_WS_SEQS);
    uint8_t* const lit = ws + ZS_WS_LIT;
    uint8_t* const codes = ws + ZS_WS_CODES;
    uint8_t* const blockout = ws + ZS_WS_BLOCKOUT;
    uint32_t* const huftmp = (uint32_t*)(blockout + (256u << 10));                  // 4-byte aligned stream scratch
    if (fuse.crc) {
        const uint32_t crc = crc32c_wave(fuse.crc, src, srcSize, L.crcTab, lane);
        if (lane == 0) descs[chunk].crc32c = crc;
        PT(16);
    }
    if (fuse.self_status) { if (lane == 0) status[chunk] = TSX_OK; }    // (finish_frame publishes the chunk's final status in its descriptor)
    else if (status[chunk] != TSX_OK) { if (lane == 0) { zlen[chunk] = 0; if (fuse.key) descs[chunk].dst_len = 0; } return false; }

    // level 1 or 2 (tsx_zseg.level); anything else is level 3.  Level 1 and level 2 outside (128 KiB, 256 KiB] are strategy fast: one table
    // (hashLong's place), the fast parse and the fast pre-splitter; level 2 inside that band is dfast like level 3, with its own parameters.
    zs_cparams cp = zs_level3_cparams(srcSize);
    bool fast = false;
    if (level == 1 || level == 2) {
        const zs_level_params q = zs_level_cparams((int)level, srcSize ? srcSize : 1);
        cp.windowLog = q.windowLog; cp.chainLog = q.chainLog; cp.hashLog = q.hashLog; cp.minMatch = q.minMatch;
        fast = q.strategy == ZS_STRAT_FAST;
    }
    {   // fresh tables (ZSTD_reset_matchState): zero hashLong[1 << hashLog] and (dfast) hashSmall[1 << chainLog]
        uint4 z; z.x = z.y = z.z = z.w = 0;
        uint4* a = (uint4*)hashLong; uint4* b = (uint4*)hashSmall;
        for (uint32_t i = lane; i < (1u << cp.hashLog) / 4; i += LANES) a[i] = z;
        if (!fast) for (uint32_t i = lane; i < (1u << cp.chainLog) / 4; i += LANES) b[i] = z;
    }
    // ---- frame header (ZSTD_writeFrameHeader: content size known, the checksum bit on request, no dictID) ----
    uint32_t hdr = 0;
    {   const uint32_t windowSize = 1u << cp.windowLog;
        const uint32_t single = windowSize >= srcSize;
        const uint32_t fcs = (srcSize >= 256) + (srcSize >= 65536 + 256);
        uint8_t h[16]; uint32_t k = 0;
        h[k++] = 0x28; h[k++] = 0xB5; h[k++] = 0x2F; h[k++] = 0xFD;
        h[k++] = (uint8_t)((single << 5) + (fcs << 6) + (checksum ? 4u : 0u));
        if (!single) h[k++] = (uint8_t)((cp.windowLog - 10) << 3);
        if (fcs == 0) { if (single) h[k++] = (uint8_t)srcSize; }
        else if (fcs == 1) { h[k++] = (uint8_t)(srcSize - 256); h[k++] = (uint8_t)((srcSize - 256) >> 8); }
        else { h[k++] = (uint8_t)srcSize; h[k++] = (uint8_t)(srcSize >> 8); h[k++] = (uint8_t)(srcSize >> 16); h[k++] = (uint8_t)(srcSize >> 24); }
        hdr = k;
        if (lane == 0) for (uint32_t i = 0; i < k; i++) frame[i] = h[i];
    }
    uint8_t* op = frame + hdr;
    if (srcSize == 0) {
        if (lane == 0) put_block_header(op, 1, ZS_BLOCK_RAW, 0);
        op += 3;
        if (checksum) op = append_checksum(op, src, 0, lane);
        finish_frame(descs, chunk, frame, (uint32_t)(op - frame), zlen, status, fuse, ws + ZS_WS_KEYCOPY, L, lane);
        return false;
    }
    uint32_t* const hufSave = (uint32_t*)(ws + ZS_WS_HUFSAVE);
    if (lane == 0) L.scal[ZS_SCAL_MULT] = fast ? 10u - ZS_STRAT_FAST : 10u - ZS_STRAT_DFAST;
    static_assert(sizeof(L.huf) % 4 == 0 && sizeof(L.huf) <= 2048, "Huffman tables fit their place in the workspace");
    if (lane == 0) { L.hufRepeat[0] = 0; L.hufRepeat[1] = 0; L.huf[0].maxSym = 0; L.huf[1].maxSym = 0; }
    __syncthreads();
    huf_to_workspace(hufSave, L, lane);
    PT(0);
    uint32_t repc[3] = {1, 4, 8};                                       // confirmed repcode history
    const uint32_t blockSizeMax = (1u << cp.windowLog) < ZS_BLOCK_MAX ? (1u << cp.windowLog) : ZS_BLOCK_MAX;
    uint32_t ipos = 0, remaining = srcSize, dictLimit = 2;
    int64_t savings = 0;
    int cur = 0;                 // index of the confirmed Huffman table (L.huf[cur]); a candidate is built in L.huf[cur ^ 1]
    bool first = true;
    while (remaining) {
        if (hb.yield || hb.reserved) {                                  // a guest: is the CU wanted back?  anybody else: am I (still) off the reserved CUs -
            uint32_t y = 0;                                             // and if I am not (restored there by the hardware's scheduler): is the CU wanted?
            if (lane == 0) y = svc_must_yield(hb);
            if (UNI(y)) return true;
        }
        // ---- block size (ZSTD_optimalBlockSize) ----
        uint32_t blockSize = remaining < blockSizeMax ? remaining : blockSizeMax;
        if (profile == TSX_ZSTD_PROFILE_1_5_7 && remaining >= ZS_BLOCK_MAX && blockSizeMax >= ZS_BLOCK_MAX && savings >= 3)
            blockSize = fast ? UNI(split_block_fast_1_5_7(src + ipos, L, lane)) : UNI(split_block_1_5_7(src + ipos, L, lane));
        PT(1);
        const uint32_t lastBlock = blockSize == remaining;
        {   // ZSTD_window_enforceMaxDist(&ms->window, ip, maxDist, ...): libzstd >= 1.5.0 slides the window to the block's start
            const uint32_t blockEndIdx = ipos + 2, maxDist = 1u << cp.windowLog;
            if (blockEndIdx > maxDist && dictLimit < blockEndIdx - maxDist) dictLimit = blockEndIdx - maxDist;
        }
        uint32_t cSize = 0;                                             // 0 -> raw block
        if (blockSize >= 7) {
            uint32_t rep[3] = {repc[0], repc[1], repc[2]};
            MfState ms;
            // (the device profile has no levels, so `fast` is false with it: naming the profile in the first test as well is what keeps this
            // kernel's register allocation and spill counts the ones it had with two parsers - profiles/device_profile_resource_usage.txt)
            if (fast && profile != TSX_ZSTD_PROFILE_DEVICE) fast_block(src, ipos, blockSize, hashLong, cp, dictLimit, rep, seqs, ms, L.p.ring, lane);
            else if (profile == TSX_ZSTD_PROFILE_DEVICE) device_block(src, srcSize, ipos, blockSize, hashLong, hashSmall, cp, rep, seqs, ms, lane);
            else match_block(src, srcSize, ipos, blockSize, hashLong, hashSmall, cp, dictLimit, rep, seqs, ms, L.p.ring, L.p.scr, lane, sched);
            stage_sync();
            gather_literals(lit, src, seqs, ms.nbSeq, ms.anchor, ms.lastLL, lane);
            stage_sync();
            PT(18); PCNT(20, 1);
            // ---- ZSTD_entropyCompressSeqStore ----
            if (lane == 0) L.scal[ZS_SCAL_NEWHUF] = 0;
            __syncthreads();
            const bool suspect = ms.nbSeq == 0 || (ms.litSize / ms.nbSeq >= 20);
            huf_from_workspace(L, hufSave, lane);
            uint32_t litBytes = UNI(compress_literals(blockout, lit, ms.litSize, L, cur, suspect, huftmp, lane));
            stage_sync();
            huf_to_workspace(hufSave, L, lane);                         // the LL table takes their place
            uint32_t seqBytes = UNI(compress_sequences(blockout + litBytes, blockout + (255u << 10), seqs, ms.nbSeq, codes, L, huftmp, (ZS_BLOCKOUT_CAP - (256u << 10)) - 64, lane));
            const bool newHuf = UNI(L.scal[ZS_SCAL_NEWHUF]) != 0;
            if (seqBytes != 0xFFFFFFFFu) {
                cSize = litBytes + seqBytes;
                const uint32_t maxCSize = blockSize - ((blockSize >> 6) + 2);
                if (cSize >= maxCSize) cSize = 0;
            }
            if (!first && ms.nbSeq < 4 && ms.litSize < 10 && wave_is_rle(src + ipos, blockSize, lane)) cSize = 1;
            if (cSize > 1) {                                            // confirm repcodes + entropy tables
                repc[0] = rep[0]; repc[1] = rep[1]; repc[2] = rep[2];
                if (newHuf) { cur ^= 1; if (lane == 0) L.hufRepeat[cur] = 1; }      // HUF_repeat_check for the next block
                __syncthreads();
            }
        }
        // ---- emit the block ----
        if (cSize == 0) {
            if (lane == 0) put_block_header(op, lastBlock, ZS_BLOCK_RAW, blockSize);
            wave_copy(op + 3, src + ipos, blockSize, lane);
            cSize = 3 + blockSize;
        } else if (cSize == 1) {
            if (lane == 0) { put_block_header(op, lastBlock, ZS_BLOCK_RLE, blockSize); op[3] = src[ipos]; }
            cSize = 4;
        } else {
            if (lane == 0) put_block_header(op, lastBlock, ZS_BLOCK_COMPRESSED, cSize);
            wave_copy(op + 3, blockout, cSize, lane);
            cSize += 3;
        }
        PT(11);
        savings += (int64_t)blockSize - (int64_t)cSize;
        ipos += blockSize; remaining -= blockSize; op += cSize; first = false;
        __syncthreads();
    }
    if (checksum) {
        op = append_checksum(op, src, srcSize, lane);
        stage_sync();
    }
    finish_frame(descs, chunk, frame, (uint32_t)(op - frame), zlen, status, fuse, ws + ZS_WS_KEYCOPY, L, lane);
    PT(17);                                                             // (with a content checksum: its hash as well)
#ifdef TSX_PROF
    if (lane == 0 && prof_out) {
        g_prof[14] = (unsigned long long)clock64() - g_prof[22];
        g_prof[3] = wall_clock64();                                    // [2], [3]: the chunk's begin and end on the 100 MHz wall clock; [19]: where it ran (CU key | guest << 16)
        g_prof[19] = svc_cu_key() | (hb.yield ? 1u << 16 : 0u);
        for (int i = 0; i < 24; i++) prof_out[(size_t)chunk * 24 + i] = g_prof[i];
    }
#endif
    return false;
}

// ---------------------------------------------------------------------------------------------------
// the compressor service (tsx_internal.h: tsx_svc_host / tsx_svc_dev): persistent waves, one device-wide ticket queue.
// The protocol - who takes which ticket, who leaves when - is svc_dev.h; what follows fetches a member's entry and compresses.
// ---------------------------------------------------------------------------------------------------
static_assert(sizeof(tsx_zseg) == 128 && offsetof(tsx_zseg, src_base) == 16 && offsetof(tsx_zseg, fuse) == 72 && offsetof(tsx_zseg, done) == 112,
              "zstd_service_kernel reads a member entry as 16 eight-byte words, one per lane");
static_assert(sizeof(tsx_chain_fuse) == 40 && offsetof(tsx_chain_fuse, self_status) == 32, "layout of the fuse words");

__device__ static inline uint64_t svc_word(uint64_t w, int k) {            // word k of the member entry (lane k holds it), in every lane
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, k), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), k);
    return ((uint64_t)hi << 32) | lo;
}

static_assert(sizeof(EncLds) <= 5 * 1280, "five 1280-byte LDS granules per chunk: 25 chunks fit a CU's 160 KiB, the registers allow 24");
__global__ __launch_bounds__(LANES, ZS_WAVES_PER_SIMD) void zstd_service_kernel(tsx_svc_host* H, tsx_svc_dev* D, const tsx_svc_launch a ZS_PROF_PARAM) {
    __shared__ EncLds L;
    const uint32_t lane = threadIdx.x;
    const uint64_t t_start = svc_now();
    if (lane == 0) svc_wave_enter(H, D, a, t_start);
    if (a.calibrate_ticks) {                                              // how many of these workgroups does the chip hold at once?  (svc_create)
        if (lane == 0) svc_calibrate(H, D, a, t_start);
        return;
    }
    const uint32_t key = UNI(svc_cu_key());
    uint32_t role = 0;
    if (lane == 0) role = svc_admit(H, D, a, key);
    role = UNI(role);
    if (role == SVC_LEAVES) return;
    const svc_handback hb = svc_handback_of(H, D, role);
    uint32_t key_busy = 0;                                              // the CU this wave's chunk in progress is counted on (tsx_svc_dev.cu_busy)
    for (;;) {
        uint32_t got = 0, ticket = 0, chunk = 0;
        if (lane == 0) {
            got = svc_next(H, D, a, t_start, hb, &ticket, &chunk, &key_busy);
#ifdef TSX_PROF
            g_prof_take = wall_clock64();
#endif
        }
        key_busy = UNI(key_busy);
        got = UNI(got); ticket = UNI(ticket); chunk = UNI(chunk);
        if (got != 1 && got != 3) break;
        svc_acquire_chunk();
        // the ticket's record (a chunk that was handed back comes with its content) and its member's entry, straight from host memory
        uint32_t mg = ticket;
        if (got == 1) {
            if (lane == 0) { const tsx_svc_ticket* t = &H->ticket[ticket & (TSX_SVC_TICKETS - 1)]; mg = SVC_LD_SYS(&t->member_gen); chunk = SVC_LD_SYS(&t->chunk); }
            mg = UNI(mg); chunk = UNI(chunk);
        }
        const uint32_t slot = mg & 0xFFFFu;
        uint64_t w = 0;
        if (lane < 16 && slot < TSX_SVC_MEMBERS) w = SVC_LD_SYS(reinterpret_cast<const uint64_t*>(&H->member[slot]) + lane);
        const uint64_t w0 = svc_word(w, 0), w1 = svc_word(w, 1);
        const uint32_t n = (uint32_t)w0, profile = (uint32_t)(w0 >> 32), gen = (uint32_t)w1, level = (uint32_t)(w1 >> 32);
        if (slot >= TSX_SVC_MEMBERS || (gen & 0xFFFFu) != (mg >> 16) || chunk >= n) {          // an abandoned member's ticket
            if (lane == 0) svc_chunk_skipped(D, key_busy);
            continue;
        }
        tsx_chain_fuse fuse;
        fuse.crc = (const tsx_crc_tables*)svc_word(w, 9); fuse.aes = (const tsx_aes_tables*)svc_word(w, 10);
        fuse.key = (const tsx_gcm_key*)svc_word(w, 11); fuse.out = (uint8_t*)svc_word(w, 12);
        { const uint64_t f = svc_word(w, 13); fuse.self_status = (uint32_t)f; fuse.key_on_host = (uint32_t)(f >> 32); }
        uint32_t* const done = (uint32_t*)svc_word(w, 14); uint32_t* const flag = (uint32_t*)svc_word(w, 15);
        const bool handed_back = zstd_compress_chunk(L, (const uint8_t*)svc_word(w, 2), (tsx_chunk_desc*)svc_word(w, 3), (uint8_t*)svc_word(w, 4), svc_word(w, 5),
                            (uint32_t*)svc_word(w, 6), (int32_t*)svc_word(w, 7), (uint8_t*)svc_word(w, 8), profile, level, a.sched, fuse, chunk, hb ZS_PROF_ARG);
#ifdef TSX_PROF
        if (lane == 0 && prof_out && !handed_back) { prof_out[(size_t)chunk * 24 + 21] = t_start; prof_out[(size_t)chunk * 24 + 22] = g_prof_take; prof_out[(size_t)chunk * 24 + 19] |= (unsigned long long)key_busy << 20; }   // [21], [22]: when this wave began, when it had the ticket
#endif
        __syncthreads();                                                // (every lane's stores for the chunk are complete before lane 0 releases them)
        if (handed_back) {
            if (lane == 0) svc_chunk_handed_back(H, D, key_busy, mg, chunk, svc_is_guest(hb));
            break;
        }
        if (lane == 0) svc_chunk_finished(H, D, key_busy, n, done, flag);
        __syncthreads();
    }
    if (lane == 0) svc_wave_exit(H, D, a.launch_id, a.guest_launch);
}

// A launch that covers the chip (48 KiB of LDS per one-wave workgroup: three per CU) and notes every CU key it meets.
__global__ __launch_bounds__(LANES) void cu_probe_kernel(tsx_svc_dev* D) {
    __shared__ uint32_t big[12288];
    big[threadIdx.x] = threadIdx.x;
    __syncthreads();
    const uint32_t key = UNI(svc_cu_key());
    if (threadIdx.x == 0) svc_note_cu(D, key);
    const uint64_t t0 = svc_now();
    while (svc_now() - t0 < 3000u && big[(threadIdx.x * 7u) & 63u] != 0xFFFFFFFFu) svc_nap(1);   // ~30 us: later workgroups must go elsewhere
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
size_t tsx_zstd_consts_bytes(void) { return sizeof(tsx_zstd_consts); }
void tsx_zstd_build_consts(tsx_zstd_consts* h) { h->abi = 1; h->pad[0] = h->pad[1] = h->pad[2] = 0; }
size_t tsx_zstd_workspace_bytes(uint32_t n, uint32_t /*max_len*/) { return (size_t)n * ZS_WS_BYTES; }

void tsx_launch_zstd_service(hipStream_t st, tsx_svc_host* hd, tsx_svc_dev* d, uint32_t grid, tsx_svc_launch a) {
    if (!grid) return;
    hipLaunchKernelGGL(zstd_service_kernel, dim3(grid), dim3(LANES), 0, st, hd, d, a ZS_PROF_LAUNCH_ARG);
}
void tsx_launch_cu_probe(hipStream_t st, tsx_svc_dev* d, uint32_t grid) {
    if (grid) hipLaunchKernelGGL(cu_probe_kernel, dim3(grid), dim3(LANES), 0, st, d);
}
