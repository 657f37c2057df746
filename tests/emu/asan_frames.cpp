// TEST HARNESS ONLY: the bounds of both Zstandard decoder forms (csrc/zstd_dec.hip, csrc/zstd_dec_blocks.hip) under AddressSanitizer.  ONE
// executable: the emulated sources compiled with -fsanitize=address + this driver (csrc/Makefile, emu-asan-frames).  The corpus comes from
// tests/test_emu_frames_asan.py as a file: libzstd's frames with every feature the library emits and several hundred damaged ones
// (tests/frame_vocab_cases.py).  Every frame lies in a heap block of its own that ends with the frame's last byte, every output slot has
// exactly the declared size and the gaps between the slots are poisoned: a kernel that reads one byte past a frame, or writes one byte
// outside a slot, ends the program with a report.  Output: one line per frame and form - status and CRC32C of the restored bytes - which
// the Python side compares with the plain emulator's and with libzstd's verdicts.
//
// File format (little endian): u32 frames, then per frame u32 declared size, u32 frame length, the frame.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsxform.h"

extern "C" long long tsx_debug_config(const char* key, long long value);

struct Frame { uint8_t* bytes; uint32_t len, size; };

static uint32_t crc32c(const uint8_t* p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u))); tab[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

static int g_runs = 0;

// frames [lo, hi) as one batch through the form in force
static bool runBatch(tsx_ctx* ctx, const std::vector<Frame>& F, size_t lo, size_t hi, const char* form) {
    const uint32_t n = (uint32_t)(hi - lo);
    std::vector<tsx_chunk_desc> d(n);
    uintptr_t base = UINTPTR_MAX, end = 0;
    for (size_t i = lo; i < hi; i++) { base = std::min(base, (uintptr_t)F[i].bytes); end = std::max(end, (uintptr_t)F[i].bytes + F[i].len); }
    size_t dof = 0;
    for (uint32_t i = 0; i < n; i++) {
        memset(&d[i], 0, sizeof d[i]);
        d[i].src_off = (uintptr_t)F[lo + i].bytes - base; d[i].src_len = F[lo + i].len;
        d[i].dst_off = dof; d[i].dst_cap = F[lo + i].size;
        dof += ((F[lo + i].size + 15) & ~(size_t)15) + 16;
    }
    uint8_t* dst = (uint8_t*)aligned_alloc(16, dof);
    memset(dst, 0xEE, dof);
    for (uint32_t i = 0; i < n; i++) {                                  // everything between two slots, and behind the last one, is out of bounds
        const size_t a = d[i].dst_off + d[i].dst_cap, b = i + 1 < n ? d[i + 1].dst_off : dof;
        ASAN_POISON_MEMORY_REGION(dst + a, b - a);
    }
    tsx_batch_params p; memset(&p, 0, sizeof p);
    p.flags = TSX_COMPRESS; p.zstd_profile = TSX_ZSTD_PROFILE_1_5_7;
    const int rc = tsx_detransform_batch(ctx, &p, d.data(), n, (const void*)base, end - base, dst, dof, TSX_MEM_DEVICE);
    if (rc == TSX_OK)
        for (uint32_t i = 0; i < n; i++) {
            const bool sane = d[i].dst_len <= d[i].dst_cap && (d[i].status == TSX_OK || d[i].dst_len == 0);
            printf("frame %zu %s %d %08x%s\n", lo + i, form, d[i].status, sane ? crc32c(dst + d[i].dst_off, d[i].dst_len) : 0u, sane ? "" : " BAD-LENGTH");
            g_runs++;
        }
    else printf("batch %zu..%zu %s: tsx_detransform_batch returned %d\n", lo, hi, form, rc);
    ASAN_UNPOISON_MEMORY_REGION(dst, dof);
    free(dst);
    return rc == TSX_OK;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: asan_frames CORPUS [BATCH]\n"); return 2; }
    const size_t batch = argc > 2 ? (size_t)atoi(argv[2]) : 128;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    std::vector<Frame> F(count);
    for (uint32_t i = 0; i < count; i++) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) { printf("short corpus\n"); return 2; }
        F[i].size = hdr[0]; F[i].len = hdr[1];
        F[i].bytes = (uint8_t*)malloc(hdr[1] ? hdr[1] : 1);             // the block ends where the frame ends: the redzone starts at its last byte + 1
        if (hdr[1] && fread(F[i].bytes, 1, hdr[1], f) != hdr[1]) { printf("short corpus\n"); return 2; }
    }
    fclose(f);
    setenv("TSX_ALLOW_ANY_ARCH", "1", 1);                               // the emulator reports arch "emu"
    if (tsx_init(1, nullptr) < 1) { printf("tsx_init failed\n"); return 2; }
    tsx_ctx* ctx = nullptr;
    if (tsx_ctx_create(0, 0, 0, &ctx) != TSX_OK) { printf("tsx_ctx_create failed\n"); return 2; }
    bool ok = true;
    for (size_t lo = 0; lo < F.size(); lo += batch) {
        const size_t hi = std::min(F.size(), lo + batch);
        ok = runBatch(ctx, F, lo, hi, "block") && ok;
        const long long old = tsx_debug_config("dec_block_chunks", 0);
        ok = runBatch(ctx, F, lo, hi, "chunk") && ok;
        tsx_debug_config("dec_block_chunks", old);
    }
    tsx_ctx_destroy(ctx);
    tsx_shutdown();
    for (Frame& x : F) free(x.bytes);
    printf("asan frames: %d runs, %s\n", g_runs, ok ? "complete" : "INCOMPLETE");
    return ok ? 0 : 1;
}
