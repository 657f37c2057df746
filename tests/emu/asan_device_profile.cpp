// TEST HARNESS ONLY: the bounds of the lane-parallel parse (csrc/zstd_enc_devparse.h, TSX_ZSTD_PROFILE_DEVICE) under AddressSanitizer.  ONE
// executable: the emulated sources compiled with -fsanitize=address + this driver (csrc/Makefile, emu-asan-device-profile).  The case list
// of tests/device_profile_cases.py arrives in a file that tests/test_emu_device_profile_asan.py writes (u32 count; per case u32 size and
// the bytes).  Every chunk is compressed on its own, as device memory: its source in a heap block that ends with the chunk's last byte,
// its output slot exactly tsx_transformed_bound large - so the 8-byte reads at a slice's end, the candidates' bytes, a lane's sequence
// slots and their compaction (the library's own workspace blocks) end the program with a report if they leave their blocks.  Chunks up
// to three blocks are then restored into a block of exactly their size and compared.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsxform.h"

struct Case { uint32_t size; uint8_t* bytes; };
static int g_runs = 0, g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d (case %u, %u bytes): %s\n", __LINE__, g_case, g_size, #c); g_failed++; } } while (0)
static uint32_t g_case = 0, g_size = 0;

static void runCase(tsx_ctx* ctx, const Case& c, uint32_t flags) {
    g_runs++; g_size = c.size;
    tsx_chunk_desc d; memset(&d, 0, sizeof d);
    d.src_len = c.size; d.dst_cap = (uint32_t)tsx_transformed_bound(c.size, flags);
    uint8_t* dst = (uint8_t*)malloc(d.dst_cap);
    tsx_batch_params p; memset(&p, 0, sizeof p);
    p.flags = flags; p.zstd_profile = TSX_ZSTD_PROFILE_DEVICE;
    CHECK(tsx_transform_batch(ctx, &p, &d, 1, c.bytes, c.size, dst, d.dst_cap, TSX_MEM_DEVICE) == TSX_OK);
    CHECK(d.status == TSX_OK && d.dst_len > 0 && d.dst_len <= d.dst_cap);
    if (d.status == TSX_OK && c.size <= 3u * (128u << 10)) {
        tsx_chunk_desc e; memset(&e, 0, sizeof e);
        e.src_len = d.dst_len; e.dst_cap = c.size;
        uint8_t* frame = (uint8_t*)malloc(d.dst_len);                   // ... and the frame in a block that ends with its last byte
        memcpy(frame, dst, d.dst_len);
        uint8_t* back = (uint8_t*)malloc(c.size ? c.size : 1);
        CHECK(tsx_detransform_batch(ctx, &p, &e, 1, frame, d.dst_len, back, c.size, TSX_MEM_DEVICE) == TSX_OK);
        CHECK(e.status == TSX_OK && e.dst_len == c.size && (!c.size || memcmp(back, c.bytes, c.size) == 0));
        free(back); free(frame);
    }
    free(dst);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: asan_device_profile CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    std::vector<Case> C(count);
    for (uint32_t i = 0; i < count; i++) {
        if (fread(&C[i].size, 4, 1, f) != 1) { printf("short case file\n"); return 2; }
        C[i].bytes = (uint8_t*)malloc(C[i].size ? C[i].size : 1);       // the block ends where the chunk ends: the redzone starts at its last byte + 1
        if (C[i].size && fread(C[i].bytes, 1, C[i].size, f) != C[i].size) { printf("short case file\n"); return 2; }
    }
    fclose(f);
    setenv("TSX_ALLOW_ANY_ARCH", "1", 1);                               // the emulator reports arch "emu"
    if (tsx_init(1, nullptr) < 1) { printf("tsx_init failed\n"); return 2; }
    tsx_ctx* ctx = nullptr;
    if (tsx_ctx_create(0, 0, 0, &ctx) != TSX_OK) { printf("tsx_ctx_create failed\n"); return 2; }
    for (g_case = 0; g_case < count; g_case++) {
        runCase(ctx, C[g_case], TSX_COMPRESS);
        if (g_case % 7 == 0) runCase(ctx, C[g_case], TSX_COMPRESS | TSX_ZSTD_CHECKSUM | TSX_VERIFY);
    }
    tsx_ctx_destroy(ctx);
    tsx_shutdown();
    for (Case& c : C) free(c.bytes);
    printf("asan device profile: %d runs, %d failed\n", g_runs, g_failed);
    return g_failed ? 1 : 0;
}
