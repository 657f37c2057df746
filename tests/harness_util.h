/* TEST HARNESS ONLY: what the JNI harnesses (tests/jni/, C) and the host programs (tests/host/, C++17) share that is not a check: the
 * oracle's zstd prototypes, the input text, the slot layout of a batch, a v2 record batch, and libzstd's checksummed frame.  Every helper
 * is static inline, so a program that leaves one unused neither warns nor links what the helper calls. */
#ifndef TSX_HARNESS_UTIL_H
#define TSX_HARNESS_UTIL_H
#include <dlfcn.h>
#include <stdint.h>
#include <string.h>

#include "tsxform.h"

#ifdef __cplusplus
extern "C" {
#endif
size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   /* oracle/zstd_ref.c */
long long orc_zstd_decompress_chunk(const uint8_t* frame, size_t len, uint8_t* dst, size_t cap);
const char* orc_zstd_path(void);
const char* orc_zstd_version(void);
long long tsx_debug_config(const char* key, long long value);          /* test hook of the library, not in the header */
#ifdef __cplusplus
}
#endif

/* log-like text: words of a small vocabulary picked by an LCG */
static inline void harness_log_text(uint8_t* p, size_t n, uint32_t seed) {
    static const char* const words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
    uint32_t x = seed; size_t i = 0;
    while (i < n) {
        x = x * 1103515245u + 12345u;
        const char* w = words[(x >> 16) % 12];
        for (size_t k = 0; w[k] && i < n; k++) p[i++] = (uint8_t)w[k];
        if (((x >> 8) & 7) == 0 && i < n) p[i++] = (uint8_t)('0' + ((x >> 20) % 10));
    }
}

/* n zeroed descriptors, chunk i of sizes[i] bytes: slots 16-aligned with a 16-byte gap in both buffers, dst_cap the library's bound for
 * bound_flags; *src_bytes and *dst_bytes are the buffer sizes the layout needs */
static inline void harness_slots(tsx_chunk_desc* d, const uint32_t* sizes, int n, uint32_t bound_flags, size_t* src_bytes, size_t* dst_bytes) {
    size_t so = 0, dof = 0;
    memset(d, 0, (size_t)n * sizeof *d);
    for (int i = 0; i < n; i++) {
        d[i].src_off = so; d[i].dst_off = dof; d[i].src_len = sizes[i]; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], bound_flags);
        so += ((sizes[i] + 15) & ~15u) + 16; dof += ((d[i].dst_cap + 15) & ~15u) + 16;
    }
    *src_bytes = so; *dst_bytes = dof;
}

/* the fetch of what an upload laid out in d and wrote (done[i].dst_len bytes each): every chunk back to where its source was */
static inline void harness_fetch_slots(tsx_chunk_desc* b, const tsx_chunk_desc* d, const tsx_chunk_desc* done, int n) {
    memset(b, 0, (size_t)n * sizeof *b);
    for (int i = 0; i < n; i++) { b[i].src_off = d[i].dst_off; b[i].src_len = done[i].dst_len; b[i].dst_off = d[i].src_off; b[i].dst_cap = d[i].src_len; }
}

static inline uint32_t harness_crc32c(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u))); }
    return ~c;
}
static inline void harness_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
/* one v2 record batch of `total` bytes at p: header, then payload byte i = text[(i * stride + base_offset) % strlen(text)] */
static inline void harness_record_batch(uint8_t* p, uint32_t total, uint32_t base_offset, const char* text, uint32_t stride) {
    const uint32_t m = (uint32_t)strlen(text);
    memset(p, 0, 61);
    harness_be32(p + 4, base_offset); harness_be32(p + 8, total - 12); p[16] = 2; harness_be32(p + 57, 1);
    for (uint32_t i = 61; i < total; i++) p[i] = (uint8_t)text[(i * stride + base_offset) % m];
    harness_be32(p + 17, harness_crc32c(p + 21, total - 21));
}

/* libzstd's frame with ZSTD_c_checksumFlag, from the real libzstd the oracle has loaded and by the call sequence of oracle/zstd_ref.c;
 * (size_t)-1 when there is no library or it reports an error */
static inline size_t harness_libzstd_checksummed(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level) {
    static void* h;
    if (!h) h = dlopen(orc_zstd_path(), RTLD_NOW);
    if (!h) return (size_t)-1;
    void* (*create)(void) = (void* (*)(void))dlsym(h, "ZSTD_createCCtx");
    size_t (*destroy)(void*) = (size_t (*)(void*))dlsym(h, "ZSTD_freeCCtx");
    size_t (*set)(void*, int, int) = (size_t (*)(void*, int, int))dlsym(h, "ZSTD_CCtx_setParameter");
    size_t (*pledge)(void*, unsigned long long) = (size_t (*)(void*, unsigned long long))dlsym(h, "ZSTD_CCtx_setPledgedSrcSize");
    size_t (*compress2)(void*, void*, size_t, const void*, size_t) = (size_t (*)(void*, void*, size_t, const void*, size_t))dlsym(h, "ZSTD_compress2");
    unsigned (*isError)(size_t) = (unsigned (*)(size_t))dlsym(h, "ZSTD_isError");
    void* c = create();
    pledge(c, n);
    set(c, 200 /* ZSTD_c_contentSizeFlag */, 1); set(c, 100 /* ZSTD_c_compressionLevel */, level); set(c, 201 /* ZSTD_c_checksumFlag */, 1);
    const size_t r = compress2(c, dst, cap, src, n);
    destroy(c);
    return isError(r) ? (size_t)-1 : r;
}
#endif
