/* TEST HARNESS ONLY: TsxNative.ZSTD_CHECKSUM through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are) with a hand-made
 * JNIEnv (tests/jni/jni.h), as tests/jni/jni_levels_harness.c drives the level natives.  Checks: with the flag the frames carry bit 2 and
 * libzstd's checksum (the real libzstd the oracle has loaded, ZSTD_c_checksumFlag), slot and packed layouts alike, at the default level
 * and at level 1; without it today's bytes; the flag without TSX_COMPRESS is refused; detransform restores checksummed frames. */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jni.h"
#include "tsxform.h"

struct _jobject { void* addr; jlong cap; };
static jsize f_len(JNIEnv* e, jbyteArray a) { (void)e; return (jsize)a->cap; }
static void f_region(JNIEnv* e, jbyteArray a, jsize off, jsize n, jbyte* out) { (void)e; memcpy(out, (char*)a->addr + off, (size_t)n); }
static void* f_addr(JNIEnv* e, jobject b) { (void)e; return b ? b->addr : NULL; }
static jlong f_cap(JNIEnv* e, jobject b) { (void)e; return b ? b->cap : -1; }
static jstring f_str(JNIEnv* e, const char* s) { (void)e; jobject o = malloc(sizeof *o); o->addr = strdup(s); o->cap = (jlong)strlen(s); return o; }
static const struct JNINativeInterface_ kFns = {f_len, f_region, f_addr, f_cap, f_str};

jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_init(JNIEnv*, jclass);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_detransformBatch(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jobject, jint, jobject, jobject);
size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   /* oracle/zstd_ref.c */
const char* orc_zstd_path(void);

/* libzstd's frame with ZSTD_c_checksumFlag, by the call sequence of oracle/zstd_ref.c */
static size_t libzstd_checksummed(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level) {
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

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define N 3
int main(void) {
    JNIEnv envp = &kFns; JNIEnv* env = &envp;
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_init(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 30001, 60000};
    tsx_chunk_desc d[N]; memset(d, 0, sizeof d);
    size_t so = 0, dof = 0;
    for (int i = 0; i < N; i++) {
        d[i].src_off = so; d[i].dst_off = dof; d[i].src_len = sizes[i]; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], TSX_COMPRESS | TSX_ZSTD_CHECKSUM);
        CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], TSX_COMPRESS));        /* the bound covers the four bytes already */
        so += ((sizes[i] + 15) & ~15u) + 16; dof += ((d[i].dst_cap + 15) & ~15u) + 16;
    }
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    unsigned char* back = calloc(so, 1);
    {   /* log-like text: words of a small vocabulary picked by an LCG */
        static const char* words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
        uint32_t x = 99; size_t i = 0;
        while (i < so) {
            x = x * 1103515245u + 12345u;
            const char* w = words[(x >> 16) % 12];
            for (size_t k = 0; w[k] && i < so; k++) src[i++] = (unsigned char)w[k];
            if (((x >> 8) & 7) == 0 && i < so) src[i++] = (unsigned char)('0' + ((x >> 20) % 10));
        }
    }
    struct _jobject jsrc = {src, (jlong)so}, jdst = {dst, (jlong)dof}, jpk = {packed, (jlong)dof}, jback = {back, (jlong)so};
    for (int on = 0; on <= 1; on++) {
        const jint flags = (jint)(TSX_COMPRESS | (on ? TSX_ZSTD_CHECKSUM : 0u));
        for (int level = 0; level <= 1; level++) {
            tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
            struct _jobject js = {s, sizeof s};
            if (level == 0) CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &js, N, &jsrc, &jdst) == 0);
            else CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &js, N, &jsrc, &jdst) == 0);
            tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
            struct _jobject jp = {p, sizeof p};
            CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &jp, N, &jsrc, &jpk) == 0);
            size_t at = 0;
            for (int i = 0; i < N; i++) {
                const int lv = level ? level : 3;
                const size_t r = on ? libzstd_checksummed(src + d[i].src_off, sizes[i], ref, dof, lv) : orc_zstd_compress_chunk(src + d[i].src_off, sizes[i], ref, dof, lv);
                CHECK(r != (size_t)-1 && ((ref[4] >> 2) & 1) == on);
                CHECK(s[i].status == 0 && s[i].dst_len == r && memcmp(dst + d[i].dst_off, ref, r) == 0);
                CHECK(p[i].status == 0 && p[i].dst_off == at && p[i].dst_len == r && memcmp(packed + at, ref, r) == 0);
                at += r;
            }
            /* back through the fetch side's native: no flag needed, the frame decides */
            tsx_chunk_desc b[N]; memset(b, 0, sizeof b);
            for (int i = 0; i < N; i++) { b[i].src_off = d[i].dst_off; b[i].src_len = s[i].dst_len; b[i].dst_off = d[i].src_off; b[i].dst_cap = sizes[i]; }
            struct _jobject jb = {b, sizeof b};
            memset(back, 0, so);
            CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_detransformBatch(env, NULL, TSX_COMPRESS, NULL, NULL, &jb, N, &jdst, &jback) == 0);
            for (int i = 0; i < N; i++) CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, src + d[i].src_off, sizes[i]) == 0);
            printf("checksum %s, level %d: %u %u %u bytes\n", on ? "on" : "off", level, s[0].dst_len, s[1].dst_len, s[2].dst_len);
        }
    }
    /* a damaged checksummed frame comes back as a corrupt frame, where a ZstdException would surface */
    {
        tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
        struct _jobject js = {s, sizeof s};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, (jint)(TSX_COMPRESS | TSX_ZSTD_CHECKSUM), NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &js, N, &jsrc, &jdst) == 0);
        dst[d[1].dst_off + s[1].dst_len - 2] ^= 0x10;                     /* inside chunk 1's checksum */
        tsx_chunk_desc b[N]; memset(b, 0, sizeof b);
        for (int i = 0; i < N; i++) { b[i].src_off = d[i].dst_off; b[i].src_len = s[i].dst_len; b[i].dst_off = d[i].src_off; b[i].dst_cap = sizes[i]; }
        struct _jobject jb = {b, sizeof b};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_detransformBatch(env, NULL, TSX_COMPRESS, NULL, NULL, &jb, N, &jdst, &jback) == 0);
        CHECK(b[0].status == 0 && b[1].status == TSX_E_BAD_FRAME && b[1].dst_len == 0 && b[2].status == 0);
    }
    /* the flag without compression is refused */
    {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = {b, sizeof b};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, (jint)TSX_ZSTD_CHECKSUM, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jb, N, &jsrc, &jdst) == TSX_E_INVAL);
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, (jint)(TSX_ZSTD_CHECKSUM | TSX_CRC), NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 1, &jb, N, &jsrc, &jpk) == TSX_E_INVAL);
    }
    free(src); free(dst); free(packed); free(ref); free(back);
    printf("jni checksum ok\n");
    return 0;
}
