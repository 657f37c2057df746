/* TEST HARNESS ONLY: TSX_ZSTD_PROFILE_DEVICE through the natives of the JNI shim (java/jni/tsx_jni.c) and a hand-made JNIEnv
 * (tests/jni/jni.h), as tests/jni/jni_levels_harness.c drives the levels.  Checks: the profile reaches the batch (the frames are not
 * libzstd's level-3 frames, and the oracle's libzstd restores every chunk from them), transformBatch, transformBatchLevel at level 0
 * and both packed natives write the same bytes, a level together with the profile comes back as TSX_E_UNSUPPORTED, and a fetch with the
 * profile in its parameter block restores the chunks. */
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
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPacked(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   /* oracle/zstd_ref.c */
long long orc_zstd_decompress_chunk(const uint8_t* frame, size_t len, uint8_t* dst, size_t cap);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define N 3
int main(void) {
    JNIEnv envp = &kFns; JNIEnv* env = &envp;
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_init(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 140001, 60000};
    tsx_chunk_desc d[N]; memset(d, 0, sizeof d);
    size_t so = 0, dof = 0;
    for (int i = 0; i < N; i++) {
        d[i].src_off = so; d[i].dst_off = dof; d[i].src_len = sizes[i]; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], TSX_COMPRESS);
        so += ((sizes[i] + 15) & ~15u) + 16; dof += ((d[i].dst_cap + 15) & ~15u) + 16;
    }
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* dst2 = calloc(dof, 1);
    unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    {   /* log-like text: words of a small vocabulary picked by an LCG */
        static const char* words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
        uint32_t x = 999; size_t i = 0;
        while (i < so) {
            x = x * 1103515245u + 12345u;
            const char* w = words[(x >> 16) % 12];
            for (size_t k = 0; w[k] && i < so; k++) src[i++] = (unsigned char)w[k];
            if (((x >> 8) & 7) == 0 && i < so) src[i++] = (unsigned char)('0' + ((x >> 20) % 10));
        }
    }
    struct _jobject jsrc = {src, (jlong)so}, jdst = {dst, (jlong)dof}, jdst2 = {dst2, (jlong)dof}, jpk = {packed, (jlong)dof};
    tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
    struct _jobject js = {s, sizeof s};
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, &js, N, &jsrc, &jdst) == 0);
    tsx_chunk_desc l[N]; memcpy(l, d, sizeof l);
    struct _jobject jl = {l, sizeof l};
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, 0, &jl, N, &jsrc, &jdst2) == 0);
    tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
    struct _jobject jp = {p, sizeof p};
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPacked(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, &jp, N, &jsrc, &jpk) == 0);
    size_t at = 0;
    for (int i = 0; i < N; i++) {
        CHECK(s[i].status == 0 && s[i].dst_len > 0 && s[i].dst_len <= d[i].dst_cap);
        CHECK(l[i].status == 0 && l[i].dst_len == s[i].dst_len && memcmp(dst2 + d[i].dst_off, dst + d[i].dst_off, s[i].dst_len) == 0);
        CHECK(p[i].status == 0 && p[i].dst_off == at && p[i].dst_len == s[i].dst_len && memcmp(packed + at, dst + d[i].dst_off, s[i].dst_len) == 0);
        at += s[i].dst_len;
        CHECK(orc_zstd_decompress_chunk(dst + d[i].dst_off, s[i].dst_len, ref, sizes[i]) == (long long)sizes[i] && memcmp(ref, src + d[i].src_off, sizes[i]) == 0);
    }
    {   /* not the exact parse's frame: the profile reached the batch */
        const size_t r3 = orc_zstd_compress_chunk(src + d[1].src_off, sizes[1], ref, dof, 3);
        CHECK(r3 != s[1].dst_len || memcmp(dst + d[1].dst_off, ref, r3) != 0);
        printf("device profile: %u %u %u bytes (level 3: %zu for the second)\n", s[0].dst_len, s[1].dst_len, s[2].dst_len, r3);
    }
    memcpy(p, d, sizeof p);
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, 0, &jp, N, &jsrc, &jpk) == 0);
    CHECK(p[2].status == 0 && p[2].dst_len == s[2].dst_len);
    for (int level = 1; level <= 3; level++) {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = {b, sizeof b};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, level, &jb, N, &jsrc, &jdst2) == TSX_E_UNSUPPORTED);
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, level, &jb, N, &jsrc, &jpk) == TSX_E_UNSUPPORTED);
    }
    {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = {b, sizeof b};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, TSX_COMPRESS, NULL, NULL, 3, &jb, N, &jsrc, &jdst2) == TSX_E_UNSUPPORTED);
    }
    {   /* a fetch whose parameter block names the profile: the library ignores it */
        tsx_chunk_desc e[N]; memset(e, 0, sizeof e);
        size_t fo = 0, oo = 0;
        unsigned char* frames = calloc(dof, 1); unsigned char* back = calloc(so, 1);
        for (int i = 0; i < N; i++) {
            e[i].src_off = fo; e[i].src_len = s[i].dst_len; e[i].dst_off = oo; e[i].dst_cap = sizes[i];
            memcpy(frames + fo, dst + d[i].dst_off, s[i].dst_len);
            fo += ((s[i].dst_len + 15) & ~15u) + 16; oo += ((sizes[i] + 15) & ~15u) + 16;
        }
        tsx_batch_params prm; memset(&prm, 0, sizeof prm);
        prm.flags = TSX_COMPRESS; prm.zstd_profile = TSX_ZSTD_PROFILE_DEVICE;
        CHECK(tsx_detransform_batch(NULL, &prm, e, N, frames, fo, back, oo, TSX_MEM_HOST) == TSX_OK);
        for (int i = 0; i < N; i++) CHECK(e[i].status == 0 && e[i].dst_len == sizes[i] && memcmp(back + e[i].dst_off, src + d[i].src_off, sizes[i]) == 0);
        free(frames); free(back);
    }
    free(src); free(dst); free(dst2); free(packed); free(ref);
    printf("jni device profile ok\n");
    return 0;
}
