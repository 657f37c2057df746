/* TEST HARNESS ONLY: the level-taking natives of the JNI shim (TsxNative.transformBatchLevel / transformBatchPackedLevel,
 * java/jni/tsx_jni.c) through a hand-made JNIEnv (tests/jni/jni.h), as tests/jni/jni_harness.c drives the others.  Checks: the level
 * reaches the batch (a level-1 frame is libzstd's level-1 frame, checked with the oracle's libzstd), level 0 is level 3, the packed
 * variant writes the same bytes, and a level the library does not implement comes back as TSX_E_UNSUPPORTED. */
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
size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   /* oracle/zstd_ref.c */

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define N 3
int main(void) {
    JNIEnv envp = &kFns; JNIEnv* env = &envp;
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_init(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 30001, 60000};
    tsx_chunk_desc d[N]; memset(d, 0, sizeof d);
    size_t so = 0, dof = 0;
    for (int i = 0; i < N; i++) {
        d[i].src_off = so; d[i].dst_off = dof; d[i].src_len = sizes[i]; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], TSX_COMPRESS);
        so += ((sizes[i] + 15) & ~15u) + 16; dof += ((d[i].dst_cap + 15) & ~15u) + 16;
    }
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    {   /* log-like text: words of a small vocabulary picked by an LCG */
        static const char* words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
        uint32_t x = 777; size_t i = 0;
        while (i < so) {
            x = x * 1103515245u + 12345u;
            const char* w = words[(x >> 16) % 12];
            for (size_t k = 0; w[k] && i < so; k++) src[i++] = (unsigned char)w[k];
            if (((x >> 8) & 7) == 0 && i < so) src[i++] = (unsigned char)('0' + ((x >> 20) % 10));
        }
    }
    struct _jobject jsrc = {src, (jlong)so}, jdst = {dst, (jlong)dof}, jpk = {packed, (jlong)dof};
    for (int level = 0; level <= 3; level++) {
        tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
        struct _jobject js = {s, sizeof s};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &js, N, &jsrc, &jdst) == 0);
        tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
        struct _jobject jp = {p, sizeof p};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &jp, N, &jsrc, &jpk) == 0);
        size_t at = 0;
        for (int i = 0; i < N; i++) {
            const size_t r = orc_zstd_compress_chunk(src + d[i].src_off, sizes[i], ref, dof, level ? level : 3);
            CHECK(s[i].status == 0 && s[i].dst_len == r && memcmp(dst + d[i].dst_off, ref, r) == 0);
            CHECK(p[i].status == 0 && p[i].dst_off == at && p[i].dst_len == r && memcmp(packed + at, ref, r) == 0);
            at += r;
        }
        if (level == 1) {                                    /* a level-1 frame is not the default frame: the level reached the batch */
            const size_t r3 = orc_zstd_compress_chunk(src + d[2].src_off, sizes[2], ref, dof, 3);
            CHECK(r3 != s[2].dst_len || memcmp(dst + d[2].dst_off, ref, r3) != 0);
        }
        printf("level %d: %u %u %u bytes\n", level, s[0].dst_len, s[1].dst_len, s[2].dst_len);
    }
    /* the old native is level 0 */
    tsx_chunk_desc o[N]; memcpy(o, d, sizeof o);
    struct _jobject jo = {o, sizeof o};
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jo, N, &jsrc, &jdst) == 0);
    CHECK(o[2].status == 0 && o[2].dst_len == orc_zstd_compress_chunk(src + d[2].src_off, sizes[2], ref, dof, 3));
    for (int bad = -1; bad <= 22; bad += 1) {
        if (bad >= 0 && bad <= 3) continue;
        if (bad != -1 && bad != 4 && bad != 19 && bad != 22) continue;
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = {b, sizeof b};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, bad, &jb, N, &jsrc, &jdst) == TSX_E_UNSUPPORTED);
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, bad, &jb, N, &jsrc, &jpk) == TSX_E_UNSUPPORTED);
    }
    free(src); free(dst); free(packed); free(ref);
    printf("jni levels ok\n");
    return 0;
}
