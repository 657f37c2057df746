/* TEST HARNESS ONLY: TsxNative.VERIFY_GCM through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are) with a hand-made JNIEnv
 * (tests/jni/jni.h), as tests/jni/jni_verify_harness.c drives TsxNative.VERIFY.  Checks, encrypt-only and compress + encrypt, slot and
 * packed layouts: clean chunks come back TSX_OK with the bytes of a batch without the flag; with the library's test switch
 * verify_damage_out_chunk set (one bit of that chunk's delivered tag), the chunk is TSX_E_VERIFY exactly when the flag is in the batch (so
 * the flag arrives) and delivered - damaged - without it; the flag without TSX_ENCRYPT is refused; detransform ignores it. */
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
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_detransformBatch(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jobject, jint, jobject, jobject);
long long tsx_debug_config(const char* key, long long value);          /* test hook of the library, not in the header */

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#define N 3
int main(void) {
    JNIEnv envp = &kFns; JNIEnv* env = &envp;
    CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_init(env, NULL) >= 1);
    CHECK(TSX_VERIFY_GCM == 0x80u && TSX_E_VERIFY == -10);
    const uint32_t sizes[N] = {1000, 65537, 30001};
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)(7 * i + 3); aad[i] = (unsigned char)(200 - i); }
    struct _jobject jkey = {key, 32}, jaad = {aad, 32};
    for (int compress = 0; compress <= 1; compress++) {
        const uint32_t chain = TSX_ENCRYPT | (compress ? TSX_COMPRESS : 0u);
        tsx_chunk_desc d[N]; memset(d, 0, sizeof d);
        size_t so = 0, dof = 0;
        for (int i = 0; i < N; i++) {
            d[i].src_off = so; d[i].dst_off = dof; d[i].src_len = sizes[i]; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], chain | TSX_VERIFY_GCM);
            CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], chain));
            for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(16 * i + k + compress);
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
        struct _jobject jsrc = {src, (jlong)so}, jdst = {dst, (jlong)dof}, jpk = {packed, (jlong)dof}, jref = {ref, (jlong)dof}, jback = {back, (jlong)so};
        tsx_chunk_desc r[N]; memcpy(r, d, sizeof r);
        struct _jobject jr = {r, sizeof r};
        CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, (jint)chain, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, &jr, N, &jsrc, &jref) == 0);
        for (int i = 0; i < N; i++) CHECK(r[i].status == 0 && r[i].dst_len >= 28);
        for (int damaged = 0; damaged <= 1; damaged++) {
            tsx_debug_config("verify_damage_out_chunk", damaged ? 1 : -1); tsx_debug_config("verify_damage_out_off", (long long)r[1].dst_len - 1);   /* last tag byte */
            for (int on = 0; on <= 1; on++) {
                const jint flags = (jint)(chain | (on ? TSX_VERIFY_GCM : 0u));
                tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
                struct _jobject js = {s, sizeof s};
                CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, flags, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, &js, N, &jsrc, &jdst) == 0);
                tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
                struct _jobject jp = {p, sizeof p};
                CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, flags, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, 3, &jp, N, &jsrc, &jpk) == 0);
                size_t at = 0;
                for (int i = 0; i < N; i++) {
                    const int hit = damaged && i == 1, fails = hit && on;
                    CHECK(s[i].status == (fails ? TSX_E_VERIFY : 0) && p[i].status == s[i].status && p[i].dst_off == at);
                    if (fails) { CHECK(s[i].dst_len == 0 && p[i].dst_len == 0); continue; }
                    CHECK(s[i].dst_len == r[i].dst_len && p[i].dst_len == r[i].dst_len);
                    if (hit) ref[d[i].dst_off + r[i].dst_len - 1] ^= 1;      /* delivered as the hook left it: one bit of the tag */
                    CHECK(memcmp(dst + d[i].dst_off, ref + d[i].dst_off, r[i].dst_len) == 0 && memcmp(packed + at, ref + d[i].dst_off, r[i].dst_len) == 0);
                    if (hit) ref[d[i].dst_off + r[i].dst_len - 1] ^= 1;
                    at += r[i].dst_len;
                }
                printf("%s, gcm verify %s, output %s: status %d %d %d\n", compress ? "compress + encrypt" : "encrypt", on ? "on" : "off", damaged ? "damaged" : "intact",
                       s[0].status, s[1].status, s[2].status);
            }
        }
        tsx_debug_config("verify_damage_out_chunk", -1);
        /* back through the fetch side's native with the upload's flags word: the flag means nothing there */
        {
            tsx_chunk_desc b[N]; memset(b, 0, sizeof b);
            for (int i = 0; i < N; i++) { b[i].src_off = d[i].dst_off; b[i].src_len = r[i].dst_len; b[i].dst_off = d[i].src_off; b[i].dst_cap = sizes[i]; }
            struct _jobject jb = {b, sizeof b};
            CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_detransformBatch(env, NULL, (jint)(chain | TSX_VERIFY_GCM), &jkey, &jaad, &jb, N, &jref, &jback) == 0);
            for (int i = 0; i < N; i++) CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, src + d[i].src_off, sizes[i]) == 0);
        }
        /* the flag without encryption is refused */
        {
            tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
            struct _jobject jb = {b, sizeof b};
            const jint bad = (jint)(TSX_VERIFY_GCM | (compress ? TSX_COMPRESS : TSX_CRC));
            CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatch(env, NULL, bad, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jb, N, &jsrc, &jdst) == TSX_E_INVAL);
            CHECK(Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_transformBatchPackedLevel(env, NULL, bad, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 1, &jb, N, &jsrc, &jpk) == TSX_E_INVAL);
        }
        free(src); free(dst); free(packed); free(ref); free(back);
    }
    printf("jni gcm verify ok\n");
    return 0;
}
