/* TEST HARNESS ONLY: TsxNative.VERIFY through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are).  Checks: clean chunks come
 * back TSX_OK with the bytes of a batch without the flag, slot and packed layouts alike; with the library's test switch
 * verify_damage_src_chunk set, that chunk is TSX_E_VERIFY exactly when the flag is in the batch (so the flag arrives); the flag without
 * TSX_COMPRESS is refused; detransform ignores it. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(TSX_VERIFY == 0x20u && TSX_E_VERIFY == -10);
    const uint32_t sizes[N] = {1000, 30001, 60000};
    tsx_chunk_desc d[N];
    size_t so, dof;
    harness_slots(d, sizes, N, TSX_COMPRESS | TSX_VERIFY, &so, &dof);
    for (int i = 0; i < N; i++) CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], TSX_COMPRESS));
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    unsigned char* back = calloc(so, 1);
    harness_log_text(src, so, 99);
    struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jpk = JBUF(packed, dof), jref = JBUF(ref, dof), jback = JBUF(back, so);
    tsx_chunk_desc r[N]; memcpy(r, d, sizeof r);
    CHECK(NATIVE(transformBatch)(env, NULL, (jint)TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &JBUF(r, sizeof r), N, &jsrc, &jref) == 0);
    for (int damaged = 0; damaged <= 1; damaged++) {
        tsx_debug_config("verify_damage_src_chunk", damaged ? 1 : -1); tsx_debug_config("verify_damage_src_off", 12345);
        for (int on = 0; on <= 1; on++) {
            const jint flags = (jint)(TSX_COMPRESS | (on ? TSX_VERIFY : 0u));
            tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
            CHECK(NATIVE(transformBatch)(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
            tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
            CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
            size_t at = 0;
            for (int i = 0; i < N; i++) {
                const int fails = damaged && on && i == 1;
                CHECK(s[i].status == (fails ? TSX_E_VERIFY : 0) && p[i].status == s[i].status && p[i].dst_off == at);
                if (fails) { CHECK(s[i].dst_len == 0 && p[i].dst_len == 0); continue; }
                CHECK(s[i].dst_len == r[i].dst_len && memcmp(dst + d[i].dst_off, ref + d[i].dst_off, r[i].dst_len) == 0);
                CHECK(p[i].dst_len == r[i].dst_len && memcmp(packed + at, ref + d[i].dst_off, r[i].dst_len) == 0);
                at += r[i].dst_len;
            }
            printf("verify %s, source %s: status %d %d %d\n", on ? "on" : "off", damaged ? "damaged" : "intact", s[0].status, s[1].status, s[2].status);
        }
    }
    tsx_debug_config("verify_damage_src_chunk", -1);
    /* back through the fetch side's native with the upload's flags word: the flag means nothing there */
    {
        tsx_chunk_desc b[N];
        harness_fetch_slots(b, d, r, N);
        CHECK(NATIVE(detransformBatch)(env, NULL, (jint)(TSX_COMPRESS | TSX_VERIFY), NULL, NULL, &JBUF(b, sizeof b), N, &jref, &jback) == 0);
        for (int i = 0; i < N; i++) CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, src + d[i].src_off, sizes[i]) == 0);
    }
    /* the flag without compression is refused */
    {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = JBUF(b, sizeof b);
        CHECK(NATIVE(transformBatch)(env, NULL, (jint)TSX_VERIFY, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jb, N, &jsrc, &jdst) == TSX_E_INVAL);
        CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, (jint)(TSX_VERIFY | TSX_CRC), NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 1, &jb, N, &jsrc, &jpk) == TSX_E_INVAL);
    }
    free(src); free(dst); free(packed); free(ref); free(back);
    printf("jni verify ok\n");
    return 0;
}
