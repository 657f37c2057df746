/* TEST HARNESS ONLY: TsxNative.VERIFY_GCM through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are).  Checks, encrypt-only
 * and compress + encrypt, slot and packed layouts: clean chunks come back TSX_OK with the bytes of a batch without the flag; with the
 * library's test switch verify_damage_out_chunk set (one bit of that chunk's delivered tag), the chunk is TSX_E_VERIFY exactly when the
 * flag is in the batch (so the flag arrives) and delivered - damaged - without it; the flag without TSX_ENCRYPT is refused; detransform
 * ignores it. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(TSX_VERIFY_GCM == 0x80u && TSX_E_VERIFY == -10);
    const uint32_t sizes[N] = {1000, 65537, 30001};
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)(7 * i + 3); aad[i] = (unsigned char)(200 - i); }
    struct _jobject jkey = JBUF(key, 32), jaad = JBUF(aad, 32);
    for (int compress = 0; compress <= 1; compress++) {
        const uint32_t chain = TSX_ENCRYPT | (compress ? TSX_COMPRESS : 0u);
        tsx_chunk_desc d[N];
        size_t so, dof;
        harness_slots(d, sizes, N, chain | TSX_VERIFY_GCM, &so, &dof);
        for (int i = 0; i < N; i++) {
            CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], chain));
            for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(16 * i + k + compress);
        }
        unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
        unsigned char* back = calloc(so, 1);
        harness_log_text(src, so, 99);
        struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jpk = JBUF(packed, dof), jref = JBUF(ref, dof), jback = JBUF(back, so);
        tsx_chunk_desc r[N]; memcpy(r, d, sizeof r);
        CHECK(NATIVE(transformBatch)(env, NULL, (jint)chain, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, &JBUF(r, sizeof r), N, &jsrc, &jref) == 0);
        for (int i = 0; i < N; i++) CHECK(r[i].status == 0 && r[i].dst_len >= 28);
        for (int damaged = 0; damaged <= 1; damaged++) {
            tsx_debug_config("verify_damage_out_chunk", damaged ? 1 : -1); tsx_debug_config("verify_damage_out_off", (long long)r[1].dst_len - 1);   /* last tag byte */
            for (int on = 0; on <= 1; on++) {
                const jint flags = (jint)(chain | (on ? TSX_VERIFY_GCM : 0u));
                tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
                CHECK(NATIVE(transformBatch)(env, NULL, flags, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
                tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
                CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, flags, &jkey, &jaad, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
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
            tsx_chunk_desc b[N];
            harness_fetch_slots(b, d, r, N);
            CHECK(NATIVE(detransformBatch)(env, NULL, (jint)(chain | TSX_VERIFY_GCM), &jkey, &jaad, &JBUF(b, sizeof b), N, &jref, &jback) == 0);
            for (int i = 0; i < N; i++) CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, src + d[i].src_off, sizes[i]) == 0);
        }
        /* the flag without encryption is refused */
        {
            tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
            struct _jobject jb = JBUF(b, sizeof b);
            const jint bad = (jint)(TSX_VERIFY_GCM | (compress ? TSX_COMPRESS : TSX_CRC));
            CHECK(NATIVE(transformBatch)(env, NULL, bad, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jb, N, &jsrc, &jdst) == TSX_E_INVAL);
            CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, bad, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 1, &jb, N, &jsrc, &jpk) == TSX_E_INVAL);
        }
        free(src); free(dst); free(packed); free(ref); free(back);
    }
    printf("jni gcm verify ok\n");
    return 0;
}
