/* TEST HARNESS ONLY: TsxNative.ZSTD_CHECKSUM through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are).  Checks: with the
 * flag the frames carry bit 2 and libzstd's checksum (the real libzstd the oracle has loaded, ZSTD_c_checksumFlag), slot and packed layouts
 * alike, at the default level and at level 1; without it today's bytes; the flag without TSX_COMPRESS is refused; detransform restores
 * checksummed frames. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 30001, 60000};
    tsx_chunk_desc d[N];
    size_t so, dof;
    harness_slots(d, sizes, N, TSX_COMPRESS | TSX_ZSTD_CHECKSUM, &so, &dof);
    for (int i = 0; i < N; i++) CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], TSX_COMPRESS));        /* the bound covers the four bytes already */
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    unsigned char* back = calloc(so, 1);
    harness_log_text(src, so, 99);
    struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jpk = JBUF(packed, dof), jback = JBUF(back, so);
    for (int on = 0; on <= 1; on++) {
        const jint flags = (jint)(TSX_COMPRESS | (on ? TSX_ZSTD_CHECKSUM : 0u));
        for (int level = 0; level <= 1; level++) {
            tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
            struct _jobject js = JBUF(s, sizeof s);
            if (level == 0) CHECK(NATIVE(transformBatch)(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &js, N, &jsrc, &jdst) == 0);
            else CHECK(NATIVE(transformBatchLevel)(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &js, N, &jsrc, &jdst) == 0);
            tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
            CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, flags, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
            size_t at = 0;
            for (int i = 0; i < N; i++) {
                const int lv = level ? level : 3;
                const size_t r = on ? harness_libzstd_checksummed(src + d[i].src_off, sizes[i], ref, dof, lv) : orc_zstd_compress_chunk(src + d[i].src_off, sizes[i], ref, dof, lv);
                CHECK(r != (size_t)-1 && ((ref[4] >> 2) & 1) == on);
                CHECK(s[i].status == 0 && s[i].dst_len == r && memcmp(dst + d[i].dst_off, ref, r) == 0);
                CHECK(p[i].status == 0 && p[i].dst_off == at && p[i].dst_len == r && memcmp(packed + at, ref, r) == 0);
                at += r;
            }
            /* back through the fetch side's native: no flag needed, the frame decides */
            tsx_chunk_desc b[N];
            harness_fetch_slots(b, d, s, N);
            memset(back, 0, so);
            CHECK(NATIVE(detransformBatch)(env, NULL, TSX_COMPRESS, NULL, NULL, &JBUF(b, sizeof b), N, &jdst, &jback) == 0);
            for (int i = 0; i < N; i++) CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, src + d[i].src_off, sizes[i]) == 0);
            printf("checksum %s, level %d: %u %u %u bytes\n", on ? "on" : "off", level, s[0].dst_len, s[1].dst_len, s[2].dst_len);
        }
    }
    /* a damaged checksummed frame comes back as a corrupt frame, where a ZstdException would surface */
    {
        tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
        CHECK(NATIVE(transformBatch)(env, NULL, (jint)(TSX_COMPRESS | TSX_ZSTD_CHECKSUM), NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
        dst[d[1].dst_off + s[1].dst_len - 2] ^= 0x10;                     /* inside chunk 1's checksum */
        tsx_chunk_desc b[N];
        harness_fetch_slots(b, d, s, N);
        CHECK(NATIVE(detransformBatch)(env, NULL, TSX_COMPRESS, NULL, NULL, &JBUF(b, sizeof b), N, &jdst, &jback) == 0);
        CHECK(b[0].status == 0 && b[1].status == TSX_E_BAD_FRAME && b[1].dst_len == 0 && b[2].status == 0);
    }
    /* the flag without compression is refused */
    {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = JBUF(b, sizeof b);
        CHECK(NATIVE(transformBatch)(env, NULL, (jint)TSX_ZSTD_CHECKSUM, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &jb, N, &jsrc, &jdst) == TSX_E_INVAL);
        CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, (jint)(TSX_ZSTD_CHECKSUM | TSX_CRC), NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, 1, &jb, N, &jsrc, &jpk) == TSX_E_INVAL);
    }
    free(src); free(dst); free(packed); free(ref); free(back);
    printf("jni checksum ok\n");
    return 0;
}
