/* TEST HARNESS ONLY: the level-taking natives of the JNI shim (TsxNative.transformBatchLevel / transformBatchPackedLevel,
 * java/jni/tsx_jni.c).  Checks: the level reaches the batch (a level-1 frame is libzstd's level-1 frame, checked with the oracle's libzstd),
 * level 0 is level 3, the packed variant writes the same bytes, and a level the library does not implement comes back as TSX_E_UNSUPPORTED. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 30001, 60000};
    tsx_chunk_desc d[N];
    size_t so, dof;
    harness_slots(d, sizes, N, TSX_COMPRESS, &so, &dof);
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    harness_log_text(src, so, 777);
    struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jpk = JBUF(packed, dof);
    for (int level = 0; level <= 3; level++) {
        tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
        CHECK(NATIVE(transformBatchLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
        tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
        CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, level, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
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
    CHECK(NATIVE(transformBatch)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, &JBUF(o, sizeof o), N, &jsrc, &jdst) == 0);
    CHECK(o[2].status == 0 && o[2].dst_len == orc_zstd_compress_chunk(src + d[2].src_off, sizes[2], ref, dof, 3));
    for (int bad = -1; bad <= 22; bad += 1) {
        if (bad >= 0 && bad <= 3) continue;
        if (bad != -1 && bad != 4 && bad != 19 && bad != 22) continue;
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = JBUF(b, sizeof b);
        CHECK(NATIVE(transformBatchLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, bad, &jb, N, &jsrc, &jdst) == TSX_E_UNSUPPORTED);
        CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_1_5_7, bad, &jb, N, &jsrc, &jpk) == TSX_E_UNSUPPORTED);
    }
    free(src); free(dst); free(packed); free(ref);
    printf("jni levels ok\n");
    return 0;
}
