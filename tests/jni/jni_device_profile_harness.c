/* TEST HARNESS ONLY: TSX_ZSTD_PROFILE_DEVICE through the natives of the JNI shim (java/jni/tsx_jni.c).  Checks: the profile reaches the
 * batch (the frames are not libzstd's level-3 frames, and the oracle's libzstd restores every chunk from them), transformBatch,
 * transformBatchLevel at level 0 and both packed natives write the same bytes, a level together with the profile comes back as
 * TSX_E_UNSUPPORTED, and a fetch with the profile in its parameter block restores the chunks. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    const uint32_t sizes[N] = {1000, 140001, 60000};
    tsx_chunk_desc d[N];
    size_t so, dof;
    harness_slots(d, sizes, N, TSX_COMPRESS, &so, &dof);
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* dst2 = calloc(dof, 1);
    unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
    harness_log_text(src, so, 999);
    struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jdst2 = JBUF(dst2, dof), jpk = JBUF(packed, dof);
    tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
    CHECK(NATIVE(transformBatch)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
    tsx_chunk_desc l[N]; memcpy(l, d, sizeof l);
    CHECK(NATIVE(transformBatchLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, 0, &JBUF(l, sizeof l), N, &jsrc, &jdst2) == 0);
    tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
    struct _jobject jp = JBUF(p, sizeof p);
    CHECK(NATIVE(transformBatchPacked)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, &jp, N, &jsrc, &jpk) == 0);
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
    CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, 0, &jp, N, &jsrc, &jpk) == 0);
    CHECK(p[2].status == 0 && p[2].dst_len == s[2].dst_len);
    for (int level = 1; level <= 3; level++) {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        struct _jobject jb = JBUF(b, sizeof b);
        CHECK(NATIVE(transformBatchLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, level, &jb, N, &jsrc, &jdst2) == TSX_E_UNSUPPORTED);
        CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, TSX_COMPRESS, NULL, NULL, TSX_ZSTD_PROFILE_DEVICE, level, &jb, N, &jsrc, &jpk) == TSX_E_UNSUPPORTED);
    }
    {
        tsx_chunk_desc b[N]; memcpy(b, d, sizeof b);
        CHECK(NATIVE(transformBatch)(env, NULL, TSX_COMPRESS, NULL, NULL, 3, &JBUF(b, sizeof b), N, &jsrc, &jdst2) == TSX_E_UNSUPPORTED);
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
