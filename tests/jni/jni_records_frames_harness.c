/* TEST HARNESS ONLY: TsxNative.VALIDATE_FRAMES through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are).  Three chunks that
 * are, in order, one stream of five well-framed v2 record batches; plain, encrypt and compress + encrypt chains: a clean stream comes back
 * TSX_OK with the bytes of a batch without the flag; with one batch's recordsCount raised by one and the batch SEALED with a fresh CRC, the
 * chunk that batch begins in and the chunks behind it are TSX_E_RECORDS exactly when the flag is in the batch (so the flag arrives) -
 * TSX_VALIDATE_RECORDS alone finds nothing; the flag without TSX_VALIDATE_RECORDS is refused; detransform ignores it. */
#include "jni_fake.h"
#include "../records_frames_harness.h"

#define N 3
#define BATCHES 5
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(TSX_VALIDATE_FRAMES == 0x400u && TSX_VALIDATE_RECORDS == 0x100u && TSX_E_RECORDS == -11);
    const uint32_t nrec[BATCHES] = {3, 40, 1, 60, 20}, vlen[BATCHES] = {200, 700, 5, 900, 800};
    unsigned char* stream = malloc(200000);
    uint32_t bat[BATCHES + 1], total = 0;
    for (int b = 0; b < BATCHES; b++) { bat[b] = total; total += frames_batch(stream + total, (uint32_t)(100 * b), nrec[b], vlen[b], "offset=key=value=ts=\n"); }
    bat[BATCHES] = total;
    const uint32_t sizes[N] = {40000, 40001, total - 80001};
    CHECK(total > 90000 && total < 200000 && bat[3] < 40000 && bat[4] > 80001);      /* batch 3 begins in chunk 0 and ends in chunk 2 */
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)(7 * i + 3); aad[i] = (unsigned char)(200 - i); }
    struct _jobject jkey = JBUF(key, 32), jaad = JBUF(aad, 32);
    const uint32_t chains[3] = {0u, TSX_ENCRYPT, TSX_ENCRYPT | TSX_COMPRESS};
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int c = 0; c < 3; c++) {
        const uint32_t chain = chains[c];
        tsx_chunk_desc d[N];
        size_t so, dof;
        harness_slots(d, sizes, N, chain | TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES, &so, &dof);
        for (int i = 0; i < N; i++) {
            CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], chain));
            for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(16 * i + k + c);
        }
        unsigned char* src = malloc(so); unsigned char* dst = calloc(dof, 1); unsigned char* ref = calloc(dof, 1); unsigned char* back = calloc(so, 1);
        memset(src, 0x5A, so);                                                  /* the gaps between the slots are no part of the stream */
        struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jref = JBUF(ref, dof), jback = JBUF(back, so);
        struct _jobject* const jk = chain & TSX_ENCRYPT ? &jkey : NULL; struct _jobject* const ja = chain & TSX_ENCRYPT ? &jaad : NULL;
        tsx_chunk_desc r[N];
        for (int which = -1; which <= 4; which += (which < 0 ? 4 : 1)) {       /* intact; batch 3 (begins in chunk 0); batch 4 (in chunk 2) */
            unsigned char* s2 = malloc(total);
            memcpy(s2, stream, total);
            if (which >= 0) {
                harness_be32(s2 + bat[which] + 57, nrec[which] + 1);
                frames_seal(s2 + bat[which], bat[which + 1] - bat[which]);
            }
            uint32_t at = 0;
            for (int i = 0; i < N; i++) { memcpy(src + d[i].src_off, s2 + at, sizes[i]); at += sizes[i]; }
            free(s2);
            const int first_bad = which < 0 ? N : which == 3 ? 0 : 2;
            memcpy(r, d, sizeof r);
            CHECK(NATIVE(transformBatch)(env, NULL, (jint)chain, jk, ja, TSX_ZSTD_PROFILE_1_5_7, &JBUF(r, sizeof r), N, &jsrc, &jref) == 0);
            for (int k = 0; k < N; k++) CHECK(r[k].status == 0 && r[k].dst_len > 0);
            for (int on = 0; on <= 1; on++) {
                const jint flags = (jint)(chain | TSX_VALIDATE_RECORDS | (on ? TSX_VALIDATE_FRAMES : 0u));
                tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
                CHECK(NATIVE(transformBatch)(env, NULL, flags, jk, ja, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
                for (int k = 0; k < N; k++) {
                    const int fails = on && k >= first_bad;
                    CHECK(s[k].status == (fails ? TSX_E_RECORDS : 0));
                    if (fails) { CHECK(s[k].dst_len == 0); continue; }
                    CHECK(s[k].dst_len == r[k].dst_len && memcmp(dst + d[k].dst_off, ref + d[k].dst_off, r[k].dst_len) == 0);
                }
                printf("%s, records validate on, frames %s, source %s%s: status %d %d %d\n", names[c], on ? "on" : "off", which < 0 ? "intact" : "sealed with a wrong count in batch ",
                       which < 0 ? "" : which == 3 ? "3" : "4", s[0].status, s[1].status, s[2].status);
            }
            if (which < 0) {                                                    /* the flag alone: refused, nothing is touched */
                tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
                s[0].status = 77;
                CHECK(NATIVE(transformBatch)(env, NULL, (jint)(chain | TSX_VALIDATE_FRAMES), jk, ja, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == TSX_E_INVAL);
                CHECK(s[0].status == 77);
                printf("%s, frames without records validate: refused\n", names[c]);
                /* back through the fetch side's native with the upload's flags word: the flags mean nothing there */
                tsx_chunk_desc b[N];
                harness_fetch_slots(b, d, r, N);
                CHECK(NATIVE(detransformBatch)(env, NULL, (jint)(chain | TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES), jk, ja, &JBUF(b, sizeof b), N, &jref, &jback) == 0);
                at = 0;
                for (int i = 0; i < N; i++) { CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, stream + at, sizes[i]) == 0); at += sizes[i]; }
            }
        }
        free(src); free(dst); free(ref); free(back);
    }
    free(stream);
    printf("jni records frames ok\n");
    return 0;
}
