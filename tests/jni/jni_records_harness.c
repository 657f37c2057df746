/* TEST HARNESS ONLY: TsxNative.VALIDATE_RECORDS through the JNI shim (java/jni/tsx_jni.c passes `flags` on as they are).  Three chunks that
 * are, in order, one stream of five hand-made v2 record batches; plain, encrypt and compress + encrypt chains, slot and packed layouts: a
 * clean stream comes back TSX_OK with the bytes of a batch without the flag; with one bit of a batch's crc field flipped in the source, the
 * chunk that batch begins in and the chunks behind it are TSX_E_RECORDS exactly when the flag is in the batch (so the flag arrives);
 * detransform ignores it. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 3
#define BATCHES 5
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(TSX_VALIDATE_RECORDS == 0x100u && TSX_E_RECORDS == -11);
    const uint32_t blen[BATCHES] = {700, 30000, 61, 52000, 18239};           /* 101000 bytes; batch 3 begins in chunk 0 and ends in chunk 2 */
    const uint32_t sizes[N] = {40000, 40001, 20999};
    unsigned char* stream = malloc(101000);
    uint32_t bat[BATCHES], at0 = 0;
    for (int b = 0; b < BATCHES; b++) { bat[b] = at0; harness_record_batch(stream + at0, blen[b], (uint32_t)b, "offset=key=value=ts=\n", 7); at0 += blen[b]; }
    CHECK(at0 == 101000 && bat[3] < 40000 && bat[4] > 80001);
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)(7 * i + 3); aad[i] = (unsigned char)(200 - i); }
    struct _jobject jkey = JBUF(key, 32), jaad = JBUF(aad, 32);
    const uint32_t chains[3] = {0u, TSX_ENCRYPT, TSX_ENCRYPT | TSX_COMPRESS};
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int c = 0; c < 3; c++) {
        const uint32_t chain = chains[c];
        tsx_chunk_desc d[N];
        size_t so, dof;
        harness_slots(d, sizes, N, chain | TSX_VALIDATE_RECORDS, &so, &dof);
        for (int i = 0; i < N; i++) {
            CHECK(d[i].dst_cap == tsx_transformed_bound(sizes[i], chain));
            for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(16 * i + k + c);
        }
        unsigned char* src = malloc(so); unsigned char* dst = calloc(dof, 1); unsigned char* packed = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
        unsigned char* back = calloc(so, 1);
        memset(src, 0x5A, so);                                                  /* the gaps between the slots are no part of the stream */
        struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jpk = JBUF(packed, dof), jref = JBUF(ref, dof), jback = JBUF(back, so);
        struct _jobject* const jk = chain & TSX_ENCRYPT ? &jkey : NULL; struct _jobject* const ja = chain & TSX_ENCRYPT ? &jaad : NULL;
        tsx_chunk_desc r[N];
        for (int damaged = 0; damaged <= 1; damaged++) {
            /* batch 3's crc field: the batch begins in chunk 0 -> every chunk fails; batch 4's: it begins in chunk 2 -> that chunk alone */
            for (int which = 3; which <= (damaged ? 4 : 3); which++) {
                uint32_t at = 0;
                for (int i = 0; i < N; i++) { memcpy(src + d[i].src_off, stream + at, sizes[i]); at += sizes[i]; }
                const int first_bad = !damaged ? N : which == 3 ? 0 : 2;
                if (damaged) {
                    const uint32_t pos = bat[which] + 18;
                    uint32_t lo = 0; int i = 0;
                    while (pos >= lo + sizes[i]) { lo += sizes[i]; i++; }
                    src[d[i].src_off + (pos - lo)] ^= 1;
                }
                if (!damaged) {
                    memcpy(r, d, sizeof r);
                    CHECK(NATIVE(transformBatch)(env, NULL, (jint)chain, jk, ja, TSX_ZSTD_PROFILE_1_5_7, &JBUF(r, sizeof r), N, &jsrc, &jref) == 0);
                    for (int k = 0; k < N; k++) CHECK(r[k].status == 0 && r[k].dst_len > 0);
                }
                for (int on = 0; on <= 1; on++) {
                    const jint flags = (jint)(chain | (on ? TSX_VALIDATE_RECORDS : 0u));
                    tsx_chunk_desc s[N]; memcpy(s, d, sizeof s);
                    CHECK(NATIVE(transformBatch)(env, NULL, flags, jk, ja, TSX_ZSTD_PROFILE_1_5_7, &JBUF(s, sizeof s), N, &jsrc, &jdst) == 0);
                    tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
                    CHECK(NATIVE(transformBatchPackedLevel)(env, NULL, flags, jk, ja, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
                    size_t pat = 0;
                    for (int k = 0; k < N; k++) {
                        const int fails = on && k >= first_bad;
                        CHECK(s[k].status == (fails ? TSX_E_RECORDS : 0) && p[k].status == s[k].status && p[k].dst_off == pat);
                        if (fails) { CHECK(s[k].dst_len == 0 && p[k].dst_len == 0); continue; }
                        CHECK(s[k].dst_len > 0 && p[k].dst_len == s[k].dst_len && memcmp(dst + d[k].dst_off, packed + pat, s[k].dst_len) == 0);
                        if (!damaged) CHECK(s[k].dst_len == r[k].dst_len && memcmp(dst + d[k].dst_off, ref + d[k].dst_off, r[k].dst_len) == 0);
                        pat += p[k].dst_len;
                    }
                    printf("%s, records validate %s, source %s%s: status %d %d %d\n", names[c], on ? "on" : "off", damaged ? "damaged in batch " : "intact",
                           damaged ? (which == 3 ? "3" : "4") : "", s[0].status, s[1].status, s[2].status);
                }
            }
        }
        /* back through the fetch side's native with the upload's flags word: the flag means nothing there */
        {
            tsx_chunk_desc b[N];
            harness_fetch_slots(b, d, r, N);
            CHECK(NATIVE(detransformBatch)(env, NULL, (jint)(chain | TSX_VALIDATE_RECORDS), jk, ja, &JBUF(b, sizeof b), N, &jref, &jback) == 0);
            uint32_t at = 0;
            for (int i = 0; i < N; i++) { CHECK(b[i].status == 0 && b[i].dst_len == sizes[i] && memcmp(back + d[i].src_off, stream + at, sizes[i]) == 0); at += sizes[i]; }
        }
        free(src); free(dst); free(packed); free(ref); free(back);
    }
    free(stream);
    printf("jni records ok\n");
    return 0;
}
