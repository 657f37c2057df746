/* TEST HARNESS ONLY: a segment validated over several batches through the JNI shim (java/jni/tsx_jni.c: recordsBegin, transformBatchStream,
 * transformBatchPackedStream, recordsResult - the state in a direct ByteBuffer of 192 bytes).  jni_records_harness.c's stream - three chunks
 * that are, in order, five hand-made v2 record batches, batch 3 begins in chunk 0 and ends in chunk 2 - in batches of TWO chunks; plain,
 * encrypt and compress + encrypt chains, slot and packed layouts: clean, both batches come back TSX_OK with the bytes of the same batches
 * without the flag and the result is complete; with one bit of batch 3's crc field flipped the first batch is delivered and the second is
 * TSX_E_RECORDS, and the result names the position and the reason; a declared length one byte too long never completes. */
#include "jni_fake.h"
#include "../harness_util.h"

jint NATIVE(recordsBegin)(JNIEnv*, jclass, jobject, jlong);
jint NATIVE(transformBatchStream)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject, jobject);
jint NATIVE(transformBatchPackedStream)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject, jobject);
jint NATIVE(recordsResult)(JNIEnv*, jclass, jobject, jobject);

#define N 3
#define BATCHES 5
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(sizeof(tsx_records_state) == 192 && TSX_RECORDS_STATE_BYTES == 192 && sizeof(tsx_records_info) == 40);
    const uint32_t blen[BATCHES] = {700, 30000, 61, 52000, 18239};           /* 101000 bytes; batch 3 begins in chunk 0 and ends in chunk 2 */
    const uint32_t sizes[N] = {40000, 40001, 20999};
    unsigned char* stream = malloc(101000);
    uint32_t bat[BATCHES], at0 = 0;
    for (int b = 0; b < BATCHES; b++) { bat[b] = at0; harness_record_batch(stream + at0, blen[b], (uint32_t)b, "offset=key=value=ts=\n", 7); at0 += blen[b]; }
    CHECK(at0 == 101000 && bat[3] < 40000 && bat[3] + blen[3] > 80001);
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)(7 * i + 3); aad[i] = (unsigned char)(200 - i); }
    struct _jobject jkey = JBUF(key, 32), jaad = JBUF(aad, 32);
    /* the state: a direct buffer of exactly its size; anything smaller, or none, is refused */
    tsx_records_state* st = malloc(sizeof *st);
    tsx_records_info info;
    struct _jobject jst = JBUF(st, sizeof *st), jsmall = JBUF(st, sizeof *st - 1), jinfo = JBUF(&info, sizeof info), jinfosmall = JBUF(&info, sizeof info - 1);
    CHECK(NATIVE(recordsBegin)(env, NULL, &jsmall, 5) == TSX_E_INVAL && NATIVE(recordsBegin)(env, NULL, NULL, 5) == TSX_E_INVAL && NATIVE(recordsBegin)(env, NULL, &jst, -1) == TSX_E_INVAL);
    memset(st, 0, sizeof *st);
    CHECK(NATIVE(recordsResult)(env, NULL, &jst, &jinfo) == TSX_E_INVAL);      /* never begun */
    CHECK(NATIVE(recordsBegin)(env, NULL, &jst, 101000) == 0);
    CHECK(NATIVE(recordsResult)(env, NULL, &jst, &jinfosmall) == TSX_E_INVAL && NATIVE(recordsResult)(env, NULL, &jsmall, &jinfo) == TSX_E_INVAL);
    CHECK(NATIVE(recordsResult)(env, NULL, &jst, &jinfo) == 0 && info.batches == 0 && info.first_bad_pos == UINT64_MAX);
    const uint32_t chains[3] = {0u, TSX_ENCRYPT, TSX_ENCRYPT | TSX_COMPRESS};
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int c = 0; c < 3; c++) {
        const uint32_t chain = chains[c];
        struct _jobject* const jk = chain & TSX_ENCRYPT ? &jkey : NULL; struct _jobject* const ja = chain & TSX_ENCRYPT ? &jaad : NULL;
        for (int packed = 0; packed <= 1; packed++) {
            /* variant 0: clean; 1: batch 3's crc field; 2: clean, declared one byte too long */
            for (int variant = 0; variant <= 2; variant++) {
                if (variant == 1) stream[bat[3] + 18] ^= 1;
                CHECK(NATIVE(recordsBegin)(env, NULL, &jst, 101000 + (variant == 2)) == 0);
                int status[N], done = -1;
                for (int call = 0; call < 2; call++) {
                    const int lo = call * 2, n = call ? 1 : 2;
                    tsx_chunk_desc d[2], r[2];
                    size_t so, dof;
                    harness_slots(d, sizes + lo, n, chain, &so, &dof);
                    for (int i = 0; i < n; i++) for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(16 * (lo + i) + k + c);
                    unsigned char* src = malloc(so); unsigned char* dst = calloc(dof, 1); unsigned char* ref = calloc(dof, 1);
                    memset(src, 0x5A, so);
                    uint32_t at = lo ? sizes[0] + sizes[1] : 0;
                    for (int i = 0; i < n; i++) { memcpy(src + d[i].src_off, stream + at, sizes[lo + i]); at += sizes[lo + i]; }
                    struct _jobject jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jref = JBUF(ref, dof);
                    memcpy(r, d, sizeof r);
                    CHECK((packed ? NATIVE(transformBatchPackedLevel) : NATIVE(transformBatchLevel))(env, NULL, (jint)chain, jk, ja, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(r, sizeof r), n, &jsrc, &jref) == 0);
                    /* without a state the stream natives refuse; without the flag the library does, and the state stays */
                    tsx_chunk_desc s[2]; memcpy(s, d, sizeof s);
                    tsx_records_state before = *st;
                    CHECK(NATIVE(transformBatchStream)(env, NULL, (jint)(chain | TSX_VALIDATE_RECORDS), jk, ja, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(s, sizeof s), n, &jsrc, &jdst, NULL) == TSX_E_INVAL);
                    CHECK(NATIVE(transformBatchPackedStream)(env, NULL, (jint)chain, jk, ja, TSX_ZSTD_PROFILE_1_5_7, 3, &JBUF(s, sizeof s), n, &jsrc, &jdst, &jst) == TSX_E_INVAL);
                    CHECK(memcmp(&before, st, sizeof before) == 0);
                    CHECK((packed ? NATIVE(transformBatchPackedStream) : NATIVE(transformBatchStream))(env, NULL, (jint)(chain | TSX_VALIDATE_RECORDS), jk, ja, TSX_ZSTD_PROFILE_1_5_7, 3,
                                                                                                       &JBUF(s, sizeof s), n, &jsrc, &jdst, &jst) == 0);
                    for (int i = 0; i < n; i++) {
                        status[lo + i] = s[i].status;
                        CHECK(r[i].status == 0 && r[i].dst_len > 0);
                        if (s[i].status == 0) CHECK(s[i].dst_len == r[i].dst_len && s[i].dst_off == r[i].dst_off && memcmp(dst + s[i].dst_off, ref + r[i].dst_off, r[i].dst_len) == 0);
                        else CHECK(s[i].dst_len == 0);
                    }
                    done = NATIVE(recordsResult)(env, NULL, &jst, &jinfo);
                    CHECK(done == (call == 1 && variant != 2 ? 1 : 0));
                    free(src); free(dst); free(ref);
                }
                if (variant == 1) {
                    CHECK(status[0] == 0 && status[1] == 0 && status[2] == TSX_E_RECORDS && info.first_bad_pos == bat[3] && info.first_bad_reason == 4 && info.batches == 3);
                    stream[bat[3] + 18] ^= 1;
                } else CHECK(status[0] == 0 && status[1] == 0 && status[2] == 0 && info.batches == BATCHES && info.first_bad_reason == 0 && info.first_bad_pos == UINT64_MAX);
                printf("%s, %s, %s: status %d %d %d, complete %d, first bad %lld reason %u\n", names[c], packed ? "packed" : "slots",
                       variant == 0 ? "source intact" : variant == 1 ? "source damaged in batch 3" : "declared one byte too long", status[0], status[1], status[2], done,
                       (long long)info.first_bad_pos, info.first_bad_reason);
            }
        }
    }
    free(st); free(stream);
    printf("jni records stream ok\n");
    return 0;
}
