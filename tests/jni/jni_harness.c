/* TEST HARNESS ONLY: drives the JNI shim (java/jni/tsx_jni.c) the way TsxNative's native methods would, through the hand-made JNIEnv
 * of tests/jni/jni_fake.h.  Checks: init, transformedBound, a transform/detransform round trip through direct buffers, packed output,
 * the per-chunk "Tag mismatch" of a forged chunk, rejection of a descriptor that points beyond the src buffer. */
#include "jni_fake.h"
#include "../harness_util.h"

#define N 5
int main(void) {
    JNI_ENV(env);
    CHECK(NATIVE(init)(env, NULL) >= 1);
    CHECK(NATIVE(deviceCount)(env, NULL) >= 1);
    CHECK(NATIVE(setThreadDevice)(env, NULL, 0) == 0);
    CHECK(NATIVE(setThreadDevice)(env, NULL, 99) == TSX_E_INVAL);
    const int flags = TSX_ENCRYPT | TSX_CRC;
    CHECK(NATIVE(transformedBound)(env, NULL, 4194304, TSX_ENCRYPT) == 4194332);
    unsigned char key[32], aad[32];
    for (int i = 0; i < 32; i++) { key[i] = (unsigned char)i; aad[i] = (unsigned char)(32 + i); }
    struct _jobject jkey = JBUF(key, 32), jaad = JBUF(aad, 32);
    const uint32_t sizes[N] = {0, 1, 1000, 65537, 70001};
    tsx_chunk_desc d[N];
    size_t so, dof;
    harness_slots(d, sizes, N, flags, &so, &dof);                              /* dst_cap = size + 28 */
    for (int i = 0; i < N; i++) for (int k = 0; k < 12; k++) d[i].iv[k] = (uint8_t)(i * 16 + k);
    unsigned char* src = calloc(so, 1); unsigned char* dst = calloc(dof, 1); unsigned char* back = calloc(so, 1); unsigned char* packed = calloc(dof, 1);
    for (size_t i = 0; i < so; i++) src[i] = (unsigned char)(i * 131 + (i >> 9));
    struct _jobject jd = JBUF(d, sizeof d), jsrc = JBUF(src, so), jdst = JBUF(dst, dof), jback = JBUF(back, so), jpk = JBUF(packed, dof);
    CHECK(NATIVE(hostRegister)(env, NULL, &jsrc) == 0);
    CHECK(NATIVE(transformBatch)(env, NULL, flags, &jkey, &jaad, 0, &jd, N, &jsrc, &jdst) == 0);
    CHECK(NATIVE(hostUnregister)(env, NULL, &jsrc) == 0);
    uint32_t crc[N];
    for (int i = 0; i < N; i++) { CHECK(d[i].status == 0 && d[i].dst_len == sizes[i] + 28); crc[i] = d[i].crc32c; CHECK(memcmp(dst + d[i].dst_off, d[i].iv, 12) == 0); }
    /* packed: same bytes, back to back */
    tsx_chunk_desc p[N]; memcpy(p, d, sizeof p);
    CHECK(NATIVE(transformBatchPacked)(env, NULL, flags, &jkey, &jaad, 0, &JBUF(p, sizeof p), N, &jsrc, &jpk) == 0);
    size_t at = 0;
    for (int i = 0; i < N; i++) { CHECK(p[i].status == 0 && p[i].dst_off == at && p[i].dst_len == d[i].dst_len); CHECK(memcmp(packed + at, dst + d[i].dst_off, d[i].dst_len) == 0); at += p[i].dst_len; }
    /* inverse, chunk 3 forged */
    dst[d[3].dst_off + 40] ^= 1;
    tsx_chunk_desc e[N];
    harness_fetch_slots(e, d, d, N);
    CHECK(NATIVE(detransformBatch)(env, NULL, flags, &jkey, &jaad, &JBUF(e, sizeof e), N, &jdst, &jback) == 0);
    for (int i = 0; i < N; i++) {
        if (i == 3) { CHECK(e[i].status == TSX_E_TAG_MISMATCH && e[i].dst_len == 0); continue; }
        CHECK(e[i].status == 0 && e[i].dst_len == sizes[i] && e[i].crc32c == crc[i]);
        CHECK(memcmp(back + e[i].dst_off, src + d[i].src_off, sizes[i]) == 0);
    }
    jstring s = NATIVE(strerror)(env, NULL, TSX_E_TAG_MISMATCH);
    CHECK(strcmp((const char*)s->addr, "Tag mismatch") == 0);
    /* a descriptor that reaches beyond the src ByteBuffer never gets to the library */
    tsx_chunk_desc bad[1]; memcpy(bad, d, sizeof bad); bad[0].src_off = so - 16; bad[0].src_len = 64;
    CHECK(NATIVE(transformBatch)(env, NULL, flags, &jkey, &jaad, 0, &JBUF(bad, sizeof bad), 1, &jsrc, &jdst) == TSX_E_INVAL);
    /* wrong key length */
    CHECK(NATIVE(transformBatch)(env, NULL, flags, &JBUF(key, 16), &jaad, 0, &jd, N, &jsrc, &jdst) == TSX_E_INVAL);
    printf("jni shim ok\n");
    return 0;
}
