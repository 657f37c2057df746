/* TEST HARNESS ONLY: everything a JNI harness needs that is not a check.  The hand-made JNIEnv behind tests/jni/jni.h - byte[] and direct
 * ByteBuffers are plain structs here -, the prototypes of every native of java/jni/tsx_jni.c, and the CHECK that ends main.  A harness is
 * compiled together with the shim and linked against a libtsxform build by tests/hostjni.py. */
#ifndef TSX_TEST_JNI_FAKE_H
#define TSX_TEST_JNI_FAKE_H
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jni.h"
#include "tsxform.h"

struct _jobject { void* addr; jlong cap; };             /* a direct ByteBuffer, a byte[] (cap = length) or a String (addr = chars) */
static jsize f_len(JNIEnv* e, jbyteArray a) { (void)e; return (jsize)a->cap; }
static void f_region(JNIEnv* e, jbyteArray a, jsize off, jsize n, jbyte* out) { (void)e; memcpy(out, (char*)a->addr + off, (size_t)n); }
static void* f_addr(JNIEnv* e, jobject b) { (void)e; return b ? b->addr : NULL; }
static jlong f_cap(JNIEnv* e, jobject b) { (void)e; return b ? b->cap : -1; }
static jstring f_str(JNIEnv* e, const char* s) { (void)e; jobject o = malloc(sizeof *o); o->addr = strdup(s); o->cap = (jlong)strlen(s); return o; }
static const struct JNINativeInterface_ kFns = {f_len, f_region, f_addr, f_cap, f_str};

#define JBUF(ptr, cap) ((struct _jobject){(void*)(ptr), (jlong)(cap)})             /* an lvalue: pass &JBUF(p, n), or keep it in a variable */
#define JNI_ENV(env) JNIEnv envp = &kFns; JNIEnv* env = &envp
#define NATIVE(name) Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_##name

jint NATIVE(init)(JNIEnv*, jclass);
jstring NATIVE(strerror)(JNIEnv*, jclass, jint);
jlong NATIVE(transformedBound)(JNIEnv*, jclass, jlong, jint);
jint NATIVE(setThreadDevice)(JNIEnv*, jclass, jint);
jint NATIVE(deviceCount)(JNIEnv*, jclass);
jint NATIVE(hostRegister)(JNIEnv*, jclass, jobject);
jint NATIVE(hostUnregister)(JNIEnv*, jclass, jobject);
jint NATIVE(transformBatch)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jobject, jint, jobject, jobject);
jint NATIVE(transformBatchPacked)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jobject, jint, jobject, jobject);
jint NATIVE(transformBatchLevel)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint NATIVE(transformBatchPackedLevel)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jint, jint, jobject, jint, jobject, jobject);
jint NATIVE(detransformBatch)(JNIEnv*, jclass, jint, jbyteArray, jbyteArray, jobject, jint, jobject, jobject);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
#endif
