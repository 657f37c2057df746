// TEST HARNESS ONLY: what a host_<feature>.cpp program needs that is not a check: the counting CHECK, the Backend over the libtsxform build
// named on the command line, the program's last line, and the few objects every program builds the same way.
#pragma once
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tsxhost.hpp"
#include "../harness_util.h"

using namespace tsx;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

// the Backend over argv[1]; without that argument the usage line and a null pointer (main returns 2)
static inline std::shared_ptr<Backend> host_backend(int argc, char** argv, const char* program) {
    if (argc < 2) { printf("usage: %s <libtsxform path>\n", program); return nullptr; }
    return std::make_shared<Backend>(argv[1]);
}
static inline int host_done(const char* name) {
    printf("%s: %d failed\n", name, g_failed);
    return g_failed ? 1 : 0;
}

// the library's test switches (tsx_debug_config), from the library the backend has loaded: same handle; null, and a line, if it has none
static inline decltype(&tsx_debug_config) host_debug_config(const char* lib) {
    void* h = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
    auto config = h ? (decltype(&tsx_debug_config))dlsym(h, "tsx_debug_config") : nullptr;
    if (!config) printf("no tsx_debug_config in %s\n", lib);
    return config;
}
static inline Bytes host_log_text(size_t n, uint32_t seed) { Bytes b(n); harness_log_text(b.data(), n, seed); return b; }
static inline std::shared_ptr<BaseTransformChunkEnumeration> host_chunks(const Bytes& data, int chunk) {
    return std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
}
static inline DataKeyAndAAD host_keys() {
    DataKeyAndAAD keys;
    keys.dataKey.resize(32); keys.aad.resize(32);
    for (int i = 0; i < 32; i++) { keys.dataKey[i] = (uint8_t)(5 * i + 1); keys.aad[i] = (uint8_t)(99 + i); }
    return keys;
}
// the same IVs for every enumeration that sets counter = 0 first: the same bytes, option on or off
static inline IvSupplier host_counting_ivs(uint8_t& counter) {
    return [&counter](uint8_t iv[12]) { for (int k = 0; k < 12; k++) iv[k] = (uint8_t)(counter + k); counter++; };
}
template <class E, class F> static bool host_throws(F f) {
    try { f(); } catch (const E&) { return true; }
    return false;
}
