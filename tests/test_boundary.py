"""The drop-in boundary: the C-ABI library loads, exports every symbol include/tsxform.h declares, its structs
have the documented layout, and the product never reaches into oracle/ (no compute calls here: no GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

import tsxform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiered-storage-for-apache-kafka_amd")
nat = tsxform._native


def header_functions():
    h = open(os.path.join(ROOT, "include", "tsxform.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(tsx_[a-z0-9_]+)\s*\(", h)))


@pytest.fixture(scope="module")
def product_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "csrc")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert os.path.exists(nat.LIB_PATH)
    return nat.LIB_PATH


def test_header_and_binding_agree():
    assert header_functions() == sorted(nat.EXPORTS)


def test_library_loads_and_exports_every_declared_symbol(product_lib):
    lib = ctypes.CDLL(product_lib)
    for name in header_functions():
        assert hasattr(lib, name), name
    lib.tsx_abi_version.restype = ctypes.c_uint32
    assert lib.tsx_abi_version() == 4
    lib.tsx_strerror.restype = ctypes.c_char_p
    assert lib.tsx_strerror(-5) == b"Tag mismatch"
    assert b"Invalid decompressed size" in lib.tsx_strerror(-7)


def test_library_contains_gfx950_code_only(product_lib, tmp_path):
    # llvm-objdump --offloading also EXTRACTS every bundle entry next to the path it was given: hand it a link in a scratch directory
    # so that nothing lands in the package directory (hygiene)
    link = tmp_path / os.path.basename(product_lib)
    os.symlink(os.path.abspath(product_lib), link)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(link)], capture_output=True, text=True, cwd=tmp_path).stdout
    pkg = os.path.dirname(os.path.abspath(product_lib))
    assert not [f for f in os.listdir(pkg) if ".hipv4-" in f or ".host-x86_64-" in f], "offload-bundle pieces in the package directory"
    archs = set(re.findall(r"gfx[0-9a-f]+", out))
    assert archs == {"gfx950"}, archs


def test_struct_layouts():
    assert ctypes.sizeof(nat.ChunkDesc) == 48 and nat.ChunkDesc.iv.offset == 36
    assert ctypes.sizeof(nat.BatchParams) == 4 + 4 + 32 + 64 + 4 + 4


def test_transformed_bound(product_lib):
    lib = ctypes.CDLL(product_lib)
    lib.tsx_transformed_bound.restype = ctypes.c_size_t
    lib.tsx_transformed_bound.argtypes = [ctypes.c_size_t, ctypes.c_uint32]
    assert lib.tsx_transformed_bound(4194304, nat.ENCRYPT) == 4194332
    assert lib.tsx_transformed_bound(4194304, nat.COMPRESS) == 4194304 + 16384  # ZSTD_compressBound
    assert lib.tsx_transformed_bound(15, nat.COMPRESS) == 15 + 63


def test_no_gpu_means_loud_failure_not_fallback(product_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    n = nat.Native(product_lib)
    with pytest.raises(nat.TsxError) as e:
        n.init()
    assert e.value.code == nat.E_DEVICE
    with pytest.raises(nat.TsxError):
        n.ctx_create()


def test_product_never_touches_the_oracle_or_the_emulator():
    """No import/link/dlopen of the oracle, libzstd, OpenSSL or the emulator anywhere in the product package."""
    needles = ("liboracle", "from oracle", "import oracle", "dlopen", "ZSTD_compress2", "ZSTD_createCCtx", "ZSTD_decompress(",
               "EVP_", "libcrypto", "-lzstd", "-lcrypto", "CDLL(EMU", "emu_native")
    bad = []
    for dp, _, files in os.walk(PKG):
        if "_obj" in dp:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".java", ".c")) or f == "Makefile":
                text = open(os.path.join(dp, f), errors="ignore").read()
                bad += [(f, n) for n in needles if n in text]
    # the C++ host layer loads libtsxform itself by the path its caller names (so the same host code can be pointed at the
    # emulated build by the tests); that is its only dlopen and it names no library of its own
    host = open(os.path.join(PKG, "host", "tsxhost.cpp")).read()
    assert host.count("dlopen(") == 1 and "dlopen(libPath.c_str()" in host
    assert not re.search(r"libzstd|libcrypto|liboracle|_emu", host)
    bad = [b for b in bad if b != ("tsxhost.cpp", "dlopen")]
    assert not bad, bad
    linked = subprocess.run(["ldd", nat.LIB_PATH], capture_output=True, text=True).stdout
    assert "zstd" not in linked and "crypto" not in linked and "oracle" not in linked


def test_no_kernel_on_the_fetch_path_uses_scratch(product_lib):
    """A queue's first dispatch that needs scratch makes the runtime (re)size that queue's scratch, and while the compressor service's
    long-lived kernel holds its own the request waits for that kernel to END: the first fetch after uploads began took 18.6 s on the device
    (every later one 4 ms).  So only two kernels of the library may have a private segment at all - the compressor itself and the batch
    build of the chunk-serial decoder, which is never launched while the service is alive (tsx_batch.hip launch_stages).  Read from the
    compiler's resource report of the build that produced libtsxform.so (csrc/Makefile)."""
    obj = os.path.join(PKG, "csrc", "_obj")
    reports = [f for f in os.listdir(obj) if f.endswith(".usage.txt")] if os.path.isdir(obj) else []
    if len(reports) < 6:
        pytest.skip("no resource reports next to the library (not built by csrc/Makefile in this tree)")
    usage = {}
    for f in reports:
        name = None
        for line in open(os.path.join(obj, f), errors="ignore"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name:
                usage[name] = int(m.group(1))
    kernels = {k: v for k, v in usage.items() if "kernel" in k}
    assert len(kernels) >= 18, sorted(kernels)
    with_scratch = sorted(k for k, v in kernels.items() if v)
    assert all(("zstd_service_kernel" in k) or ("22zstd_decompress_kernel" in k) for k in with_scratch), with_scratch
    for must in ("zstd_decompress_fallback_kernel", "zb_index_kernel", "zb_decode_kernel", "gcm_ctr_ghash_kernel", "crc32c_partial_kernel"):
        assert any(must in k and v == 0 for k, v in kernels.items()), must


def test_java_binding_agrees_with_the_header_and_the_shim():
    """The Java side cannot be compiled in this image (no JDK): what can be checked is that TsxNative.java's constants are the
    C header's, and that every `native` method has its JNI entry point in java/jni/tsx_jni.c with the same number of arguments
    (and the other way round)."""
    jdir = os.path.join(ROOT, "java", "io", "aiven", "kafka", "tieredstorage", "gpu")
    src = open(os.path.join(jdir, "TsxNative.java")).read()
    consts = {k: int(v, 0) for k, v in re.findall(r"public static final int (\w+) = (-?(?:0x)?[0-9A-Fa-f]+);", src)}
    assert consts["DESC_BYTES"] == ctypes.sizeof(nat.ChunkDesc)
    for jname, field in [("DESC_SRC_OFF", "src_off"), ("DESC_DST_OFF", "dst_off"), ("DESC_SRC_LEN", "src_len"), ("DESC_DST_CAP", "dst_cap"),
                         ("DESC_DST_LEN", "dst_len"), ("DESC_CRC32C", "crc32c"), ("DESC_STATUS", "status"), ("DESC_IV", "iv")]:
        assert consts[jname] == getattr(nat.ChunkDesc, field).offset, jname
    assert (consts["COMPRESS"], consts["ENCRYPT"], consts["CRC"]) == (nat.COMPRESS, nat.ENCRYPT, nat.CRC)
    assert (consts["OK"], consts["E_TAG_MISMATCH"], consts["E_BAD_FRAME"], consts["E_BAD_SIZE"]) == (0, nat.E_TAG_MISMATCH, nat.E_BAD_FRAME, nat.E_BAD_SIZE)
    assert (consts["ZSTD_PROFILE_1_5_6"], consts["ZSTD_PROFILE_1_5_7"]) == (nat.ZSTD_PROFILE_1_5_6, nat.ZSTD_PROFILE_1_5_7)
    h = open(os.path.join(ROOT, "include", "tsxform.h")).read()
    for cname, jname in [("TSX_E_TAG_MISMATCH", "E_TAG_MISMATCH"), ("TSX_E_BAD_FRAME", "E_BAD_FRAME"), ("TSX_E_BAD_SIZE", "E_BAD_SIZE")]:
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % cname, h) or re.search(r"%s\s*=\s*(-?\d+)" % cname, h)
        assert m and int(m.group(1)) == consts[jname], cname
    # native methods <-> JNI entry points (JNIEnv*, jclass + the Java parameters)
    natives = {}
    for m in re.finditer(r"native\s+\w+(?:\[\])?\s+(\w+)\s*\(([^)]*)\)", src, flags=re.S):
        params = [p for p in m.group(2).split(",") if p.strip()]
        natives[m.group(1)] = len(params)
    shim = open(os.path.join(ROOT, "java", "jni", "tsx_jni.c")).read()
    entries = {}
    for m in re.finditer(r"Java_io_aiven_kafka_tieredstorage_gpu_TsxNative_(\w+)\s*\(([^)]*)\)", shim, flags=re.S):
        entries[m.group(1)] = len([p for p in m.group(2).split(",") if p.strip()]) - 2
    assert natives == entries, (natives, entries)
    # every class that calls into TsxNative uses methods that exist
    for f in os.listdir(jdir):
        for ref in re.findall(r"TsxNative\.(\w+)", open(os.path.join(jdir, f)).read()):
            assert ref in natives or ref in consts or ref == "Buffers", (f, ref)


def test_gpu_chunk_cache_meets_the_references_cache_selection_contract():
    """`fetch.chunk.cache.class` selects a cache by reflection (reference ChunkManagerFactory.java:39-46):
    cacheClass.getDeclaredConstructor(ChunkManager.class).newInstance(defaultChunkManager) assigned to a ChunkCache<?>, then
    configure(prefix-stripped map).  No JDK here, so the source is checked for exactly that shape: subclass of ChunkCache, the
    one-argument constructor, configure(Map) reading the reference's keys through ChunkCacheConfig, ChunkCache's four abstract hooks,
    and - ADVICE r2 - no ForkJoinPool (its workers time out and would leave pinned buffers registered with the device runtime)."""
    jdir = os.path.join(ROOT, "java", "io", "aiven", "kafka", "tieredstorage", "gpu")
    src = open(os.path.join(jdir, "GpuChunkCache.java")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    assert re.search(r"public class GpuChunkCache extends ChunkCache<byte\[\]>", code)
    assert re.search(r"public GpuChunkCache\(final ChunkManager \w+\)\s*\{\s*super\(\w+\);", code)
    assert re.search(r"public void configure\(final Map<String, \?> configs\)", code) and "new ChunkCacheConfig(configs)" in code
    for accessor in ("cachePrefetchingSize()", "cacheSize()", "getTimeout()", "threadPoolSize()"):
        assert accessor in code, accessor
    assert '"gpu.coalesce.wait.us"' in code
    for hook in ("cachedChunkToInputStream", "cacheChunk", "removalListener", "weigher"):
        assert re.search(r"@Override\s+public [\w<>\[\], ]+ %s\(" % hook, code), hook
    assert "ForkJoinPool" not in code and "newFixedThreadPool" in code and "TsxNative.Buffers.release()" in code
    # the reference's abstract class really has these hooks and this constructor shape (if the reference tree is at hand)
    ref = "/root/reference/core/src/main/java/io/aiven/kafka/tieredstorage/fetch/cache/ChunkCache.java"
    if os.path.exists(ref):
        r = open(ref).read()
        for hook in ("cachedChunkToInputStream", "cacheChunk", "removalListener", "weigher"):
            assert re.search(r"public abstract [\w<>\[\], ]+ %s\(" % hook, r), hook
        assert "protected ChunkCache(final ChunkManager chunkManager)" in r
    # the upload side gives its device hint back
    t = open(os.path.join(jdir, "GpuTransformChunkEnumeration.java")).read()
    assert "TsxNative.setThreadDevice(-1)" in t


def test_stale_abi_is_refused(tmp_path):
    """ABI 3 put src_size in the middle of the batch entry points; a library of another ABI must be refused at load, not
    called with shifted arguments."""
    c = tmp_path / "stale.c"
    c.write_text("unsigned tsx_abi_version(void) { return 2; }\n")
    so = tmp_path / "libtsxform_stale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(c)])
    with pytest.raises(RuntimeError, match="ABI 2"):
        nat.Native(str(so))
    shim = open(os.path.join(ROOT, "java", "jni", "tsx_jni.c")).read()
    assert "tsx_abi_version() != TSX_ABI_VERSION" in shim              # the JNI shim's init() refuses a mismatched pair as well
