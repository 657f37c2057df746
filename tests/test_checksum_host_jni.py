"""The Zstandard content checksum through the host layers: the JNI shim (tests/jni/jni_checksum_harness.c: TsxNative.ZSTD_CHECKSUM in the
flags it passes on) and the C++ host layer's option (tests/host/host_checksum.cpp: zstdChecksum, the twin of the Java classes'), over the
CPU-emulated library here and the product library on a GPU box (-m gpu).  No JDK here: the Java classes are checked as source."""
import re

import pytest

from tests import hostjni


def _need157(oracle):
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")


def test_jni_flag_against_the_emulated_library(oracle, tmp_path):
    _need157(oracle)
    out = hostjni.run_jni("jni_checksum_harness", hostjni.emu_target(), tmp_path, "jni checksum ok", libs=("-ldl",))
    assert "checksum on, level 1:" in out and "checksum off, level 0:" in out


def test_host_option_against_the_emulated_library(oracle, tmp_path):
    _need157(oracle)
    out = hostjni.run_host("host_checksum", hostjni.emu_target(), "host checksum: 0 failed")
    assert "checksum on:" in out and "checksum off:" in out


def test_java_classes_carry_the_option():
    """The constant equals the header's and the Python binding's; both upload-side classes take the option, refuse it without
    compression, and put the flag into the batch; the fetch-side classes have no such option (the frame decides)."""
    import tsxform
    assert hostjni.header_define("TSX_ZSTD_CHECKSUM") == hostjni.java_constant("ZSTD_CHECKSUM") == tsxform._native.ZSTD_CHECKSUM == 8
    assert hostjni.header_define("TSX_ABI_VERSION") == 4
    for f in ("GpuTransformChunkEnumeration", "GpuTransformFinisher"):
        code = hostjni.java_code(f)
        assert re.search(r"final int zstdLevel, final boolean zstdChecksum\)", code), f
        assert re.search(r"if \(zstdChecksum && !compress\) \{\s*throw new IllegalArgumentException\(", code), f
        assert re.search(r"\(zstdChecksum \? TsxNative\.ZSTD_CHECKSUM : 0\)", code), f
        assert re.search(r"readAhead, zstdLevel, false\);", code), f      # the older constructors: off, the reference's bytes
    for f in ("GpuDetransformChunkEnumeration", "GpuChunkManager", "GpuChunkCache"):
        assert "ZSTD_CHECKSUM" not in hostjni.java_text(f), f


@pytest.mark.gpu
def test_jni_and_host_checksum_against_the_product_library(gpu, oracle, tmp_path):
    _need157(oracle)
    hostjni.run_jni("jni_checksum_harness", hostjni.product_target(), tmp_path, "jni checksum ok", libs=("-ldl",))
    hostjni.run_host("host_checksum", hostjni.product_target(), "host checksum: 0 failed")
