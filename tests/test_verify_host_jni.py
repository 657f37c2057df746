"""Verify on upload through the host layers: the JNI shim (tests/jni/jni_verify_harness.c: TsxNative.VERIFY in the flags it passes on)
and the C++ host layer's option (tests/host/host_verify.cpp: zstdVerify, the twin of the Java classes'), over the CPU-emulated library
here and the product library on a GPU box (-m gpu).  No JDK here: the Java classes are checked as source."""
import re

import pytest

from tests import hostjni


def test_jni_flag_against_the_emulated_library(tmp_path):
    out = hostjni.run_jni("jni_verify_harness", hostjni.emu_target(), tmp_path, "jni verify ok", oracle=False, libs=("-ldl",))
    assert "verify on, source damaged: status 0 -10 0" in out and "verify off, source damaged: status 0 0 0" in out
    assert "verify on, source intact: status 0 0 0" in out


def test_host_option_against_the_emulated_library(tmp_path):
    out = hostjni.run_host("host_verify", hostjni.emu_target(), "host verify: 0 failed")
    assert "verify on:" in out and "verify off:" in out
    assert "damaged source, verify on: the frame written for this chunk does not restore it" in out and "damaged source, verify off: no error" in out


def test_java_classes_carry_the_option():
    """The constants equal the header's and the Python binding's; both upload-side classes have an overload that ends in the option,
    refuse it without compression and put the flag into the batch; the older constructors pass false; the fetch side has no such option."""
    import tsxform
    assert hostjni.header_define("TSX_VERIFY") == hostjni.java_constant("VERIFY") == tsxform._native.VERIFY == 0x20
    assert hostjni.header_define("TSX_E_VERIFY") == hostjni.java_constant("E_VERIFY") == tsxform._native.E_VERIFY == -10
    assert hostjni.header_define("TSX_ABI_VERSION") == 4
    for f in ("GpuTransformChunkEnumeration", "GpuTransformFinisher"):
        code = hostjni.java_code(f)
        assert re.search(r"final boolean zstdChecksum,\s*final boolean zstdVerify\)", code), f
        assert re.search(r"if \(zstdVerify && !compress\) \{\s*throw new IllegalArgumentException\(", code), f
        assert re.search(r"\(zstdVerify \? TsxNative\.VERIFY : 0\)", code), f
        assert re.search(r"zstdLevel, zstdChecksum, false\);", code), f      # the older constructors: off
    for f in ("GpuDetransformChunkEnumeration", "GpuChunkManager", "GpuChunkCache"):
        assert "VERIFY" not in hostjni.java_text(f), f


@pytest.mark.gpu
def test_jni_and_host_verify_against_the_product_library(gpu, tmp_path):
    hostjni.run_jni("jni_verify_harness", hostjni.product_target(), tmp_path, "jni verify ok", oracle=False, libs=("-ldl",))
    hostjni.run_host("host_verify", hostjni.product_target(), "host verify: 0 failed")
