"""Verify on upload, AES-GCM stage, through the host layers: the JNI shim (tests/jni/jni_gcm_verify_harness.c: TsxNative.VERIFY_GCM in the
flags it passes on) and the C++ host layer's option (tests/host/host_gcm_verify.cpp: gcmVerify, the twin of the Java classes'), over the
CPU-emulated library here and the product library on a GPU box (-m gpu).  No JDK here: the Java classes are checked as source."""
import re

import pytest

from tests import hostjni


def _check_jni_output(out):
    for chain in ("encrypt", "compress + encrypt"):
        assert chain + ", gcm verify on, output damaged: status 0 -10 0" in out and chain + ", gcm verify off, output damaged: status 0 0 0" in out
        assert chain + ", gcm verify on, output intact: status 0 0 0" in out and chain + ", gcm verify off, output intact: status 0 0 0" in out


def _check_host_output(out):
    for chain in ("encrypt", "compress + encrypt"):
        assert chain + ", gcm verify on:" in out and chain + ", gcm verify off:" in out
        assert chain + ", damaged output, gcm verify on: the frame written for this chunk does not restore it" in out
        assert chain + ", damaged output, gcm verify off: no error" in out


def test_jni_flag_against_the_emulated_library(tmp_path):
    _check_jni_output(hostjni.run_jni("jni_gcm_verify_harness", hostjni.emu_target(), tmp_path, "jni gcm verify ok", oracle=False, libs=("-ldl",)))


def test_host_option_against_the_emulated_library(tmp_path):
    _check_host_output(hostjni.run_host("host_gcm_verify", hostjni.emu_target(), "host gcm verify: 0 failed"))


def test_java_classes_carry_the_option():
    """The constant equals the header's and the Python binding's; both upload-side classes have an overload that ends in the option,
    refuse it without encryption and put the flag into the batch; the overloads that were there delegate with false; the fetch side has
    no such option."""
    import tsxform
    assert hostjni.header_define("TSX_VERIFY_GCM") == hostjni.java_constant("VERIFY_GCM") == tsxform._native.VERIFY_GCM == 0x80
    assert hostjni.header_define("TSX_ABI_VERSION") == 4
    for f in ("GpuTransformChunkEnumeration", "GpuTransformFinisher"):
        code = hostjni.java_code(f)
        assert re.search(r"final boolean zstdVerify,\s*final boolean gcmVerify\)", code), f
        assert re.search(r"final boolean zstdChecksum,\s*final boolean zstdVerify\)", code), f      # the overload that was there stays
        assert re.search(r"if \(gcmVerify && keyAndAad == null\) \{\s*throw new IllegalArgumentException\(", code), f
        assert re.search(r"\(gcmVerify \? TsxNative\.VERIFY_GCM : 0\)", code), f
        assert re.search(r"zstdLevel,\s*zstdChecksum,\s*zstdVerify,\s*false\);", code), f       # ... and delegates: off
    for f in ("GpuDetransformChunkEnumeration", "GpuChunkManager", "GpuChunkCache"):
        src = hostjni.java_text(f)
        assert "VERIFY" not in src and "gcmVerify" not in src, f
    shim = open(hostjni.SHIM).read()
    assert "p->flags = (uint32_t)flags;" in shim and "VERIFY" not in shim   # the flags word passes through untouched


@pytest.mark.gpu
def test_jni_and_host_gcm_verify_against_the_product_library(gpu, tmp_path):
    _check_jni_output(hostjni.run_jni("jni_gcm_verify_harness", hostjni.product_target(), tmp_path, "jni gcm verify ok", oracle=False, libs=("-ldl",)))
    _check_host_output(hostjni.run_host("host_gcm_verify", hostjni.product_target(), "host gcm verify: 0 failed"))
