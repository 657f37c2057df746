"""TSX_ZSTD_PROFILE_DEVICE through the host layers: the JNI shim's natives (tests/jni/jni_device_profile_harness.c) and the C++ host layer's
enumeration and finishers (tests/host/host_device_profile.cpp), over the CPU-emulated library here and the product library on a GPU box
(-m gpu)."""
import pytest

from tests import hostjni


def test_jni_natives_pass_the_profile_to_the_emulated_library(oracle, tmp_path):
    out = hostjni.run_jni("jni_device_profile_harness", hostjni.emu_target(), tmp_path, "jni device profile ok")
    assert "device profile:" in out


def test_host_enumeration_and_finishers_against_the_emulated_library(oracle, tmp_path):
    out = hostjni.run_host("host_device_profile", hostjni.emu_target(), "host device profile: 0 failed")
    assert "device profile:" in out


@pytest.mark.gpu
def test_jni_and_host_against_the_product_library(gpu, oracle, tmp_path):
    hostjni.run_jni("jni_device_profile_harness", hostjni.product_target(), tmp_path, "jni device profile ok")
    hostjni.run_host("host_device_profile", hostjni.product_target(), "host device profile: 0 failed")
