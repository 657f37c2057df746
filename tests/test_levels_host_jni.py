"""Zstandard levels through the host layers: the JNI shim's level-taking natives (tests/jni/jni_levels_harness.c) and the C++ host layer's
level option (tests/host/host_levels.cpp), over the CPU-emulated library here and the product library on a GPU box (-m gpu)."""
import pytest

from tests import hostjni


def test_jni_level_natives_against_the_emulated_library(oracle, tmp_path):
    out = hostjni.run_jni("jni_levels_harness", hostjni.emu_target(), tmp_path, "jni levels ok")
    assert "level 1:" in out


def test_host_level_option_against_the_emulated_library(oracle, tmp_path):
    out = hostjni.run_host("host_levels", hostjni.emu_target(), "host levels: 0 failed")
    assert "level 2:" in out


@pytest.mark.gpu
def test_jni_and_host_levels_against_the_product_library(gpu, oracle, tmp_path):
    hostjni.run_jni("jni_levels_harness", hostjni.product_target(), tmp_path, "jni levels ok")
    hostjni.run_host("host_levels", hostjni.product_target(), "host levels: 0 failed")
