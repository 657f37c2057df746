"""The JNI shim (java/jni/tsx_jni.c) compiled for real and driven through a hand-made JNIEnv (tests/jni/): there is no JDK in this
image, so this is the evidence that the C half of the Java binding moves the right pointers - against the CPU-emulated library
here, against the product library on a GPU box (-m gpu)."""
import os

import pytest

from tests import hostjni

BUILD = os.path.join(hostjni.ROOT, "tests", "jni", "_build")


def test_jni_shim_against_the_emulated_library():
    hostjni.run_jni("jni_harness", hostjni.emu_target(), BUILD, "jni shim ok", oracle=False)


@pytest.mark.gpu
def test_jni_shim_against_the_product_library(gpu):
    hostjni.run_jni("jni_harness", hostjni.product_target(), BUILD, "jni shim ok", oracle=False)
