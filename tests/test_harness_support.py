"""The shared pieces of the host and JNI harnesses (tests/jni/jni_fake.h, tests/host/host_check.hpp, tests/harness_util.h) stand in front
of every check of those programs: a CHECK that stopped failing, or an input text that changed, would go unnoticed there.  Two throw-away
programs show that a false CHECK still fails its program, and that the text generator still writes the bytes the harnesses were written
over.  No GPU, and no library of the project is loaded."""
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, d) for d in ("tests/jni", "tests/host", "tests", "include", "tiered-storage-for-apache-kafka_amd/host")]
# SHA-256 of the 4096 bytes the generator spelled out in tests/host/host_checksum.cpp wrote for seed 4242, before it moved to harness_util.h
LOG_TEXT_4096_SEED_4242 = "67d854aeb307c995b9adad08b8b4b3aa8599b9ea04f77ac34120f764d3d2b17c"

PROGRAM_A = """
#include "jni_fake.h"
#include "harness_util.h"
int main(void) {
    JNI_ENV(env); (void)env;
    static uint8_t text[4096];
    harness_log_text(text, sizeof text, 4242);
    fwrite(text, 1, sizeof text, stdout);
    CHECK(1 == 1);
    CHECK(1 == 2);
    printf("reached\\n");
    return 0;
}
"""

PROGRAM_B = """
#include "host_check.hpp"
int main() {
    CHECK(2 > 1);
    CHECK(1 > 2);
    CHECK(3 < 2);
    return host_done("host support");
}
"""


def _compile_and_run(tmp_path, name, compiler, source):
    (tmp_path / name).write_text(source)
    exe = str(tmp_path / "program")
    subprocess.check_call(compiler + ["-Wall", "-Werror"] + INCLUDES + [str(tmp_path / name), "-ldl", "-o", exe])
    return subprocess.run([exe], capture_output=True, timeout=60)


def test_a_false_check_fails_the_program_and_the_text_is_the_parents(tmp_path):
    a = _compile_and_run(tmp_path, "a.c", ["gcc", "-O1"], PROGRAM_A)
    assert a.returncode == 1 and b"FAILED line 10: 1 == 2" in a.stderr and b"1 == 1" not in a.stderr and b"reached" not in a.stdout
    assert len(a.stdout) == 4096 and hashlib.sha256(a.stdout).hexdigest() == LOG_TEXT_4096_SEED_4242
    b = _compile_and_run(tmp_path, "b.cpp", ["g++", "-std=c++17", "-O2", "-Wextra"], PROGRAM_B)
    assert b.returncode == 1 and b"host support: 2 failed" in b.stdout
    assert b"FAIL line 5: 1 > 2" in b.stdout and b"FAIL line 6: 3 < 2" in b.stdout and b"2 > 1" not in b.stdout
