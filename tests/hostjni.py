"""What the host and JNI test modules share (tests/test_*_host_jni.py, tests/test_jni_shim.py): building and running a JNI harness
(tests/jni/) or a host program (tests/host/) against a libtsxform build, and reading the Java sources and the C header as text."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBUILD = os.path.join(ROOT, "oracle", "_build")
HOST_DIR = os.path.join(ROOT, "tests", "host")
JAVA_DIR = os.path.join(ROOT, "java", "io", "aiven", "kafka", "tieredstorage", "gpu")
SHIM = os.path.join(ROOT, "java", "jni", "tsx_jni.c")


def emu_target():
    """The CPU-emulated library, built if need be: (directory, link name, path, environment)."""
    from tests.emu import emu_native
    lib = emu_native.build()
    return os.path.dirname(lib), "tsxform_emu", lib, {"TSX_ALLOW_ANY_ARCH": "1"}


def product_target():
    import tsxform
    return os.path.join(ROOT, "tiered-storage-for-apache-kafka_amd"), "tsxform", tsxform._native.LIB_PATH, {}


def _run(args, env_extra, ok):
    r = subprocess.run(args, env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and ok in r.stdout, r.stdout + r.stderr
    return r.stdout


def run_jni(harness, target, tmp_path, ok, oracle=True, libs=()):
    """tests/jni/<harness>.c compiled with the shim, linked against the target (and the oracle), run: its stdout, which holds `ok`."""
    libdir, libname, _, env_extra = target
    os.makedirs(tmp_path, exist_ok=True)
    exe = os.path.join(tmp_path, harness + "_" + libname)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "jni"), "-I" + os.path.join(ROOT, "include"),
                           SHIM, os.path.join(ROOT, "tests", "jni", harness + ".c"),
                           "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir]
                          + (["-L" + OBUILD, "-loracle", "-Wl,-rpath," + OBUILD] if oracle else []) + list(libs) + ["-o", exe])
    return _run([exe], env_extra, ok)


def run_host(program, target, ok):
    """tests/host/<program>.cpp linked against the host layer's one object file and the oracle (tests/host/Makefile), run on the target."""
    from oracle import oracle
    oracle.build()
    subprocess.check_call(["make", "-s", "-C", HOST_DIR, "_build/" + program])
    return _run([os.path.join(HOST_DIR, "_build", program), target[2]], target[3], ok)


def java_text(name):
    return open(os.path.join(JAVA_DIR, name + ".java")).read()


def java_code(name):
    """The class's source without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", java_text(name), flags=re.S))


def header_define(name):
    """The value of `#define name` in include/tsxform.h: an integer, hexadecimal with a `u` or decimal with a sign."""
    h = open(os.path.join(ROOT, "include", "tsxform.h")).read()
    return int(re.search(r"#define\s+" + name + r"\s+(0x[0-9A-Fa-f]+(?=u)|-?\d+\b)", h).group(1), 0)


def java_constant(name):
    return int(re.search(r"public static final int " + name + r" = (0x[0-9A-Fa-f]+|-?\d+);", java_text("TsxNative")).group(1), 0)
