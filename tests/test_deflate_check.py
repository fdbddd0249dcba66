"""tools/deflate_check.cpp: the host build of gsky_amd/csrc/deflate_core.h as
a stand-alone program under the address and undefined-behaviour sanitizers --
the encoder tests' corpus as zlib and raw streams at levels 0 and 6, inflated
by zlib, with exact-size buffers, and the code-length limiter seen to run on
the Fibonacci-weighted block.  Built with the host compiler, the sanitizer
runtime linked statically where the compiler can, and run as its own process
in the environment the test itself has.  Nothing of it is loaded into Python.
It is a check of host code for a machine without a GPU: where a device is
visible, or the environment preloads a library (a sanitizer's runtime has to
come first in the link order), it does not run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _builds(cxx, flags, tmp_path):
    """True if a one-line program compiles, links and runs with `flags`."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp_path / "probe")
    if subprocess.run([cxx, "-std=c++17"] + flags + [str(src), "-o", exe], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


def test_deflate_core_under_sanitizers(tmp_path):
    if os.path.exists("/dev/kfd") or os.environ.get("LD_PRELOAD"):
        pytest.skip("a sanitizer run of host code: for a machine without a GPU and without preloaded libraries")
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # the toolchain is probed with a one-line program; the real build below must then succeed
    flags = None
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        if _builds(cxx, SANITIZE + static, tmp_path):
            flags = SANITIZE + static
            break
    if flags is None:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = str(tmp_path / "deflate_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags +
                           ["-I", os.path.join(ROOT, "gsky_amd", "csrc"),
                            os.path.join(ROOT, "tools", "deflate_check.cpp"), "-lz", "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "deflate_check ok" in run.stdout
    assert "code-length limiter ran" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
