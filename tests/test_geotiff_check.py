"""tools/geotiff_check.cpp: the host side of the WCS GeoTIFF writer
(gsky_amd/csrc/tiffwrite.cpp -- band rules, TIFF predictors, PackBits, BigTIFF
framing -- on the host build of deflate_core.h) as a stand-alone program under
the address and undefined-behaviour sanitizers: the shapes of
tests/test_geotiff_deflate.py written into an output buffer of exactly
gskyhip_geotiff_bound_opts from bands of exactly their size, every tile
inflated by zlib and un-predicted back to the input.  Built with the host
compiler, the sanitizer runtime linked statically where the compiler can, and
run as its own process in the environment the test itself has.  Nothing of it
is loaded into Python.  It is a check of host code for a machine without a
GPU: where a device is visible, or the environment preloads a library (a
sanitizer's runtime has to come first in the link order), it does not run."""
import os
import subprocess

import pytest

from .test_deflate_check import ROOT, SANITIZE, _builds, _compiler


def test_geotiff_writer_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "geotiff_check")
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags +
                           ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gsky_amd", "csrc"),
                            os.path.join(ROOT, "tools", "geotiff_check.cpp"),
                            os.path.join(ROOT, "gsky_amd", "csrc", "tiffwrite.cpp"), "-lz", "-pthread", "-o", exe],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "geotiff_check ok" in run.stdout
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
