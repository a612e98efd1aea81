"""The address maps of pconvt.hip's LDS-DMA ring (ds-gan_amd/csrc/pconvt_maps.h), checked on the host:
tests/pconvt_maps_check.cpp replays whole launches of the test shapes and the step's shapes over the
header the kernel uses and asserts that every LDS-DMA source lies inside its tensor, that every LDS
byte a fragment read touches is written exactly once per stage with the right value, and that the
stages fit the LDS.  A wrong source address would be a GPU fault; this runs without a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ds-gan_amd", "csrc")


def test_pconvt_ring_maps(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pconvt_maps_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(HERE, "pconvt_maps_check.cpp"), "-o", exe]
    # the stand-alone program under AddressSanitizer + UBSan where the host toolchain has their runtimes
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().startswith("OK:")
