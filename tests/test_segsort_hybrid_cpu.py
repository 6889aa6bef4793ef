"""The hybrid schedule of the binning's large sort class (gs_seg_hybrid of gs_segsort_dev.h), stepped on the host.

tests/segsort_hybrid_host.cpp includes the header with GS_SEGSORT_FN = inline and runs the schedule with tid = 0, nthreads = 1 for
n in {1, 15, 17, 2 049, 4 095, 4 096, 4 097, 5 000, 8 191, 8 192, 8 193, 12 288, 12 289, 16 384, 16 385, 20 000, 40 000}, with random
keys, keys from 16 values and all-equal keys, both padding words (24-bit and 32-bit keys), chunks of 8 192 (the kernel's), 4 096 and 64 words.
It compares every emitted word with std::sort, checks that every index is emitted exactly once and that the words behind n of a longer
backing array are unchanged.  The program is built with AddressSanitizer and UBSan where the host toolchain links them (a read or
write outside the chunk buffer or the backing array then ends it), and without them otherwise."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "geosplatting_amd", "csrc")


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I", CSRC, *extra, os.path.join(HERE, "segsort_hybrid_host.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_hybrid_schedule_sorts_like_std_sort(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "segsort_hybrid_host")
    built = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if built.returncode != 0:
        built = _compile(cxx, exe, [])
    assert built.returncode == 0, built.stdout + built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().startswith("ok "), run.stdout
    assert int(run.stdout.split()[1]) == 17 * 3 * 5
