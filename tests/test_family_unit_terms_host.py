"""The static term lists of the family parents (csrc/constraints.cpp, family_term_lists) without a device:
tests/host/family_unit_terms_check.cpp, a stand-alone program, is compiled with the system C++ compiler together with
constraints.cpp and symbolic.cpp and run once.  It checks that every (family, constraint) list is the mapping of the entry
lists with its dense terms first and its unit terms behind them, flagged and normalised, and that the lists do not depend on
the number of host threads; its header says how."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smcp_amd", "csrc")


def test_family_unit_terms_on_the_host(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler (c++, g++, clang++) on PATH")
    exe = str(tmp_path / "family_unit_terms_check")
    srcs = [os.path.join(ROOT, "tests", "host", "family_unit_terms_check.cpp"), os.path.join(CSRC, "constraints.cpp"),
            os.path.join(CSRC, "symbolic.cpp")]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-pthread", "-o", exe] + srcs, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
