"""csrc/abi_guard.h keeps exceptions inside the library: every extern "C" entry that can allocate on the host runs its body
through abi_guard.  A stand-alone program (host compiler, no HIP, its own main) checks the three outcomes."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <new>
#include <stdexcept>
#include "abi_guard.h"
int main()
{
    if (abi_guard([]() -> int { throw std::bad_alloc(); }) != PWR_ERR_NOMEM) return 1;
    if (abi_guard([]() -> int { throw std::runtime_error("other"); }) != PWR_ERR_INTERNAL) return 2;
    if (abi_guard([] { return 7; }) != 7) return 3;
    return 0;
}
"""


def test_abi_guard_turns_exceptions_into_codes(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "guard.cpp", tmp_path / "guard"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "repeatresolver_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
