"""The owning buffer and the one growth rule (csrc/eppk_mem.hpp) under a counting fake policy, compiled alone with the address and
undefined-behaviour sanitizers: tests/cpp/test_mem.cpp.  Host code only: no HIP header, no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_mem.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_mem")
HDRS = [os.path.join(ROOT, "gateway-api-inference-extension_amd", "csrc", "eppk_mem.hpp"), os.path.join(ROOT, "include", "eppk.h")]
# (the sanitizers' runtimes linked INTO the program: a dynamically linked ASan runtime has to come first in the process's library list)
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra"]


def _build():
    import __graft_entry__ as g
    if not g._newer(EXE, [SRC] + HDRS, " ".join(FLAGS)):
        subprocess.run(["g++", *FLAGS, SRC, "-o", EXE], check=True)
        g._stamp(EXE, [SRC] + HDRS, " ".join(FLAGS))
    return EXE


def test_header_compiles_alone_with_a_host_compiler():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-include", HDRS[0], "-x", "c++", os.devnull],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_buffer_and_growth_rule_under_the_sanitizers():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "mem ok" in out.stdout
