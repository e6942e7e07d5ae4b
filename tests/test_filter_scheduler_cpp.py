"""The C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with metric predicates on its profiles (ProfileSpec::predicates, SEMANTICS.md
§2c): tests/cpp/test_filter_scheduler.cpp -- both profiles against direct library calls, a shed request comes back Unavailable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_filter_scheduler.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_filter_scheduler")
PKG = os.path.join(ROOT, "gateway-api-inference-extension_amd")


def _build():
    import __graft_entry__ as g
    g.build()
    deps = [SRC, os.path.join(PKG, "host", "eppk_host.hpp"), os.path.join(ROOT, "include", "eppk.h")]
    if not g._newer(EXE, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", SRC, "-o", EXE, f"-L{PKG}", "-leppk", f"-Wl,-rpath,{PKG}"], check=True)
        g._stamp(EXE, deps)
    return EXE


def test_filter_scheduler_test_compiles():
    _build()


@pytest.mark.gpu
def test_profiles_with_predicates_equal_direct_calls_and_shed_requests_are_unavailable():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "filter scheduler ok" in out.stdout
