"""The C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with PickerKind::Bounded behind a metric predicate on the decode profile and
best-score on prefill: tests/cpp/test_bounded_scheduler.cpp (links libeppk AND liboracle: test infrastructure)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bounded_scheduler.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_bounded_scheduler")
PKG = os.path.join(ROOT, "gateway-api-inference-extension_amd")


def _build():
    import __graft_entry__ as g
    g.build()
    deps = [SRC, os.path.join(PKG, "host", "eppk_host.hpp"), os.path.join(ROOT, "include", "eppk.h"), os.path.join(ROOT, "oracle", "oracle.h")]
    if not g._newer(EXE, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", SRC, "-o", EXE, f"-L{PKG}", "-leppk", f"-L{os.path.join(ROOT, 'oracle')}", "-loracle",
                        f"-Wl,-rpath,{PKG}", f"-Wl,-rpath,{os.path.join(ROOT, 'oracle')}"], check=True)
        g._stamp(EXE, deps)
    return EXE


def test_bounded_scheduler_test_compiles():
    _build()


@pytest.mark.gpu
def test_bounded_decode_profile_equals_direct_calls_and_overflow_is_unavailable():
    # a chunk of 64 rows: the scheduler's groups of 128 requests go through the count / scan / assign launches, the last group through one
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=300, env=dict(os.environ, EPPK_BOUND_CHUNK="64"))
    assert out.returncode == 0, out.stderr + out.stdout
    assert "bounded scheduler ok" in out.stdout
