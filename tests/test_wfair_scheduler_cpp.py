"""The C++ scheduling cycle (host/eppk_host.hpp: Scheduler) with a PickerKind::Bounded profile that has flow_weights and a turn_window
(SEMANTICS.md §3h): tests/cpp/test_wfair_scheduler.cpp (links libeppk).  Here: it compiles, and Configure's refusals, which need no
device.  The run on the device is tests/test_gpu_wfair.py::test_the_scheduler_driver_on_the_device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_wfair_scheduler.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_wfair_scheduler")
PKG = os.path.join(ROOT, "gateway-api-inference-extension_amd")


def build_driver():
    import __graft_entry__ as g
    g.build()
    deps = [SRC, os.path.join(PKG, "host", "eppk_host.hpp"), os.path.join(ROOT, "include", "eppk.h")]
    if not g._newer(EXE, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", SRC, "-o", EXE, f"-L{PKG}", "-leppk", f"-Wl,-rpath,{PKG}"], check=True)
        g._stamp(EXE, deps)
    return EXE


def test_configure_refuses_weights_without_flows_a_wrong_size_and_a_zero_weight():
    out = subprocess.run([build_driver()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "wfair scheduler: configure ok" in out.stdout
