"""csrc/hip/device_mem.h on the CPU: tests/device_mem_check.cpp (a stand-alone program over a malloc / free space that can refuse an
allocation) built with the host compiler under AddressSanitizer + UBSan, and run. Needs no GPU; nothing is loaded into Python."""
import os
import subprocess

from helpers import ROOT


def test_buffer_and_registry_invariants_under_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "device_mem_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "device_mem_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_mem_check ok" in r.stdout
