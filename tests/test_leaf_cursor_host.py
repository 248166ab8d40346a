"""csrc/leaf_cursor.h on the CPU: tests/leaf_cursor_check.cpp (a stand-alone program) walks every leaf reference with first < 2^20,
count 1..4 and K in {1, 2} through leaf_advance, built with the host compiler under AddressSanitizer + UBSan, and run. A cursor that
does not advance would be an endless loop in a persistent kernel. Needs no GPU; nothing is loaded into Python."""
import os
import subprocess

from helpers import ROOT


def test_leaf_cursor_visits_every_record_once_and_ends(tmp_path):
    exe = tmp_path / "leaf_cursor_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "leaf_cursor_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "leaf_cursor_check ok" in r.stdout
