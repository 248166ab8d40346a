"""csrc/item_slice.h on the CPU: tests/item_slice_check.cpp (a stand-alone program) compares the carried decomposition of a work item
(item_slice_at: one decomposition per slice, lanes follow by carry) with the division form (item_divide) for tiles_x in {1, 2, 3, 7, 32},
tile rows in {1, 2, 5}, chunks in {1, 2, 6, 64}, every slice start and every length 1..64. Built with the host compiler under
AddressSanitizer + UBSan, and run. Needs no GPU; nothing is loaded into Python."""
import os
import subprocess

from helpers import ROOT


def test_carried_item_decomposition_equals_division_form(tmp_path):
    exe = tmp_path / "item_slice_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "item_slice_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "item_slice_check ok" in r.stdout
