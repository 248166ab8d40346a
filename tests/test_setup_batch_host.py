"""The batched sample set-up of the one-sided lane machine, on the CPU: tests/setup_batch_check.cpp (a stand-alone program) checks
(1) csrc/pcg_jump.h — the state of a PCG32 stream behind its seeding and two draws as one multiply-add, against the stepped generator for
the extremes of the stream index and 400 000 random streams — and (2) the exactness argument of csrc/hip/device_trace.h: on a
power-of-two film floor((x + ox) + r) == x + ox and the remainder == r bit for bit, for r in {0, 1, 2^31, 2^32 - 1} * 2^-32 and random r,
x + ox from -1 to the film size, film sizes 2^4 .. 2^15. Built with the host compiler under AddressSanitizer + UBSan, and run. Needs no
GPU; nothing is loaded into Python."""
import os
import subprocess

from helpers import ROOT


def test_jump_constants_and_exact_pixel_split(tmp_path):
    exe = tmp_path / "setup_batch_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "setup_batch_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "setup_batch_check ok" in r.stdout
