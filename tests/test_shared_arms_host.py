"""The shared arms of the lane machine's step, on the CPU: tests/shared_arms_check.cpp (a stand-alone program) checks (1) that an offset
lane's bounce-1 numbers drawn from the jumped state (csrc/pcg_jump.h) equal those drawn behind the stream's seeding and two steps — the same
three doubles and the same end state for the extremes of the stream index, the largest base + s of a 2^15-square film at 4096 spp and
400 000 random streams —, (2) that the one division of the step's sums gives the bits of the three it replaces: num / (prob * spp) at
num = 1.0 against 1.0 / (prob * spp), and r * (1.0 / spp) formed once against operator/'s own, for prob over the denormals and
1e-300 .. 1e300 and spp = 1 .. 4096, and (3) that contrib - (+0) is contrib bit for bit and offset k adds to component {1, 3, 2, 4}[k].
Built with the host compiler under AddressSanitizer + UBSan, and run. Needs no GPU; nothing is loaded into Python."""
import os
import subprocess

from helpers import ROOT


def test_jumped_draws_and_shared_quotients(tmp_path):
    exe = tmp_path / "shared_arms_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "shared_arms_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shared_arms_check ok" in r.stdout
