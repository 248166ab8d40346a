"""csrc/lds_layout.h on the CPU: tests/lds_layout_check.cpp (a stand-alone program) sweeps the dynamic-LDS layout of the one-sided lane
machine on an LDS-resident scene — regions disjoint, aligned as setup_trace reads them, never larger than the fixed layout and equal
to it at the caps — and, for the headline scene (cbox, prepared on the host), checks that two fitted render blocks and one block of
the small-footprint solve shape fit a CU's 160 KB of LDS, allocation granule counted. Built with the host compiler under
AddressSanitizer + UBSan, and run. Needs no GPU; nothing sanitised is loaded into Python."""
import os
import subprocess

from helpers import ROOT, SCENES

# LDS of the 32 x 32 x 16 shape of dct_fold_gemm_f64 (poisson_kernels.hip: gemm_lds_bytes(16, 32)): one A tile of 32 x 17 and one B tile
# of 16 x 34 doubles, and the four doubles of red[]
SMALL_SOLVE_BLOCK = (32 * 17 + 16 * 34) * 8 + 4 * 8


def test_layout_sweep_and_headline_fit(G, tmp_path):
    exe = tmp_path / "lds_layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "lds_layout_check.cpp")])
    info = G.debug_knobs.prepare_scene(G.parse_scene(os.path.join(SCENES, "cbox/cbox_gdpt.xml")))
    n = info["count"]
    args = [n["nodes4"], n["prims"], n["tris"], n["materials"], n["light_intensity"] // 3, info["wide_stack_need"], SMALL_SOLVE_BLOCK]
    r = subprocess.run([str(exe)] + [str(int(a)) for a in args], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lds_layout_check ok" in r.stdout
