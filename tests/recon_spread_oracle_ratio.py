"""CPU evaluation of the calibration ratio that test_gpu_recon_spread.py::test_the_estimate_means_what_it_says asserts on the GPU:

    R = sum (f_tot - f_ref)^2 / sum var

for cbox 32x32, reference shift, a group of 8 members over a block of 64 streams, one pass of 8 per member: member i draws streams
(y*W+x)*64 + 8i + s, s < 8, through OracleScene.grad_sample, accumulated as oracle_render does; f_i = fourier_solve(assemble(member
i)), f_tot = fourier_solve(assemble(the mean of the members' buffers)), var = tests/recon_spread_ref.py on the f_i with weights 8;
f_ref = fourier_solve(assemble(OracleScene.render at 4096 spp)). Its own error adds 64/4096 to the expectation 1.
Manual script (a few minutes): python tests/recon_spread_oracle_ratio.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import gdpt_amd as G
import oracle_py as O
import recon_spread_ref as S
from helpers import scene_variant

W = H = 32
MEMBERS, PASS_SPP, REF_SPP = 8, 8, 4096
BUDGET = MEMBERS * PASS_SPP
BUFS = ("img", "cx0", "cy0", "cx1", "cy1")


def oracle_window(osc, first, spp, budget):
    """The five buffers of the window [first, first + spp) of a block of `budget` streams (oracle/oracle.cpp: oracle_render's
    accumulation; the loop of test_window_is_the_stated_stream_layout_gradpath)."""
    out = {k: np.zeros((H, W, 3)) for k in BUFS}
    for y in range(H):
        for x in range(W):
            acc = {k: np.zeros(3) for k in BUFS}
            for s in range(spp):
                rec, _ = osc.grad_sample(x, y, *O.pcg_init((y * W + x) * budget + first + s))
                if rec.prob > 0.0:
                    c = np.array(rec.contrib)
                    acc["img"] = acc["img"] + np.array(rec.radiance) / float(spp)
                    acc["cx0"] = acc["cx0"] + (c - np.array(rec.contribX0)) * (rec.wX0 / (rec.prob * float(spp)))
                    acc["cy0"] = acc["cy0"] + (c - np.array(rec.contribY0)) * (rec.wY0 / (rec.prob * float(spp)))
                    acc["cx1"] = acc["cx1"] + (np.array(rec.contribX1) - c) * (rec.wX1 / (rec.prob * float(spp)))
                    acc["cy1"] = acc["cy1"] + (np.array(rec.contribY1) - c) * (rec.wY1 / (rec.prob * float(spp)))
            for k in BUFS:
                out[k][y, x] = acc[k]
    return out


def recon(bufs):
    return O.fourier_solve(*O.assemble(bufs), 0.04)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        sd = G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=W, height=H))
        osc = O.OracleScene(sd.ptr)
        members = []
        for i in range(MEMBERS):
            members.append(oracle_window(osc, i * PASS_SPP, PASS_SPP, BUDGET))
            print(f"member {i} drawn", flush=True)
        total = {k: sum(m[k] for m in members) / float(MEMBERS) for k in BUFS}
        f = [recon(m) for m in members]
        f_tot = recon(total)
        e = S.estimate(f, [float(PASS_SPP)] * MEMBERS, f_tot)
        fbar = e["mean"]
        print(f"linearity: |fbar - f_tot| / |f_tot| = {np.linalg.norm(fbar - f_tot) / np.linalg.norm(f_tot):.2e}")
        ref, _ = osc.render(REF_SPP, G.RNG_SAMPLE, threads=os.cpu_count() or 4)
        f_ref = recon(ref)
        ratio = ((f_tot - f_ref) ** 2).sum() / e["sum_var"]
        primal = ((total["img"] - ref["img"]) ** 2).sum() / (f_ref ** 2).sum()
        print(f"sum var = {e['sum_var']:.6e}, error estimate {e['error']:.6f}, left out {e['left_out']}")
        print(f"relative MSE against the {REF_SPP}-spp reference: reconstruction {((f_tot - f_ref) ** 2).sum() / (f_ref ** 2).sum():.6e}, primal {primal:.6e}")
        print(f"R = {ratio:.8f} (expected near {1 + BUDGET / REF_SPP:.4f})")


if __name__ == "__main__":
    main()
