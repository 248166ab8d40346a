"""CPU evaluation of the calibration ratio that test_gpu_progressive.py::test_the_variance_means_what_it_says asserts on the GPU:

    R = sum (mean_img - ref)^2 / sum var_mean(img)

for cbox 64x64, reference shift, 32 passes of 4 spp drawn as the session draws them (stream (y*W+x)*128 + 4k + s through
OracleScene.grad_sample, accumulated as oracle_render does), folded by tests/progressive_ref.py; ref = OracleScene.render at
4096 spp. Its own error adds 128/4096 to the expectation 1. Manual script (about a minute): python tests/progressive_oracle_ratio.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import gdpt_amd as G
import oracle_py as O
import progressive_ref as R
from helpers import scene_variant

W = H = 64
PASSES, PASS_SPP, REF_SPP = 32, 4, 4096
BUDGET = PASSES * PASS_SPP


def oracle_pass_img(osc, first, spp, budget):
    """img plane of the window [first, first + spp) of a block of `budget` streams (oracle/oracle.cpp: oracle_render's accumulation)."""
    img = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            r = np.zeros(3)
            for s in range(spp):
                rec, _ = osc.grad_sample(x, y, *O.pcg_init((y * W + x) * budget + first + s))
                if rec.prob > 0.0:
                    r = r + np.array(rec.radiance) / float(spp)
            img[y, x] = r
    return img


def main():
    with tempfile.TemporaryDirectory() as tmp:
        sd = G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=W, height=H))
        osc = O.OracleScene(sd.ptr)
        f = R.Fold()
        for k in range(PASSES):
            f.add({"img": oracle_pass_img(osc, k * PASS_SPP, PASS_SPP, BUDGET)}, PASS_SPP)
            if k + 1 in (8, 32):
                print(f"passes {k + 1}: sum var_mean(img) = {f.var_mean()['img'].sum():.6e}, error estimate {f.error_estimate()[0]:.5f}", flush=True)
        ref, _ = osc.render(REF_SPP, G.RNG_SAMPLE, threads=os.cpu_count() or 4)
        ratio = ((f.mean["img"] - ref["img"]) ** 2).sum() / f.var_mean()["img"].sum()
        print(f"R = {ratio:.4f} (expected near {1 + BUDGET / REF_SPP:.3f})")


if __name__ == "__main__":
    main()
