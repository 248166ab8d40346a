"""Manual quality measurement (not collected by pytest) of the gradient push; prints what profiles/temporal_gradients_quality.txt
records. cbox 128x128, the reconnection shift, 16 frames of a 1 degree orbit at 8 spp in passes of 4, every frame its own sample
window. The relative RMSE of the last frame against a 4096-spp Path render of that camera, for the frame's own reconstruction, the
accumulated primal, and the reconstruction (l2 and wl2) of the accumulated triple with the Jacobian and with j_max = 1, where every
pixel whose gradient would be stretched restarts (a stand-in for "no Jacobian").
    python tests/quality_temporal_gradients.py"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gdpt_amd as G
from helpers import scene_variant

W = H = 128
FRAMES, SPP, PASS, DEG, REF_SPP = 16, 8, 4, 1.0, 4096
CENTRE = (278.0, 274.4, 279.6)

with tempfile.TemporaryDirectory() as tmp:
    sd = G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=W, height=H, tag="quality"))
    sc = G.Scene(sd)
    handles = {"jacobian": (G.Temporal(W, H), {}), "j_max=1": (G.Temporal(W, H), dict(j_max=1.0))}
    last = {}
    for f in range(FRAMES):
        cam = G.orbit_camera(sd.desc.camera, CENTRE, DEG * f)
        sc.set_camera(cam)
        ses = G.Progressive(sc, FRAMES * SPP, shift=G.SHIFT_RECONNECT, path=False, slice=(f * SPP, SPP))
        for _ in range(SPP // PASS):
            ses.add_pass(PASS)
        means, vars_, asm = ses.read()
        own, _ = ses.reconstruct()
        ses.close()
        feat, _ = sc.features(SPP, window=(FRAMES * SPP, f * SPP))
        c, cx, cy = G.Temporal.assemble(means)
        for name, (t, kw) in handles.items():
            last[name] = t.push_gradients(cam, c, asm["c"], feat, cx, asm["cx"], cy, asm["cy"], **kw)
    ref, _ = sc.path_render(spp=REF_SPP)
    rel = lambda a: float(np.sqrt(np.mean((a - ref) ** 2) / np.mean(ref ** 2)))      # noqa: E731
    print(f"cbox {W}x{H}, reconnection shift, {FRAMES} frames of a {DEG} degree orbit at {SPP} spp; relative RMSE of the last frame against {REF_SPP} spp")
    print(f"  the frame's own reconstruction (l2)          {rel(own):.4f}")
    print(f"  the frame's own primal                       {rel(means['img']):.4f}")
    print(f"  the accumulated primal                       {rel(last['jacobian']['out']):.4f}")
    for name, r in last.items():
        st = r["stats"]
        l2, _ = G.reconstruct(W, H, r["out"], r["gx_out"], r["gy_out"], norm=G.RECON_L2)
        wl2, _ = G.reconstruct_weighted(W, H, r["out"], r["gx_out"], r["gy_out"], r["var_out"], r["gx_var_out"], r["gy_var_out"], norm=G.RECON_L2)
        print(f"  accumulated triple, {name:9s} l2 {rel(l2):.4f}  wl2 {rel(wl2):.4f}   (mean history {st.base.sum_history / (W * H):.2f}, mean gradient history "
              f"{st.sum_gradient_history / (W * H):.2f}, {st.pixels_gradient_reset} gradients reset, {st.base.pixels_reset} reset)")
    for t, _ in handles.values():
        t.close()
    sc.close()
