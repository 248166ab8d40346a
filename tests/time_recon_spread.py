"""Manual timing (not collected by pytest) of the spread of N images; prints what profiles/recon_spread_times.txt records. HIP events
(the library's own spread_ms and fold_ms), medians of 11 after a warm-up, at 512x512, 1024x1024, 1280x720:
  * the spread launch (spread_kernel + finish_kernel, var and the raw map written) for N = 2 and N = 8 on synthetic images, in TB/s
    of its byte count, (N + 1) x 24 read + 32 written per pixel;
  * the same with the window of radius 2 and 8 (box_kernel added: 8 read + 8 written per pixel more);
  * the fold launch (fold_kernel + finish_kernel, a GradPath pass that is not the first: 5 doubles per component, 15 components)
    measured in the same run, as tests/time_progressive_merge.py takes it.
    python tests/time_recon_spread.py [--quick]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G

quick = "--quick" in sys.argv
REPS = 3 if quick else 11
HBM_PEAK = 8.0e12
XML = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
med = lambda v: float(np.median(v))

for w, h in ((512, 512), (1024, 1024), (1280, 720)):
    sc = G.Scene(G.parse_scene(XML, film=(w, h)))
    ses = G.Progressive(sc, REPS + 3)
    for _ in range(3):                                   # warm-up: code objects, the first-pass variant, the planes
        ses.add_pass(1)
    fold = []
    for _ in range(REPS):
        ses.add_pass(1)
        fold.append(ses.status()["fold_ms"])
    ses.close()
    sc.close()
    f_ms = med(fold)
    f_tbs = w * h * 15 * 5 * 8 / (f_ms * 1e-3) / 1e12
    print(f"{w}x{h}: fold {f_ms * 1e3:.1f} us (min {min(fold) * 1e3:.1f}, max {max(fold) * 1e3:.1f}; {f_tbs:.2f} TB/s = {100 * f_tbs * 1e12 / HBM_PEAK:.0f} % of the HBM peak)", flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (2, 8):
        imgs = [1.0 + 0.1 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen) for _ in range(n)]
        total = torch.ones(h, w, 3, dtype=torch.float64, device=dev)
        var = torch.empty(h, w, 3, dtype=torch.float64, device=dev)
        emap = torch.empty(h, w, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for radius in (0, 2, 8):
            ms = []
            for r in range(2 + REPS):
                st = G.recon_spread_device(w, h, [x.data_ptr() for x in imgs], [float(k + 1) for k in range(n)], total_ptr=total.data_ptr(),
                                           radius=radius, var_ptr=var.data_ptr(), map_ptr=emap.data_ptr())
                if r >= 2:
                    ms.append(st.spread_ms)
            m = med(ms)
            nbytes = w * h * ((n + 1) * 24 + 32 + (16 if radius else 0))
            tbs = nbytes / (m * 1e-3) / 1e12
            print(f"{w}x{h}: spread N = {n}, radius {radius}: {m * 1e3:.1f} us (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}; {tbs:.2f} TB/s = "
                  f"{100 * tbs * 1e12 / HBM_PEAK:.0f} % of the HBM peak) = x{tbs / f_tbs:.2f} the fold's rate", flush=True)
