"""Manual timing (not collected by pytest) of progressive rendering; prints what profiles/progressive_times.txt records.
HIP events (the library's own render_ms / fold_ms), medians of 11 after a warm-up of every shape.
  * the fold launch (csrc/hip/progressive.hip: fold_kernel + finish_kernel, a GradPath pass that is not the first) at 512x512,
    1024x1024 and 1280x720: time, and its algorithmic bytes (15 components x 3 doubles read + 2 written per pixel) over that
    time as a share of the 8 TB/s HBM peak;
  * cbox 512x512: a session of 16 passes of 16 spp against the one-shot 256-spp render, same process, alternating: device time of
    the renders (render_ms summed over the passes) and of the folds, and the host wall time of both.
    python tests/time_progressive.py [--quick]"""
import os, sys, time
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

for w, h in ((512, 512), (1024, 1024), (1280, 720)):
    sc = G.Scene(G.parse_scene(XML, film=(w, h)))
    ses = G.Progressive(sc, REPS + 3)
    for _ in range(3):                                   # warm-up: code objects, the first-pass variant, the planes
        ses.add_pass(1)
    t = []
    for _ in range(REPS):
        ses.add_pass(1)
        t.append(ses.status()["fold_ms"])
    ms = float(np.median(t))
    nbytes = w * h * 15 * 5 * 8
    print(f"fold {w}x{h}: {ms * 1e3:.1f} us (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}), {nbytes / 1e6:.1f} MB -> {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = "
          f"{100 * nbytes / (ms * 1e-3) / HBM_PEAK:.0f} % of the HBM peak", flush=True)
    ses.close(); sc.close()

w = h = 512
sc = G.Scene(G.parse_scene(XML, film=(w, h)))
bufs = [torch.zeros((h, w, 3), dtype=torch.float64, device=dev) for _ in range(5)]
ptrs = [b.data_ptr() for b in bufs]


def one_shot():
    t0 = time.perf_counter()
    st = sc.render_device(ptrs, 256, G.RNG_SAMPLE, want_stats=True)
    return st.render_ms, (time.perf_counter() - t0) * 1e3


def session():
    t0 = time.perf_counter()
    ses = G.Progressive(sc, 256)
    fold = 0.0
    for _ in range(16):
        ses.add_pass(16)
        fold += ses.status()["fold_ms"]
    st = ses.status()
    wall = (time.perf_counter() - t0) * 1e3
    ses.close()
    return st["totals"].render_ms, fold, wall


one_shot(); session()                                    # warm-up of both shapes
a, b = [], []
for _ in range(REPS):
    a.append(one_shot()); b.append(session())
med = lambda rows, i: float(np.median([r[i] for r in rows]))
o_ms, o_wall = med(a, 0), med(a, 1)
s_ms, s_fold, s_wall = med(b, 0), med(b, 1), med(b, 2)
print(f"cbox 512x512, 256 spp: one-shot render {o_ms:.3f} ms (host wall {o_wall:.3f} ms); session of 16 passes of 16 spp: renders {s_ms:.3f} ms + folds "
      f"{s_fold:.3f} ms = {s_ms + s_fold:.3f} ms device time (host wall {s_wall:.3f} ms, planes allocated and freed inside)", flush=True)
print(f"price of progressiveness: device time x{(s_ms + s_fold) / o_ms:.3f} ({100 * ((s_ms + s_fold) / o_ms - 1):+.1f} %), of which the folds are "
      f"{100 * s_fold / o_ms:.1f} % of the one-shot render", flush=True)
