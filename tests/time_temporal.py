"""Manual timing (not collected by pytest) of the temporal push; prints what profiles/temporal_times.txt records. One process; HIP
events (the library's own push_ms and filter_ms). At 512x512 on the step scene of tests/temporal_ref.py (two planes and a strip of
background, features computed analytically, random colour and variance), the camera turning 0.5 degrees a push, so that every
push reprojects through a sheared footprint and resets at the step and at the film's edge: after two warm-up pushes, five runs of
the push alternating with the five-level a-trous call guided by albedo and normal (its product routes) on the push's outputs, the
filter a progressive preview runs behind it. Every timed call runs under an alarm of its own: a call that overruns it ends the
process, and nothing more is started.
    python tests/time_temporal.py"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
import temporal_ref as T

RUNS, WARM = 5, 2
STEP_LIMIT_S = 60


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)

w, h = 512, 512
rng = np.random.default_rng(1)
img = torch.tensor(rng.uniform(0.5, 1.5, (h, w, 3)), device=dev)
var = torch.tensor(rng.uniform(0.01, 0.02, (h, w, 3)), device=dev)
out, vout, length = torch.empty_like(img), torch.empty_like(img), torch.empty(h, w, dtype=torch.float64, device=dev)
den, dvar = torch.empty_like(img), torch.empty_like(img)
cams, feats = [], []
for k in range(WARM + RUNS):
    cam = T.camera(w, h, T.look_at((0.011, 0.006 + 0.0113 * k, 0), (0.011 + np.sin(np.radians(0.5 * k)), 0.006 + 0.0113 * k, np.cos(np.radians(0.5 * k)))), T.FOV)
    cams.append(T.gdpt_camera(G, cam))
    feats.append(torch.tensor(T.features(cam, T.step_scene())[0], device=dev))
fvar = torch.zeros(8, h, w, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
t = G.Temporal(w, h)
guide = G.nlm_guide()
push_ms, atrous_ms, stats = [], [], None
for k in range(WARM + RUNS):
    signal.alarm(STEP_LIMIT_S)
    stats = t.push_device(cams[k], img.data_ptr(), var.data_ptr(), feats[k].data_ptr(), out.data_ptr(), vout.data_ptr(), length.data_ptr())
    signal.alarm(STEP_LIMIT_S)
    a = G.denoise_atrous_device(w, h, out.data_ptr(), vout.data_ptr(), feats[k].data_ptr(), fvar.data_ptr(), 8, den.data_ptr(), dvar.data_ptr(), guide=guide)
    signal.alarm(0)
    if k >= WARM:
        push_ms.append(stats.push_ms)
        atrous_ms.append(a.filter_ms)
t.close()
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
print(f"{w}x{h}: temporal push            {', '.join(f'{x:.3f}' for x in push_ms)} ms (best {min(push_ms):.3f}, worst {max(push_ms):.3f}); last push: "
      f"mean history {stats.sum_history / (w * h):.3f}, {stats.pixels_reset} reset, {stats.pixels_background} background; sum out {float(out.sum()):.12e}", flush=True)
print(f"{w}x{h}: a-trous, 5 levels, guided  {', '.join(f'{x:.3f}' for x in atrous_ms)} ms (best {min(atrous_ms):.3f}, worst {max(atrous_ms):.3f})", flush=True)
print(f"push against the a-trous call (medians): {med(push_ms):.3f} ms against {med(atrous_ms):.3f} ms: x{med(push_ms) / med(atrous_ms):.3f}", flush=True)
