"""Manual timing (not collected by pytest) of the first-order regression on the non-local-means weights; prints what
profiles/nlm_regress_times.txt records. One process; HIP events (the library's own filter_ms; for the enqueue-only form, which
returns no stats, events recorded on the same stream around the call). At 512x512, (r, f) = (10, 3), the default guide and the
seven regressors albedo, normal and depth, four forms alternate, five runs each after one warm-up run each: regress tiled, regress
direct (knob nlm_direct), guided tiled, and regress tiled with neither var_out nor the sums asked for (no second sweep), on the
synthetic noisy film and feature planes of tests/time_nlm_guided.py. Every timed call runs under an alarm of its own: a call that
overruns it ends the process, and nothing more is started.
    python tests/time_nlm_regress.py [--quick] [--lib PATH]"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
if "--lib" in sys.argv:          # another build of the library, so that one script times two builds
    G.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])

quick = "--quick" in sys.argv
RUNS = 2 if quick else 5
STEP_LIMIT_S = 120


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)

w, h, r, f = 512, 512, 10, 3
gen = torch.Generator(device=dev).manual_seed(1)
y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64, device=dev)
img = (base + 0.05 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous()
var = (0.0025 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous()
c = torch.arange(8, dtype=torch.float64, device=dev)[:, None, None]
feat = (0.5 + 0.05 * torch.sin(0.09 * x[None] + 0.4 * c) * torch.cos(0.06 * y[None] - 0.2 * c)
        + 0.03 * torch.randn(8, h, w, dtype=torch.float64, device=dev, generator=gen)).contiguous()
fvar = (0.0009 * (0.25 + 0.75 * torch.rand(8, h, w, dtype=torch.float64, device=dev, generator=gen))).contiguous()
out, vout = torch.empty_like(img), torch.empty_like(img)
torch.cuda.synchronize()
guide, regress = G.nlm_guide(), G.nlm_regress(channels=range(7))
ptrs = (img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr())
kw = dict(guide=guide, window_radius=r, patch_radius=f)


def one(kind, form):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=form):
        if kind == "regress":
            ms = G.denoise_nlm_regress_device(w, h, *ptrs, out.data_ptr(), vout.data_ptr(), regress=regress, **kw).filter_ms
        elif kind == "guided":
            ms = G.denoise_nlm_guided_device(w, h, *ptrs, out.data_ptr(), vout.data_ptr(), **kw).filter_ms
        else:                             # the regression's first sweep and solve alone: enqueue-only, on the stream torch's events are on
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            G.denoise_nlm_regress_device(w, h, *ptrs, out.data_ptr(), None, regress=regress, stats=False, **kw)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
    signal.alarm(0)
    return ms


FORMS = (("regress tiled", "regress", 0), ("regress direct", "regress", 1), ("guided tiled", "guided", 0), ("regress tiled, out only", "out", 0))
ms = {name: [] for name, _, _ in FORMS}
sums = {}
for run in range(1 + RUNS):
    for name, kind, form in FORMS:
        t = one(kind, form)
        if run >= 1:
            ms[name].append(t)
        sums[name] = (float(out.sum()), float(vout.sum()))
for name, _, _ in FORMS:
    v = ms[name]
    print(f"{w}x{h} (r, f) = ({r}, {f}): {name:24s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f}); "
          f"sum out {sums[name][0]:.12e}", flush=True)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
print(f"regress tiled worst / regress direct best = {max(ms['regress tiled']):.3f} / {min(ms['regress direct']):.3f}; "
      f"regress / guided, tiled (medians) = x{med(ms['regress tiled']) / med(ms['guided tiled']):.2f}; "
      f"out only / both sweeps (medians) = x{med(ms['regress tiled, out only']) / med(ms['regress tiled']):.2f}", flush=True)
