"""Manual timing (not collected by pytest) of the collaborative form of the first-order regression; prints what
profiles/nlm_collab_times.txt records. One process; HIP events (the library's own filter_ms; for the enqueue-only form, which returns
no stats, events recorded on the same stream around the call). At 512x512, (r, f) = (10, 3), the default guide and the seven
regressors albedo, normal and depth, the forms alternate, five runs each after one warm-up run each: the regression with its second
sweep, the regression without it, the collaborative form tiled (both passes, then the fit alone and the gather alone under the knob
nlm_collab_pass, on a coefficient film of the caller's) and direct (knob nlm_direct), on the synthetic noisy film and feature planes
of tests/time_nlm_regress.py. Every timed call runs under an alarm of its own: a call that overruns it ends the process, and nothing
more is started.
    python tests/time_nlm_collab.py [--quick] [--lib PATH]"""
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
coef = torch.zeros(24, h, w, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
guide, regress = G.nlm_guide(), G.nlm_regress(channels=range(7))
ptrs = (img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr())
kw = dict(guide=guide, regress=regress, window_radius=r, patch_radius=f)


def one(kind, form, part):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=form, nlm_collab_pass=part):
        if kind == "regress":
            ms = G.denoise_nlm_regress_device(w, h, *ptrs, out.data_ptr(), vout.data_ptr(), **kw).filter_ms
        elif kind == "collab":
            ms = G.denoise_nlm_collab_device(w, h, *ptrs, out.data_ptr(), coef.data_ptr(), **kw).filter_ms
        else:                             # the regression's first sweep and solve alone: enqueue-only, on the stream torch's events are on
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            G.denoise_nlm_regress_device(w, h, *ptrs, out.data_ptr(), None, stats=False, **kw)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
    signal.alarm(0)
    return ms


# (the gather alone follows a run that left the coefficient film in `coef`)
FORMS = (("regress tiled", "regress", 0, 0), ("regress tiled, out only", "out", 0, 0), ("collab tiled", "collab", 0, 0),
         ("collab tiled, fit alone", "collab", 0, 1), ("collab tiled, gather alone", "collab", 0, 2), ("collab direct", "collab", 1, 0))
ms = {name: [] for name, _, _, _ in FORMS}
sums = {}
for run in range(1 + RUNS):
    for name, kind, form, part in FORMS:
        t = one(kind, form, part)
        if run >= 1:
            ms[name].append(t)
        sums[name] = float(out.sum())
for name, _, _, _ in FORMS:
    v = ms[name]
    print(f"{w}x{h} (r, f) = ({r}, {f}): {name:27s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f}); "
          f"sum out {sums[name]:.12e}", flush=True)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
print(f"collab tiled worst / collab direct best = {max(ms['collab tiled']):.3f} / {min(ms['collab direct']):.3f}; "
      f"collab / regress, tiled (medians) = x{med(ms['collab tiled']) / med(ms['regress tiled']):.2f}; "
      f"collab / regress out only (medians) = x{med(ms['collab tiled']) / med(ms['regress tiled, out only']):.2f}; "
      f"gather / fit (medians) = x{med(ms['collab tiled, gather alone']) / med(ms['collab tiled, fit alone']):.2f}", flush=True)
