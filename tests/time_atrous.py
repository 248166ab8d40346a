"""Manual timing (not collected by pytest) of the edge-avoiding a-trous wavelet filter; prints what profiles/atrous_times.txt
records. One process; HIP events (the library's own filter_ms). At 512x512 on the synthetic noisy film and feature planes of
tests/time_nlm_guided.py, every form alternating, five runs each after one warm-up run each:
  - every step 1 .. 32 as a call of one level (first_level = log2 step) under the default guide (albedo, normal), in the direct form
    (knob nlm_direct = 1) and, where it exists (steps 1 - 8), the staged form (knob 2);
  - the whole default call (5 levels, k 2.0), guided by albedo and normal, and demodulated with the normal guide, under the knob
    values 0 (the product routes), 1 (direct at every step) and 2 (staged at every step up to 8);
  - the tiled guided non-local-means filter at its defaults, the yardstick.
The product route of a step is the staged form only if its worst run beats the direct form's best run at that step. Every timed call
runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_atrous.py [--quick]"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G

quick = "--quick" in sys.argv
RUNS = 2 if quick else 5
STEP_LIMIT_S = 60


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)

w, h = 512, 512
gen = torch.Generator(device=dev).manual_seed(1)
y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64, device=dev)
img = (base + 0.05 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous()
var = (0.0025 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous()
c = torch.arange(8, dtype=torch.float64, device=dev)[:, None, None]
feat = (0.5 + 0.05 * torch.sin(0.09 * x[None] + 0.4 * c) * torch.cos(0.06 * y[None] - 0.2 * c)
        + 0.03 * torch.randn(8, h, w, dtype=torch.float64, device=dev, generator=gen)).contiguous()
fvar = (0.0009 * (0.25 + 0.75 * torch.rand(8, h, w, dtype=torch.float64, device=dev, generator=gen))).contiguous()
feat[7] = 1.0                             # the coverage plane of the demodulated call
fvar[7] = 0.0
out, vout = torch.empty_like(img), torch.empty_like(img)
torch.cuda.synchronize()
ptrs = (img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr())
both, normal = G.nlm_guide(), G.nlm_guide(groups=[(3, 3, 1e-3)])


def atrous(knob, **kw):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=knob):
        ms = G.denoise_atrous_device(w, h, *ptrs, 8, out.data_ptr(), vout.data_ptr(), **kw).filter_ms
    signal.alarm(0)
    return ms


def guided_nlm(knob):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=knob):
        ms = G.denoise_nlm_guided_device(w, h, *ptrs, out.data_ptr(), vout.data_ptr(), guide=both).filter_ms
    signal.alarm(0)
    return ms


KNOBS = {0: "product routes", 1: "direct", 2: "staged"}
FORMS = []
for lv in range(6):
    for knob in ((2, 1) if (1 << lv) <= 8 else (1,)):
        FORMS.append((f"step {1 << lv:2d}, one level, guided: {KNOBS[knob]}", lambda knob=knob, lv=lv: atrous(knob, guide=both, levels=1, first_level=lv)))
for knob in (0, 1, 2):
    FORMS.append((f"default call (5 levels), guided albedo + normal: {KNOBS[knob]}", lambda knob=knob: atrous(knob, guide=both)))
for knob in (0, 1, 2):
    FORMS.append((f"default call (5 levels), demodulated, guide normal: {KNOBS[knob]}", lambda knob=knob: atrous(knob, guide=normal, demod=G.nlm_demod())))
FORMS.append(("guided nlm (10, 3), tiled", lambda: guided_nlm(0)))

ms = {name: [] for name, _ in FORMS}
sums = {}
for run in range(1 + RUNS):
    for name, call in FORMS:
        t = call()
        if run >= 1:
            ms[name].append(t)
        sums[name] = float(out.sum())
for name, _ in FORMS:
    v = ms[name]
    print(f"{w}x{h}: {name:62s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f}); sum out {sums[name]:.12e}", flush=True)
for lv in range(4):
    st, di = ms[f"step {1 << lv:2d}, one level, guided: staged"], ms[f"step {1 << lv:2d}, one level, guided: direct"]
    print(f"step {1 << lv}: staged worst {max(st):.3f} against direct best {min(di):.3f}: the product route is the {'staged' if max(st) < min(di) else 'direct'} form",
          flush=True)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
for kind in ("guided albedo + normal", "demodulated, guide normal"):
    a = med(ms[f"default call (5 levels), {kind}: product routes"])
    print(f"default call, {kind}: {a:.3f} ms against the guided nlm filter's {med(ms['guided nlm (10, 3), tiled']):.3f} ms (medians): "
          f"x{a / med(ms['guided nlm (10, 3), tiled']):.3f}", flush=True)
