"""Manual timing (not collected by pytest) of the per-pixel filter selection; prints what profiles/filter_select_times.txt records.
One process; HIP events (the library's own select_ms and filter_ms). At 512x512 on the synthetic noisy film and feature planes of
tests/time_atrous.py, with candidates that are smooth fields plus noise: n in {2, 6} x radius in {0, 4, 8} with every output asked
for, and n = 6 at radius 4 without the optional E planes; beside them the default a-trous call (5 levels, guided by albedo and normal),
the cheapest filter the selection chooses among. Every call alternating, five runs each after one warm-up run each. Every timed call
runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_filter_select.py [--quick]"""
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

w, h, NMAX = 512, 512, 6
gen = torch.Generator(device=dev).manual_seed(1)
f64 = dict(dtype=torch.float64, device=dev)
y, x = torch.meshgrid(torch.arange(h, **f64), torch.arange(w, **f64), indexing="ij")
base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], **f64)
noisy = lambda sigma: (base + sigma * torch.randn(h, w, 3, generator=gen, **f64)).contiguous()      # noqa: E731
variance = lambda: (0.0025 * (0.5 + torch.rand(h, w, 3, generator=gen, **f64))).contiguous()      # noqa: E731
img, var = noisy(0.05), variance()
c = torch.arange(8, **f64)[:, None, None]
feat = (0.5 + 0.05 * torch.sin(0.09 * x[None] + 0.4 * c) * torch.cos(0.06 * y[None] - 0.2 * c)
        + 0.03 * torch.randn(8, h, w, generator=gen, **f64)).contiguous()
fvar = (0.0009 * (0.25 + 0.75 * torch.rand(8, h, w, generator=gen, **f64))).contiguous()
uA, uB, vA, vB = noisy(0.07), noisy(0.07), variance(), variance()
FA, FB, T = ([noisy(0.01 * (j + 1)) for j in range(NMAX)] for _ in range(3))
out, vout = torch.empty_like(img), torch.empty_like(img)
sel = torch.empty(h, w, dtype=torch.int32, device=dev)
mse = torch.empty(h, w, **f64)
E = torch.empty(NMAX, h, w, **f64)
torch.cuda.synchronize()
p = lambda ts: [t.data_ptr() for t in ts]      # noqa: E731


def select(n, s, with_E=True):
    signal.alarm(STEP_LIMIT_S)
    ms = G.filter_select_device(w, h, p(FA[:n]), p(FB[:n]), p(T[:n]), uA.data_ptr(), vA.data_ptr(), uB.data_ptr(), vB.data_ptr(), out.data_ptr(),
                                sel.data_ptr(), mse.data_ptr(), E.data_ptr() if with_E else None, radius=s).select_ms
    signal.alarm(0)
    return ms


def atrous():
    signal.alarm(STEP_LIMIT_S)
    ms = G.denoise_atrous_device(w, h, img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr(), 8, out.data_ptr(), vout.data_ptr(),
                                 guide=G.nlm_guide()).filter_ms
    signal.alarm(0)
    return ms


FORMS = [(f"select, n = {n}, radius {s}, every output", lambda n=n, s=s: select(n, s)) for n in (2, 6) for s in (0, 4, 8)]
FORMS.append(("select, n = 6, radius 4, without the E planes", lambda: select(6, 4, False)))
FORMS.append(("default a-trous call (5 levels), guided albedo + normal", atrous))

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
    print(f"{w}x{h}: {name:58s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f}); sum out {sums[name]:.12e}", flush=True)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
a = med(ms["default a-trous call (5 levels), guided albedo + normal"])
for n in (2, 6):
    for s in (0, 4, 8):
        b = med(ms[f"select, n = {n}, radius {s}, every output"])
        print(f"select n = {n}, radius {s}: {b:.3f} ms against the default a-trous call's {a:.3f} ms (medians): x{b / a:.3f}", flush=True)
