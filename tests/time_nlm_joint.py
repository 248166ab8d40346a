"""Manual timing (not collected by pytest) of the joint non-local-means filter against the guided one; prints what
profiles/nlm_joint_times.txt records. One process; HIP events (the library's own filter_ms). At 512x512, (r, f) = (10, 3) and the
default guide (albedo and normal groups over 8 planes), tiled form, these calls alternate, five runs each after one warm-up run each:
gdpt_denoise_nlm_guided_device, gdpt_denoise_nlm_joint_device with n = 1, 2 and 4 companions, and the same pair unguided (n = 2), on
the synthetic noisy film of tests/time_nlm_guided.py; the companions are noisy films of their own. Every timed call runs under an alarm
of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_nlm_joint.py [--quick] [--lib PATH]"""
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
STEP_LIMIT_S = 60


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
comp = [(0.1 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous() for _ in range(4)]
cvar = [(0.01 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous() for _ in range(4)]
out, vout = torch.empty_like(img), torch.empty_like(img)
cout, cvout = [torch.empty_like(img) for _ in range(4)], [torch.empty_like(img) for _ in range(4)]
torch.cuda.synchronize()
guide, none = G.nlm_guide(), G.nlm_guide(groups=[])
ptrs = lambda ts, n: [t.data_ptr() for t in ts[:n]]      # noqa: E731


def one(guided, n):
    signal.alarm(STEP_LIMIT_S)
    kw = dict(window_radius=r, patch_radius=f)
    with G.debug_knobs(nlm_direct=0):
        if n == 0 and guided:
            st = G.denoise_nlm_guided_device(w, h, img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr(), out.data_ptr(), vout.data_ptr(),
                                             guide=guide, **kw)
        elif n == 0:
            st = G.denoise_nlm_device(w, h, img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(), **kw)
        else:
            st = G.denoise_nlm_joint_device(w, h, img.data_ptr(), var.data_ptr(), ptrs(comp, n), ptrs(cvar, n), out.data_ptr(), ptrs(cout, n),
                                            var_out_ptr=vout.data_ptr(), comp_var_out_ptrs=ptrs(cvout, n), feat_ptr=feat.data_ptr() if guided else None,
                                            feat_var_ptr=fvar.data_ptr() if guided else None, guide=guide if guided else none, **kw).guide
    signal.alarm(0)
    return st.filter_ms


FORMS = (("guided", 1, 0), ("joint guided n=1", 1, 1), ("joint guided n=2", 1, 2), ("joint guided n=4", 1, 4), ("unguided", 0, 0), ("joint unguided n=2", 0, 2))
ms = {name: [] for name, _, _ in FORMS}
for run in range(1 + RUNS):
    for name, guided, n in FORMS:
        t = one(guided, n)
        if run >= 1:
            ms[name].append(t)
med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
for name, _, _ in FORMS:
    v = ms[name]
    print(f"{w}x{h} (r, f) = ({r}, {f}) tiled: {name:19s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f}, median {med[name]:.3f})", flush=True)
print("joint / guided (medians): " + ", ".join(f"n={n} x{med[f'joint guided n={n}'] / med['guided']:.2f}" for n in (1, 2, 4))
      + f"; joint / unguided n=2 x{med['joint unguided n=2'] / med['unguided']:.2f}", flush=True)
