"""Manual timing (not collected by pytest) of the variance smoothing; prints what profiles/var_smooth_times.txt records. One process;
HIP events (the library's own smooth_ms and filter_ms). At 512x512 and 1280x720, radius 1, 2 and 4, with and without a demod block,
five runs each after one warm-up run each, the forms alternating; the tiled non-local-means filter at (r, f) = (10, 3) runs in the
same process for scale, on the variance as given. The film is the synthetic noisy film of tests/time_nlm_demod.py. Every timed call
runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_var_smooth.py [--quick]"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G

RUNS = 2 if "--quick" in sys.argv else 5
STEP_LIMIT_S = 60


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)
block = G.nlm_demod()

for (w, h) in ((512, 512), (1280, 720)):
    gen = torch.Generator(device=dev).manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64, device=dev)
    img = (base + 0.05 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    var = (0.0025 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous()
    feat = (0.5 + 0.03 * torch.randn(8, h, w, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    fvar = (0.0009 * (0.25 + 0.75 * torch.rand(8, h, w, dtype=torch.float64, device=dev, generator=gen))).contiguous()
    chk = ((torch.div(x, 3, rounding_mode="floor") + torch.div(y, 3, rounding_mode="floor")) % 2)
    for k in range(3):
        feat[k] = (0.3 + 0.2 * k) * (1.0 + 0.5 * (chk - 0.5)) + 0.01 * torch.randn(h, w, dtype=torch.float64, device=dev, generator=gen)
    feat[7] = 1.0
    fvar[7] = 0.0
    sm, out, vout = torch.empty_like(img), torch.empty_like(img), torch.empty_like(img)
    torch.cuda.synchronize()

    def smooth(s, demod):
        signal.alarm(STEP_LIMIT_S)
        planes = dict(feat_ptr=feat.data_ptr(), feat_var_ptr=fvar.data_ptr(), num_channels=8, demod=block) if demod else {}
        st = G.variance_smooth_device(w, h, img.data_ptr(), var.data_ptr(), sm.data_ptr(), radius=s, **planes)
        signal.alarm(0)
        return st.smooth_ms

    def nlm():
        signal.alarm(STEP_LIMIT_S)
        st = G.denoise_nlm_device(w, h, img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(), window_radius=10, patch_radius=3)
        signal.alarm(0)
        return st.filter_ms

    forms = [(f"smooth s = {s}{', a~' if d else ''}", lambda s=s, d=d: smooth(s, d)) for s in (1, 2, 4) for d in (0, 1)] + [("nlm tiled (10, 3)", nlm)]
    ms = {name: [] for name, _ in forms}
    for run in range(1 + RUNS):
        for name, call in forms:
            t = call()
            if run >= 1:
                ms[name].append(t)
    scale = sorted(ms["nlm tiled (10, 3)"])[RUNS // 2]
    for name, _ in forms:
        v = ms[name]
        print(f"{w}x{h}: {name:20s} {', '.join(f'{t:.4f}' for t in v)} ms (best {min(v):.4f}, worst {max(v):.4f}; median / the filter's median "
              f"{sorted(v)[RUNS // 2] / scale:.4f})", flush=True)
