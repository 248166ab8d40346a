"""Manual timing (not collected by pytest) of the multi-scale non-local-means filters; prints what profiles/nlm_pyramid_times.txt
records. One process; HIP events (the library's own op_ms, total_ms and filter_ms). At 512x512 and 1280x720: the two operators alone,
for the plain kind and for the demodulated kind with a coverage plane, and the whole plain call at levels 1 - 3 with the filter at
(r, f) = (10, 3), five runs each after one warm-up run each, the forms alternating; the single-scale tiled filter runs in the same
process for scale. total_ms of the whole call spans the waits for every level's stats (the call is timed as a session makes it). The
film is the synthetic noisy film of tests/time_var_smooth.py. Every timed call runs under an alarm of its own: a call that overruns it
ends the process, and nothing more is started.
    python tests/time_nlm_pyramid.py [--quick] [--lib PATH]"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
if "--lib" in sys.argv:          # another build of the library, so that one script times two builds
    G.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])

RUNS = 2 if "--quick" in sys.argv else 5
STEP_LIMIT_S = 60


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)

for (w, h) in ((512, 512), (1280, 720)):
    gen = torch.Generator(device=dev).manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64, device=dev)
    img = (base + 0.05 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    var = (0.0025 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous()
    feat = (0.5 + 0.03 * torch.randn(8, h, w, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    fvar = (0.0009 * (0.25 + 0.75 * torch.rand(8, h, w, dtype=torch.float64, device=dev, generator=gen))).contiguous()
    feat[7] = 1.0
    fvar[7] = 0.0
    hc, wc = (h + 1) // 2, (w + 1) // 2
    out, vout, fil = torch.empty_like(img), torch.empty_like(img), (img + 0.01).contiguous()
    cimg, cvar = torch.empty(hc, wc, 3, dtype=torch.float64, device=dev), torch.empty(hc, wc, 3, dtype=torch.float64, device=dev)
    cfeat, cfvar = torch.empty(8, hc, wc, dtype=torch.float64, device=dev), torch.empty(8, hc, wc, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def timed(call):
        signal.alarm(STEP_LIMIT_S)
        t = call()
        signal.alarm(0)
        return t

    def down(demod):
        planes = dict(feat_ptr=feat.data_ptr(), feat_var_ptr=fvar.data_ptr(), feat_out_ptr=cfeat.data_ptr(), feat_var_out_ptr=cfvar.data_ptr(),
                      num_channels=8, kind="demod") if demod else {}
        return G.nlm_pyramid_down_device(w, h, img.data_ptr(), var.data_ptr(), cimg.data_ptr(), cvar.data_ptr(), **planes).op_ms

    def up(demod):                                         # (after a down of the same kind: cimg holds the coarse level)
        planes = dict(feat_ptr=feat.data_ptr(), feat_var_ptr=fvar.data_ptr(), num_channels=8, kind="demod") if demod else {}
        return G.nlm_pyramid_up_device(w, h, img.data_ptr(), var.data_ptr(), fil.data_ptr(), cimg.data_ptr(), out.data_ptr(), **planes).op_ms

    def multi(levels):
        return G.denoise_nlm_multiscale_device(w, h, img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(), levels=levels,
                                               window_radius=10, patch_radius=3).total_ms

    def nlm():
        return G.denoise_nlm_device(w, h, img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(), window_radius=10, patch_radius=3).filter_ms

    forms = [(f"{name}{', demod' if d else ''}", lambda op=op, d=d: op(d)) for d in (0, 1) for name, op in (("down", down), ("up", up))]
    forms += [(f"multiscale, {levels} level{'s' if levels > 1 else ''}", lambda levels=levels: multi(levels)) for levels in (1, 2, 3)]
    forms += [("nlm tiled (10, 3)", nlm)]
    ms = {name: [] for name, _ in forms}
    for run in range(1 + RUNS):
        for name, call in forms:
            t = timed(call)
            if run >= 1:
                ms[name].append(t)
    scale = sorted(ms["nlm tiled (10, 3)"])[RUNS // 2]
    for name, _ in forms:
        v = ms[name]
        print(f"{w}x{h}: {name:22s} {', '.join(f'{t:.4f}' for t in v)} ms (best {min(v):.4f}, worst {max(v):.4f}; median / the filter's median "
              f"{sorted(v)[RUNS // 2] / scale:.4f})", flush=True)
