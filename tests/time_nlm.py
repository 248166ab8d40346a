"""Manual timing (not collected by pytest) of the two forms of the non-local-means filter; prints what profiles/nlm_times.txt
records. One process; HIP events (the library's own filter_ms: the filter kernel and the two one-block reductions); the tiled form
and the direct form (knob nlm_direct) alternate, five runs each after one warm-up run each, on a synthetic noisy film:
512x512 at (r, f) = (10, 3) and (5, 1), 1280x720 at (10, 3). Every timed call runs under an alarm of its own: a call that
overruns it ends the process, and nothing more is started.
    python tests/time_nlm.py [--quick] [--lib PATH]"""
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
STEP_LIMIT_S = 60          # a direct run at 1280x720 (10, 3) is expected well under ten seconds


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)


def one(form, w, h, r, f, ptrs):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=form):
        st = G.denoise_nlm_device(w, h, *ptrs, window_radius=r, patch_radius=f)
    signal.alarm(0)
    return st.filter_ms


for (w, h, r, f) in ((512, 512, 10, 3), (512, 512, 5, 1), (1280, 720, 10, 3)):
    gen = torch.Generator(device=dev).manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    base = (0.5 + 0.25 * torch.sin(0.05 * x + 0.03 * y))[:, :, None] * torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64, device=dev)
    img = (base + 0.05 * torch.randn(h, w, 3, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    var = (0.0025 * (0.5 + torch.rand(h, w, 3, dtype=torch.float64, device=dev, generator=gen))).contiguous()
    out, vout = torch.empty_like(img), torch.empty_like(img)
    torch.cuda.synchronize()
    ptrs = (img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr())
    ms = {0: [], 1: []}
    for run in range(1 + RUNS):
        for form in (0, 1):
            t = one(form, w, h, r, f, ptrs)
            if run >= 1:
                ms[form].append(t)
    fmt = lambda v: ", ".join(f"{t:.3f}" for t in v)      # noqa: E731
    print(f"{w}x{h} (r, f) = ({r}, {f}): tiled  {fmt(ms[0])} ms (best {min(ms[0]):.3f}, worst {max(ms[0]):.3f})", flush=True)
    print(f"{w}x{h} (r, f) = ({r}, {f}): direct {fmt(ms[1])} ms (best {min(ms[1]):.3f}, worst {max(ms[1]):.3f}); "
          f"direct best / tiled worst = x{min(ms[1]) / max(ms[0]):.1f}", flush=True)
