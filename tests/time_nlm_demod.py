"""Manual timing (not collected by pytest) of the albedo-demodulated non-local-means filter; prints what profiles/nlm_demod_times.txt
records. One process; HIP events (the library's own filter_ms). At 512x512, (r, f) = (10, 3) and (5, 1), eight forms alternate, five
runs each after one warm-up run each: demodulated and not, tiled and direct (knob nlm_direct), guided (a normal group over the 8
planes) and not, on the synthetic noisy film of tests/time_nlm_guided.py with an albedo of 0.2 .. 0.9 in planes 0-2 and coverage 1 in
plane 7. Every timed call runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
A checksum of every undemodulated form's output is printed, to hold it against another build's.
    python tests/time_nlm_demod.py [--quick] [--lib PATH] [--plain-only]      --plain-only: the undemodulated forms alone (runs on a build before
                                                                 this filter, to time the two builds alternately on one device)"""
import hashlib, os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
if "--lib" in sys.argv:          # another build of the library, so that one script times two builds
    G.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])

quick, plain_only = "--quick" in sys.argv, "--plain-only" in sys.argv
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
chk = ((torch.div(x, 3, rounding_mode="floor") + torch.div(y, 3, rounding_mode="floor")) % 2)
for k in range(3):
    feat[k] = (0.3 + 0.2 * k) * (1.0 + 0.5 * (chk - 0.5)) + 0.01 * torch.randn(h, w, dtype=torch.float64, device=dev, generator=gen)
feat[7] = 1.0
fvar[7] = 0.0
out, vout = torch.empty_like(img), torch.empty_like(img)
torch.cuda.synchronize()
guide = G.nlm_guide(groups=[(3, 3, 1e-3)])


def one(demod, guided, form, r, f):
    signal.alarm(STEP_LIMIT_S)
    ptrs = (img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr())
    with G.debug_knobs(nlm_direct=form):
        if demod:
            st = G.denoise_nlm_demod_device(w, h, *ptrs, 8, out.data_ptr(), vout.data_ptr(), guide=guide if guided else None, window_radius=r, patch_radius=f)
        elif guided:
            st = G.denoise_nlm_guided_device(w, h, *ptrs, out.data_ptr(), vout.data_ptr(), guide=guide, window_radius=r, patch_radius=f)
        else:
            st = G.denoise_nlm_device(w, h, ptrs[0], ptrs[1], out.data_ptr(), vout.data_ptr(), window_radius=r, patch_radius=f)
    signal.alarm(0)
    return st.filter_ms


def checksum():
    torch.cuda.synchronize()
    return hashlib.sha256(out.cpu().numpy().tobytes() + vout.cpu().numpy().tobytes()).hexdigest()[:16]


FORMS = [(f"{'demod' if d else 'plain'} {'guided' if g else 'unguided'} {'direct' if form else 'tiled'}", d, g, form)
         for g in (0, 1) for form in (0, 1) for d in ((0,) if plain_only else (0, 1))]
median = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
for (r, f) in ((10, 3), (5, 1)):
    ms = {name: [] for name, _, _, _ in FORMS}
    sums = {}
    for run in range(1 + RUNS):
        for name, d, g, form in FORMS:
            t = one(d, g, form, r, f)
            if run >= 1:
                ms[name].append(t)
            elif not d:
                sums[name] = checksum()
    for name, d, _, _ in FORMS:
        v = ms[name]
        print(f"{w}x{h} (r, f) = ({r}, {f}): {name:22s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f})"
              + (f" sha256 {sums[name]}" if not d else ""), flush=True)
    if plain_only:
        continue
    for g in ("unguided", "guided"):
        for form in ("tiled", "direct"):
            a, b = ms[f"demod {g} {form}"], ms[f"plain {g} {form}"]
            print(f"    demodulated / undemodulated, {g} {form} (medians): {median(a):.3f} / {median(b):.3f} = x{median(a) / median(b):.3f}", flush=True)
        print(f"    demod {g}: tiled worst / direct best = {max(ms[f'demod {g} tiled']):.3f} / {min(ms[f'demod {g} direct']):.3f}", flush=True)
