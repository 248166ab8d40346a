"""Manual timing (not collected by pytest) of the guided non-local-means filter and the feature render; prints what
profiles/nlm_guided_times.txt records. One process; HIP events (the library's own filter_ms / render_ms). At 512x512, (r, f) =
(10, 3) and the default guide (albedo and normal groups over 8 planes) four forms alternate, five runs each after one warm-up run
each: guided tiled, guided direct, unguided tiled, unguided direct (knob nlm_direct), on the synthetic noisy film of
tests/time_nlm.py with smooth noisy feature planes. Then the feature render of cbox 512x512x16 and sponza 1280x720x16, one run each
after a warm-up. Every timed call runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_nlm_guided.py [--quick] [--lib PATH]"""
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
out, vout = torch.empty_like(img), torch.empty_like(img)
torch.cuda.synchronize()
guide = G.nlm_guide()


def one(guided, form):
    signal.alarm(STEP_LIMIT_S)
    with G.debug_knobs(nlm_direct=form):
        if guided:
            st = G.denoise_nlm_guided_device(w, h, img.data_ptr(), var.data_ptr(), feat.data_ptr(), fvar.data_ptr(), out.data_ptr(), vout.data_ptr(),
                                             guide=guide, window_radius=r, patch_radius=f)
        else:
            st = G.denoise_nlm_device(w, h, img.data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(), window_radius=r, patch_radius=f)
    signal.alarm(0)
    return st.filter_ms


FORMS = (("guided tiled", 1, 0), ("guided direct", 1, 1), ("unguided tiled", 0, 0), ("unguided direct", 0, 1))
ms = {name: [] for name, _, _ in FORMS}
for run in range(1 + RUNS):
    for name, guided, form in FORMS:
        t = one(guided, form)
        if run >= 1:
            ms[name].append(t)
for name, _, _ in FORMS:
    v = ms[name]
    print(f"{w}x{h} (r, f) = ({r}, {f}): {name:15s} {', '.join(f'{t:.3f}' for t in v)} ms (best {min(v):.3f}, worst {max(v):.3f})", flush=True)
print(f"guided tiled worst / guided direct best = {max(ms['guided tiled']):.3f} / {min(ms['guided direct']):.3f}; "
      f"guided / unguided, tiled (medians) = x{sorted(ms['guided tiled'])[len(ms['guided tiled']) // 2] / sorted(ms['unguided tiled'])[len(ms['unguided tiled']) // 2]:.2f}", flush=True)

for label, xml, film, spp in (("cbox 512x512x16", "cbox/cbox_gdpt.xml", (512, 512), 16), ("sponza 1280x720x16", "sponza/sponza.xml", (1280, 720), 16)):
    path = os.path.join(ROOT, "scenes", xml)
    if not os.path.exists(path):
        print(f"{label}: {path} is not here", flush=True)
        continue
    sc = G.Scene(G.parse_scene(path, film=film))
    n = 8 * film[0] * film[1]
    d_mean, d_var = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    for run in range(2):
        signal.alarm(STEP_LIMIT_S)
        st = sc.features_device(d_mean.data_ptr(), d_var.data_ptr(), spp, want_stats=True)
        signal.alarm(0)
    print(f"feature render {label}: {st.render_ms:.3f} ms, {st.rays} rays ({st.rays / st.render_ms / 1e3:.1f} Mrays/s)", flush=True)
    sc.close()
