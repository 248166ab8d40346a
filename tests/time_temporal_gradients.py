"""Manual timing (not collected by pytest) of the gradient push against the plain push; prints what
profiles/temporal_gradients_times.txt records. One process; HIP events (the library's own push_ms). At 512x512 on the step scene of
tests/temporal_ref.py (features computed analytically, random colour, gradients and variances), the camera turning 0.5 degrees a
push as in tests/time_temporal.py: two handles, one pushed with gradients and one plainly, after two warm-up pushes five runs
alternating. Every timed call runs under an alarm of its own: a call that overruns it ends the process, and nothing more is started.
    python tests/time_temporal_gradients.py"""
import os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
import temporal_ref as T

RUNS, WARM = 5, 2
STEP_LIMIT_S = 60


def overrun(signum, frame):
    print("a timed call overran its limit: stopping", flush=True)
    os._exit(124)


signal.signal(signal.SIGALRM, overrun)

w, h = 512, 512
rng = np.random.default_rng(1)
film = lambda lo, hi: torch.tensor(rng.uniform(lo, hi, (h, w, 3)), device=dev)      # noqa: E731
img, var = film(0.5, 1.5), film(0.01, 0.02)
grads = [film(-0.5, 0.5), film(0.01, 0.02), film(-0.5, 0.5), film(0.01, 0.02)]      # gx, gx_var, gy, gy_var
out, vout = torch.empty_like(img), torch.empty_like(img)
gouts = [torch.empty_like(img) for _ in range(4)]
pout, pvout = torch.empty_like(img), torch.empty_like(img)
cams, feats = [], []
for k in range(WARM + RUNS):
    cam = T.camera(w, h, T.look_at((0.011, 0.006 + 0.0113 * k, 0), (0.011 + np.sin(np.radians(0.5 * k)), 0.006 + 0.0113 * k, np.cos(np.radians(0.5 * k)))), T.FOV)
    cams.append(T.gdpt_camera(G, cam))
    feats.append(torch.tensor(T.features(cam, T.step_scene())[0], device=dev))
torch.cuda.synchronize()
tg, tp = G.Temporal(w, h), G.Temporal(w, h)
grad_ms, plain_ms, gs, ps = [], [], None, None
for k in range(WARM + RUNS):
    signal.alarm(STEP_LIMIT_S)
    gs = tg.push_gradients_device(cams[k], img.data_ptr(), var.data_ptr(), feats[k].data_ptr(), [g.data_ptr() for g in grads], out.data_ptr(),
                                  vout.data_ptr(), [g.data_ptr() for g in gouts])
    signal.alarm(STEP_LIMIT_S)
    ps = tp.push_device(cams[k], img.data_ptr(), var.data_ptr(), feats[k].data_ptr(), pout.data_ptr(), pvout.data_ptr())
    signal.alarm(0)
    if k >= WARM:
        grad_ms.append(gs.base.push_ms)
        plain_ms.append(ps.push_ms)
tg.close(), tp.close()
assert torch.equal(out, pout) and torch.equal(vout, pvout) and gs.base.sum_history == ps.sum_history, "the primal of the gradient push is the plain push's"
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
print(f"{w}x{h}: gradient push  {', '.join(f'{x:.3f}' for x in grad_ms)} ms (best {min(grad_ms):.3f}, worst {max(grad_ms):.3f}); last push: mean gradient "
      f"history {gs.sum_gradient_history / (w * h):.3f}, {gs.pixels_gradient_reset} gradients reset, {gs.base.pixels_reset} reset; "
      f"sum gx_out {float(gouts[0].sum()):.12e}", flush=True)
print(f"{w}x{h}: plain push     {', '.join(f'{x:.3f}' for x in plain_ms)} ms (best {min(plain_ms):.3f}, worst {max(plain_ms):.3f}); sum out {float(pout.sum()):.12e}",
      flush=True)
print(f"gradient push against the plain push (medians): {med(grad_ms):.3f} ms against {med(plain_ms):.3f} ms: x{med(grad_ms) / med(plain_ms):.3f}", flush=True)
