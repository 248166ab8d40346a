"""Manual timing and quality (not collected by pytest): the variance-weighted reconstruction (csrc/hip/recon_weighted.hip). Prints
what profiles/recon_weighted_times.txt records; device times are the library's own solve_ms (HIP events), medians of 11 runs
after two warm-up runs, all in this one process:
  (a) whole solve and CG iterations of weighted L2 and weighted L1 (defaults: K = 20, cg_tol 1e-6) beside reconstruct(L1) and
      fourierSolve, on the heteroscedastic input of tests/recon_weighted_ref.py at 512x512, 1024x1024 and 1280x720;
  (b) the weights pass: a round cut to one CG iteration is weights pass + round set-up + one iteration + residual + one host
      wait; the time of K = 20 minus K = 10 such rounds, over 10, is one round, the same for both reconstructions except for
      their weights pass. The per-iteration time (2N minus N iterations of a stop that is never reached) is subtracted to get at
      the pass itself; what is left still holds the two one-block kernels and the host wait, so the ratio printed is a lower
      bound of the kernels' ratio and the difference printed is exact;
  (c) cbox 128x128, reconnection shift, against the primal of a 4096-spp render: relative L2 error of the primal mean, L2, L1,
      weighted L2 and weighted L1 after 16 passes of 4 and of 16 spp.
    python tests/time_recon_weighted.py [--quick]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gdpt_amd as G
import hip_rt as H
import recon_weighted_ref as RW

quick = "--quick" in sys.argv
REPS, N = (3, 64) if quick else (11, 256)
NEVER = 1e-300                      # a relative residual no fp64 solve reaches: every iteration asked for is run
EPS = dict(eps_init=0.05, eps_decay=0.5, eps_floor=1e-3)


def median(f):
    return float(np.median([f() for _ in range(REPS)]))


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


for w, h in ((512, 512), (1024, 1024), (1280, 720)):
    clean, *planes = RW.heteroscedastic(w, h, seed=1)
    ptr = [H.upload(G, a) for a in planes]
    out = H.alloc(G, 8 * w * h * 3)

    def l1(iters=1000, k=20, tol=1e-6):
        return G.reconstruct_device(w, h, ptr[0], ptr[1], ptr[2], out, 0.04, irls_iters=k, cg_tol=tol, cg_max_iters=iters, **EPS)

    def weighted(norm, iters=1000, k=20, tol=1e-6):
        return G.reconstruct_weighted_device(w, h, *ptr, out, 0.04, norm=norm, irls_iters=k, cg_tol=tol, cg_max_iters=iters, **EPS)

    def fourier():
        return G.poisson_solve_device(w, h, ptr[0], ptr[1], ptr[2], out, want_stats=True)

    for _ in range(2):
        l1(); weighted(G.RECON_L2); weighted(G.RECON_L1); fourier()
    rows = []
    entries = (("fourierSolve", fourier, lambda st: (st.solve_ms, st.iterations)), ("reconstruct(L1)", l1, lambda st: (st.solve_ms, st.cg_iters_total)),
               ("weighted L2", lambda: weighted(G.RECON_L2), lambda st: (st.recon.solve_ms, st.recon.cg_iters_total)),
               ("weighted L1", lambda: weighted(G.RECON_L1), lambda st: (st.recon.solve_ms, st.recon.cg_iters_total)))
    for name, f, get in entries:
        its = get(f())[1]
        err = rel(H.to_host(G, out, (h, w, 3)), clean)
        rows.append(f"{name} {median(lambda: get(f())[0]):.2f} ms, {its} CG iterations, error {err:.4f}")
    print(f"(a) {w}x{h}: " + "; ".join(rows) + f"; primal error {rel(planes[0], clean):.4f}", flush=True)

    t_iter = (median(lambda: l1(2 * N, 0, NEVER).solve_ms) - median(lambda: l1(N, 0, NEVER).solve_ms)) / N
    round_l1 = (median(lambda: l1(1, 20).solve_ms) - median(lambda: l1(1, 10).solve_ms)) / 10
    round_w = (median(lambda: weighted(G.RECON_L1, 1, 20).recon.solve_ms) - median(lambda: weighted(G.RECON_L1, 1, 10).recon.solve_ms)) / 10
    conf = median(lambda: weighted(G.RECON_L2, 1).recon.solve_ms) - median(lambda: l1(1, 0).solve_ms)
    print(f"(b) {w}x{h}: one round of one iteration: L1 {round_l1 * 1e3:.1f} us, weighted {round_w * 1e3:.1f} us (difference {(round_w - round_l1) * 1e3:+.1f} us); "
          f"one iteration {t_iter * 1e3:.1f} us; round minus iteration: L1 {(round_l1 - t_iter) * 1e3:.1f} us, weighted {(round_w - t_iter) * 1e3:.1f} us, "
          f"ratio {(round_w - t_iter) / (round_l1 - t_iter):.2f}; confidence passes + both weights passes of a one-round solve, over L1's: {conf * 1e3:+.1f} us", flush=True)
    for p in ptr + [out]:
        H.free(G, p)

if not quick:
    from helpers import scene_variant
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sc = G.Scene(G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=128, height=128)))
        ref = sc.render(4096, G.RNG_SAMPLE, shift=G.SHIFT_RECONNECT)[0]["img"]
        for spp in (4, 16):
            ses = G.Progressive(sc, 16 * spp, shift=G.SHIFT_RECONNECT)
            ses.run(pass_spp=spp)
            means, _, _ = ses.read()
            imgs = {"primal": means["img"], "L2": ses.reconstruct()[0], "L1": ses.reconstruct(norm=G.RECON_L1)[0]}
            imgs["weighted L2"], st = ses.reconstruct_weighted()
            imgs["weighted L1"], _ = ses.reconstruct_weighted(norm=G.RECON_L1)
            print(f"(c) cbox 128x128 reconnect, 16 x {spp} spp, against the 4096-spp primal: " + ", ".join(f"{k} {rel(v, ref):.4f}" for k, v in imgs.items()) +
                  f"; scales {st.scale_data:.3e} / {st.scale_grad:.3e}, rows dropped {st.rows_dropped}, pixels isolated {st.pixels_isolated}", flush=True)
            ses.close()
