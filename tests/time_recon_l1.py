"""Manual timing (not collected by pytest): the L1 reconstruction (csrc/hip/recon_l1.hip) on the synthetic inputs of
tests/recon_l1_ref.py at 512x512, 1024x1024 and 1280x720. Prints what profiles/recon_l1_times.txt records:
  * per PCG iteration (pcg_step_a + pcg_step_b) beside the per-iteration time of the existing GDPT_SOLVER_CG (cg_step_a + cg_step_b),
    same process: each solver runs N and 2N iterations with a stop it cannot reach, and the difference of the two device times
    (HIP events, the library's own solve_ms) is divided by N, which removes set-up and the first pass; median of 11 runs each;
  * the whole default solve (K = 20, cg_tol 1e-6): total, CG iterations, and the share of the weights passes (measured as the
    time of a run whose CG is cut to one iteration per round, minus that one iteration).
    python tests/time_recon_l1.py [--quick]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G
import recon_l1_ref as R

quick = "--quick" in sys.argv
REPS, N = (3, 64) if quick else (11, 256)
NEVER = 1e-300                      # a relative residual no fp64 solve reaches: every iteration asked for is run


def median(f):
    return float(np.median([f() for _ in range(REPS)]))


for w, h in ((512, 512), (1024, 1024), (1280, 720)):
    clean, u, gx, gy = R.synthetic(w, h, seed=1)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u, gx, gy)]
    out = torch.zeros_like(t[0])
    ptr = [x.data_ptr() for x in t]

    def pcg(iters, k=0, tol=NEVER):
        return G.reconstruct_device(w, h, ptr[0], ptr[1], ptr[2], out.data_ptr(), 0.04, irls_iters=k, eps_init=0.05, eps_decay=0.5, eps_floor=1e-3,
                                    cg_tol=tol, cg_max_iters=iters)

    def cg(iters):
        return G.poisson_solve_device(w, h, ptr[0], ptr[1], ptr[2], out.data_ptr(), solver=G.SOLVER_CG, tol=NEVER, max_iters=iters, want_stats=True)

    for _ in range(2):                                   # warm-up: code objects, workspaces
        pcg(N); cg(N)
    # chunks are 32 iterations long in both solvers, so N and 2N iterations are run exactly
    t_pcg = (median(lambda: pcg(2 * N).solve_ms) - median(lambda: pcg(N).solve_ms)) / N * 1e3
    t_cg = (median(lambda: cg(2 * N).solve_ms) - median(lambda: cg(N).solve_ms)) / N * 1e3
    print(f"{w}x{h}: per iteration: weighted PCG {t_pcg:.2f} us, existing CG {t_cg:.2f} us, ratio {t_pcg / t_cg:.2f}", flush=True)
    K = 20
    st = pcg(1000, K, 1e-6)
    whole = median(lambda: pcg(1000, K, 1e-6).solve_ms)
    one = median(lambda: pcg(1, K, 1e-6).solve_ms)      # 21 weights passes + 21 iterations + the final energy pass
    weights_ms = one - (K + 1) * t_pcg * 1e-3
    img = out.cpu().numpy()
    rel = lambda a: float(np.linalg.norm(a - clean) / np.linalg.norm(clean))
    print(f"{w}x{h}: default solve (K = {K}, cg_tol 1e-6): {whole:.2f} ms, {st.cg_iters_total} CG iterations ({st.cg_iters_total / (K + 1):.0f} per round, "
          f"last round {st.cg_iters_last}), weights passes {weights_ms:.3f} ms = {100 * weights_ms / whole:.1f} %; energy {st.energy_first:.1f} -> {st.energy_last:.1f}; "
          f"rel. L2 error against the clean image: L1 {rel(img):.3f}, primal {rel(u):.3f}", flush=True)
