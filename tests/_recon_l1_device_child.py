"""Child of test_device_entry_point_streams_and_forgotten_scratch (not collected by pytest)."""
import os, sys
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import gdpt_amd as G
import recon_l1_ref as R

P = dict(irls_iters=5, eps_init=0.05, eps_decay=0.5, eps_floor=1e-3, cg_tol=1e-6, cg_max_iters=1000)
ok = True
for w, h in ((33, 20), (128, 96), (2, 2)):
    _, u, gx, gy = R.synthetic(w, h, seed=4)
    host, hs = G.reconstruct(w, h, u, gx, gy, 0.04, **P)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u, gx, gy)]
    outs = []

    def run(stream=None):
        out = torch.full((h, w, 3), 7.0, dtype=torch.float64, device=dev)
        st = G.reconstruct_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), 0.04, stream=stream, **P)
        torch.cuda.synchronize()
        outs.append((out.cpu().numpy(), st.cg_iters_total, st.energy_last))

    run(); run()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run(side.cuda_stream); run(side.cuda_stream)
    G.poisson_forget_stream(side.cuda_stream)            # drops the reconstruction's scratch with the solver's
    run(side.cuda_stream)
    G.poisson_forget_stream(side.cuda_stream)
    G.poisson_forget_stream(0); run()
    same = all(np.array_equal(o, host) and it == hs.cg_iters_total and e == hs.energy_last for o, it, e in outs)
    # norm = L2 on device pointers: the default solver's bits
    a = torch.zeros((h, w, 3), dtype=torch.float64, device=dev); b = torch.zeros_like(a)
    G.poisson_solve_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), a.data_ptr())
    G.reconstruct_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), b.data_ptr(), 0.04, norm=G.RECON_L2)
    torch.cuda.synchronize()
    same = same and torch.equal(a, b)
    try:
        G.reconstruct_device(w, h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[0].data_ptr(), 0.04, **P)
        same = False                                      # the output must not alias an input
    except G.GdptError:
        pass
    print(f"{w}x{h} equal: {same}", flush=True)
    ok = ok and same
print("ALL EQUAL" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
