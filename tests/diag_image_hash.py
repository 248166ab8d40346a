"""Manual (not collected by pytest): sha1 hashes of what the image-space kernels write, and the sums, energies and iteration counts
they report, from two builds of the library, each in a fresh child process; the last line says whether all of them are equal.
Poisson solve (the three solvers), gdpt_assemble_solve_device, L1 reconstruction (clean, NaN where no row reads, NaN inside),
variance-weighted reconstruction with NaN / negative variances and an isolated pixel, spread at radius 0 and 2, the non-local-means
family in both forms of nlm_direct (plain; guided with 2 groups; demodulated with and without a guide; joint with 2 companions, guided
and not; the regression and its collaborative form with 3 regressors, the coefficient film included; a-trous with 3 levels; every
output film hashed, every reported sum bit for bit), and a progressive session's fold, merge and variance read-out; on a 37 x 21 film (ragged for both tile sizes, several blocks) and a
1025 x 345 one (the second trip of every loop over groups or tiles, and of the partial reduction). Seeded inputs, small iteration caps.
    python tests/diag_image_hash.py <other.so>"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILMS = ((37, 21), (1025, 345))


def child(lib_path):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile
    import numpy as np
    import torch
    import gdpt_amd as G
    if lib_path != "-":
        G.LIB_PATH = os.path.abspath(lib_path)
    from helpers import scene_variant

    out = {}

    def sha(a):
        return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]

    def num(x):          # a reported double, bit for bit
        return float(x).hex()

    def inputs(w, h, seed):
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:h, 0:w]
        base = (0.5 + 0.3 * np.sin(0.11 * x + 0.07 * y))[:, :, None] * np.array([1.0, 0.7, 0.4])
        c = base + 0.05 * rng.standard_normal((h, w, 3))
        gx = np.zeros_like(c); gy = np.zeros_like(c)
        gx[:, 1:] = base[:, 1:] - base[:, :-1]; gy[1:] = base[1:] - base[:-1]
        gx += 0.02 * rng.standard_normal((h, w, 3)); gy += 0.02 * rng.standard_normal((h, w, 3))
        gx[rng.random((h, w)) < 0.01] += 3.0          # outliers, for the reweighting to act on
        return rng, c, gx, gy

    dev = torch.device("cuda", 0)
    for (w, h) in FILMS:
        tag = f"{w}x{h}"
        rng, c, gx, gy = inputs(w, h, 7)
        # --- screened Poisson, the three solvers (the CG's cap ends it in its second chunk of iterations)
        for name, solver in (("cg", G.SOLVER_CG), ("dct", G.SOLVER_DCT), ("dct_mfma", G.SOLVER_DCT_MFMA)):
            f, st = G.fourierSolve(w, h, c, gx, gy, 0.2, solver=solver, tol=1e-30, max_iters=40, return_stats=True)
            out[f"{tag} poisson {name}"] = [sha(f), st.iterations, num(st.rel_residual)]
        # --- assembly + solve in one call, on device buffers
        raw = [torch.from_numpy(0.5 * a if k else a).to(dev).contiguous() for k, a in enumerate((c, gx, gy, gx[:, ::-1].copy(), gy[::-1].copy()))]
        dst = [torch.empty_like(raw[0]) for _ in range(4)]
        for name, solver in (("cg", G.SOLVER_CG), ("dct", G.SOLVER_DCT), ("dct_mfma", G.SOLVER_DCT_MFMA)):
            st = G.assemble_solve_device(w, h, [t.data_ptr() for t in raw], [t.data_ptr() for t in dst[:3]], dst[3].data_ptr(), 0.2, solver=solver,
                                         tol=1e-30, max_iters=40, want_stats=True)
            torch.cuda.synchronize()
            out[f"{tag} assemble_solve {name}"] = [sha(t.cpu().numpy()) for t in dst] + [st.iterations, num(st.rel_residual)]
        # --- L1 reconstruction: clean; NaN where no row reads (gx of the first column, gy of the first row); NaN in an inner gradient
        recon = dict(irls_iters=2, cg_max_iters=40, cg_tol=1e-30)
        gx_b, gy_b = gx.copy(), gy.copy(); gx_b[:, 0] = np.nan; gy_b[0] = np.nan
        gx_n = gx.copy(); gx_n[h // 2, w // 2, 1] = np.nan
        for name, (a, b) in (("clean", (gx, gy)), ("nan_unread", (gx_b, gy_b)), ("nan_inside", (gx_n, gy))):
            f, st = G.reconstruct(w, h, c, a, b, 0.2, norm=G.RECON_L1, **recon)
            out[f"{tag} recon_l1 {name}"] = [sha(f), int(np.isnan(f).sum()), st.irls_rounds, st.cg_iters_total, st.cg_iters_last, num(st.energy_first),
                                             num(st.energy_last), num(st.rel_residual_last)]
        # --- variance-weighted reconstruction, both norms: some NaN and negative variances, a NaN input, one isolated pixel
        vc, vgx, vgy = (0.0025 * (0.5 + rng.random((h, w, 3))) for _ in range(3))
        vc[3, 4, 0] = np.nan; vgx[5, 9, 2] = -1.0; vgy[h - 1, w - 1, 1] = np.nan; vc[h - 2, 1] = 0.0
        cw = c.copy(); cw[2, 2, 1] = np.nan
        iy, ix = 7, 5
        vc[iy, ix] = np.nan; vgx[iy, ix] = np.nan; vgx[iy, ix + 1] = np.nan; vgy[iy, ix] = np.nan; vgy[iy + 1, ix] = np.nan
        for name, norm in (("l2", G.RECON_L2), ("l1", G.RECON_L1)):
            f, conf, st = G.reconstruct_weighted(w, h, cw, gx, gy, vc, vgx, vgy, 0.2, norm=norm, confidence=True, **recon)
            out[f"{tag} recon_weighted {name}"] = [sha(f), sha(conf), int(np.isnan(f).sum()), st.recon.irls_rounds, st.recon.cg_iters_total, num(st.recon.energy_first),
                                                   num(st.recon.energy_last), num(st.recon.rel_residual_last), num(st.scale_data), num(st.scale_grad),
                                                   st.rows_dropped, st.pixels_isolated]
        # --- spread of three members, radius 0 and 2, one pixel left out
        members = [c + 0.03 * rng.standard_normal((h, w, 3)) for _ in range(3)]
        members[1][1, 3, 0] = np.inf
        for radius in (0, 2):
            var, emap, st = G.recon_spread(members, [4.0, 8.0, 20.0], total=c, radius=radius)
            out[f"{tag} spread r{radius}"] = [sha(var), sha(emap), num(st.sum_var), num(st.sum_sq), st.pixels_left_out]
        # --- the NLM family, both forms: one pixel with a negative variance, one with a negative feature variance
        var = 0.0025 * (0.5 + rng.random((h, w, 3))); var[4, 6, 1] = -1.0
        yy, xx = np.mgrid[0:h, 0:w]
        feat = np.stack([0.4 + 0.3 * np.sin(0.05 * (k + 1) * xx + 0.09 * yy + k) for k in range(8)]) + 0.02 * rng.standard_normal((8, h, w))
        feat[7] = np.clip(feat[7] + 0.4, 0.0, 1.0)            # the coverage plane
        fvar = 4e-4 * (0.5 + rng.random((8, h, w))); fvar[1, 9, 11] = -1.0
        comps = [c[::-1].copy(), 0.5 * c + 0.1]; comp_vars = [var[::-1].copy(), 0.25 * var]
        guide = G.nlm_guide(groups=[(0, 3, 1e-3), (3, 3, 1e-3)])
        regress = G.nlm_regress(channels=[0, 3, 6], scales=[1.0, 0.5, 2.0])

        def sums(st):
            return [num(st.sum_var_in), num(st.sum_sq_in), num(st.sum_var_out), num(st.sum_sq_out), st.pixels_left_out]

        def joint(**kw):
            f, vf, co, cvo, st = G.denoise_nlm_joint(c, var, comps, comp_vars, **kw)
            return [f, vf] + co + cvo, sums(st.guide) + [num(st.sum_var_in[j]) for j in range(2)] + [num(st.sum_var_out[j]) for j in range(2)]

        def collab(**kw):
            f, planes, st = G.denoise_nlm_collab(c, var, feat, fvar, guide=guide, regress=regress, coef=True, **kw)
            return [f, planes], sums(st)

        def films(call):          # a call that returns its output films and then its GdptNlmStats
            def run(**kw):
                *arrays, st = call(**kw)
                return arrays, sums(st)
            return run

        rf = dict(window_radius=4, patch_radius=2)
        cases = (("nlm", films(lambda **kw: G.denoise_nlm(c, var, **kw)), rf),
                 ("nlm guided", films(lambda **kw: G.denoise_nlm_guided(c, var, feat, fvar, guide=guide, **kw)), rf),
                 ("nlm demod", films(lambda **kw: G.denoise_nlm_demod(c, var, feat, fvar, **kw)), rf),
                 ("nlm demod guided", films(lambda **kw: G.denoise_nlm_demod(c, var, feat, fvar, guide=guide, **kw)), rf),
                 ("nlm joint", joint, rf),
                 ("nlm joint guided", lambda **kw: joint(feat=feat, feat_var=fvar, guide=guide, **kw), rf),
                 ("nlm regress", films(lambda **kw: G.denoise_nlm_regress(c, var, feat, fvar, guide=guide, regress=regress, **kw)), rf),
                 ("nlm regress f0", films(lambda **kw: G.denoise_nlm_regress(c, var, feat, fvar, guide=guide, regress=regress, **kw)),
                  dict(window_radius=3, patch_radius=0)),
                 ("nlm collab", collab, rf),
                 ("atrous", films(lambda **kw: G.denoise_atrous(c, var, **kw)), dict(levels=3)),
                 ("atrous guided demod", films(lambda **kw: G.denoise_atrous(c, var, feat, fvar, guide=guide, demod=G.nlm_demod(), **kw)), dict(levels=3)))
        for name, call, kw in cases:
            for form in (0, 1):
                with G.debug_knobs(nlm_direct=form):
                    arrays, figures = call(**kw)
                out[f"{tag} {name} {'direct' if form else 'tiled'}"] = [sha(a) for a in arrays] + figures
        # --- a progressive session: three folds, then two slice sessions merged into an accumulator, and the variance read-out of each
        with tempfile.TemporaryDirectory() as tmp:
            scene = G.Scene(G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=w, height=h)))
            s = G.Progressive(scene, 4)
            for spp in (1, 2, 1):
                s.add_pass(spp)
            parts = [G.Progressive(scene, 4, slice=(0, 2)), G.Progressive(scene, 4, slice=(2, 2))]
            for p in parts:
                p.add_pass(1); p.add_pass(1)
            acc = G.Progressive(scene, 4, slice=(0, 0))
            for p in parts:
                acc.merge(p)
            for name, sess in (("fold", s), ("merge", acc)):
                means, vars_, asm = sess.read()
                st = sess.status()
                out[f"{tag} progressive {name}"] = [sha(np.stack([means[k] for k in sess.names])), sha(np.stack([vars_[k] for k in sess.names])),
                                                    sha(np.stack([asm[k] for k in ("c", "cx", "cy")])), num(st["error"]), st["pixels_left_out"], st["passes"]]
            for x in parts + [acc, s]:
                x.close()
            scene.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        got = {}
        for tag, lib in (("tree ", "-"), ("other", sys.argv[1])):
            r = subprocess.run([sys.executable, __file__, "child", lib], capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
            if r.returncode != 0 or not line:
                print(tag, "failed with exit status", r.returncode, r.stderr[-800:], flush=True)
                sys.exit(2)          # nothing more is started after a failed child
            got[tag] = json.loads(line[0][7:])
            for k, v in got[tag].items():
                print(tag, k, *v, flush=True)
        diff = [k for k in got["tree "] if got["tree "][k] != got["other"].get(k)]
        print("ALL EQUAL" if not diff and len(got["tree "]) == len(got["other"]) else "DIFFERENT: " + "; ".join(diff))
        sys.exit(1 if diff else 0)
