"""GPU variance-weighted reconstruction (gdpt_reconstruct_weighted*, gdpt_progressive_reconstruct_weighted,
csrc/hip/recon_weighted.hip) through the C ABI via the Python mirror, against the CPU restatement tests/recon_weighted_ref.py
(pinned by tests/test_recon_weighted_ref.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import hip_rt as H
import recon_l1_ref as R
import recon_weighted_ref as RW
from helpers import ROOT, rel_l2, scene_variant

pytestmark = pytest.mark.gpu

ALPHA = 0.04
K = 10
# inner solves far below the bound of the comparison: the restatement solves directly, the GPU by PCG to 1e-10
TIGHT = dict(eps_init=0.05, eps_decay=0.5, eps_floor=1e-3, cg_tol=1e-10, cg_max_iters=5000)
EXTENTS = [(17, 9), (33, 40), (64, 48)]      # a ragged tile; across the 32 x 8 tile boundary both ways; several tiles


@functools.lru_cache(maxsize=None)
def case(w, h, seed):
    """The heteroscedastic input and the restatement's iterates 0..K on it, computed once and shared (read only)."""
    clean, *planes = RW.heteroscedastic(w, h, seed)
    _, energies, iterates, conf = RW.weighted(*planes, ALPHA, K, 0.05, TIGHT["eps_init"], TIGHT["eps_decay"], TIGHT["eps_floor"])
    return clean, planes, energies, iterates, conf


@pytest.mark.parametrize("norm", ["wl2", "wl1"])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("w,h", EXTENTS)
def test_gpu_equals_the_restatement(G, w, h, seed, norm):
    """Weighted L2 (one solve) and weighted L1 (K = 10) against the direct solves of the restatement: 1e-7 relative L2, the bound of
    the L1 test against its restatement (test_gpu_recon_l1.py)."""
    _, planes, energies, iterates, conf = case(w, h, seed)
    if norm == "wl2":
        out, st = G.reconstruct_weighted(w, h, *planes, ALPHA, norm=G.RECON_L2, **TIGHT)
        ref, e_ref, rounds = iterates[0], energies[0], 1
    else:
        out, st = G.reconstruct_weighted(w, h, *planes, ALPHA, norm=G.RECON_L1, irls_iters=K, **TIGHT)
        ref, e_ref, rounds = iterates[K], energies[K], K + 1
    err = rel_l2(out, ref)
    print(f"{norm} {w}x{h} seed {seed}: rel L2 {err:.3e}, CG iterations {st.recon.cg_iters_total}, residual {st.recon.rel_residual_last:.2e}, "
          f"energy {st.recon.energy_last:.6f} (restatement {e_ref:.6f})")
    assert err < 1e-7
    assert st.recon.irls_rounds == rounds and st.recon.norm == (G.RECON_L2 if norm == "wl2" else G.RECON_L1)
    assert abs(st.recon.energy_last - e_ref) <= 1e-8 * e_ref
    assert st.recon.rel_residual_last <= TIGHT["cg_tol"] and st.recon.cg_iters_total > 0 and st.recon.solve_ms > 0
    assert st.rows_dropped == 0 and st.pixels_isolated == 0


def check_confidence(G, w, h, planes, delta):
    want = RW.confidences(*planes, delta)
    out, conf, st = G.reconstruct_weighted(w, h, *planes, ALPHA, conf_floor=delta, confidence=True, **TIGHT)
    assert abs(st.scale_data - want["scale_data"]) <= 1e-12 * want["scale_data"]
    assert abs(st.scale_grad - want["scale_grad"]) <= 1e-12 * want["scale_grad"]
    assert (st.rows_dropped, st.pixels_isolated) == (want["rows_dropped"], want["pixels_isolated"])
    for k, name in enumerate(("kd", "kx", "ky")):
        assert np.array_equal(conf[..., k] == 0, want[name] == 0), name
        assert rel_l2(conf[..., k], want[name]) <= 1e-12, name
        assert np.abs(conf[..., k] - want[name]).max() <= 1e-12 * np.abs(want[name]).max(), name
    assert np.isfinite(out).all()
    return out, st


@pytest.mark.parametrize("w,h", EXTENTS)
def test_confidence_planes_scales_and_counts(G, w, h):
    """kappa planes and the two scales against numpy to 1e-12 relative, counts exactly: on the plain input and on one with zero
    variances, a NaN and a negative variance, NaN / inf triples and an isolated pixel (recon_weighted_ref.spoil). The image of the
    spoiled input is finite, 0 at the isolated pixel, and the restatement's."""
    _, planes, _, _, _ = case(w, h, 1)
    check_confidence(G, w, h, planes, 0.05)
    check_confidence(G, w, h, planes, 0.5)
    bad = RW.spoil(*planes)
    out, st = check_confidence(G, w, h, bad, 0.05)
    assert st.rows_dropped == 9 and st.pixels_isolated == 1 and (out[6, 9] == 0).all()
    ref = RW.weighted(*bad, ALPHA, 0)[0]
    assert rel_l2(out, ref) < 1e-7
    out1, st1 = G.reconstruct_weighted(w, h, *bad, ALPHA, norm=G.RECON_L1, irls_iters=3, **TIGHT)
    assert np.isfinite(out1).all() and rel_l2(out1, RW.weighted(*bad, ALPHA, 3)[0]) < 1e-7
    # a family without a row of positive variance: scale 1, kappa = 1 / delta
    z = np.zeros_like(planes[0])
    _, conf, st = G.reconstruct_weighted(w, h, planes[0], planes[1], planes[2], z, z, z, ALPHA, confidence=True, **TIGHT)
    assert st.scale_data == 1.0 and st.scale_grad == 1.0 and (conf[..., 0] == 20.0).all() and (conf[:, 1:, 1] == 20.0).all()


@pytest.mark.parametrize("irls", [0, 5])        # the mirror's 0 is the C struct's negative count: round 0 alone
@pytest.mark.parametrize("w,h", [(33, 40), (64, 48)])
def test_uniform_variances_give_the_unweighted_reconstruction(G, w, h, irls):
    _, u, gx, gy = R.synthetic(w, h, seed=2)
    one = np.ones_like(u)
    ref, rs = G.reconstruct(w, h, u, gx, gy, ALPHA, irls_iters=irls, **TIGHT)
    out, conf, st = G.reconstruct_weighted(w, h, u, gx, gy, 0.37 * one, 0.011 * one, 0.011 * one, ALPHA, norm=G.RECON_L1, irls_iters=irls,
                                           confidence=True, **TIGHT)
    err = rel_l2(out, ref)
    print(f"{w}x{h} K = {irls}: rel L2 {err:.3e}; CG iterations {st.recon.cg_iters_total} against {rs.cg_iters_total}")
    assert err < 1e-7 and st.recon.irls_rounds == rs.irls_rounds == irls + 1
    k0 = 1 / 1.05
    assert np.abs(conf[..., 0] - k0).max() < 1e-14 and np.abs(conf[:, 1:, 1] - k0).max() < 1e-14 and np.abs(conf[1:, :, 2] - k0).max() < 1e-14
    assert abs(st.recon.energy_last - k0 * rs.energy_last) <= 1e-8 * rs.energy_last


def device_call(G, w, h, planes, stream=None, **kw):
    ins = [H.upload(G, a) for a in planes]
    out = H.upload(G, np.full((h, w, 3), 7.0))
    conf = [H.upload(G, np.full((h, w), 7.0)) for _ in range(3)]
    try:
        st = G.reconstruct_weighted_device(w, h, *ins, out, ALPHA, confidence_ptrs=conf, stream=stream, **kw)
        return H.to_host(G, out, (h, w, 3)), np.stack([H.to_host(G, c, (h, w)) for c in conf], axis=2), st
    finally:
        for p in ins + [out] + conf:
            H.free(G, p)


@pytest.mark.parametrize("w,h", [(33, 40), (64, 48)])
def test_same_inputs_give_the_same_bits_on_every_entry_and_stream(G, w, h):
    _, planes, _, _, _ = case(w, h, 2)
    bad = RW.spoil(*planes)
    kw = dict(norm=G.RECON_L1, irls_iters=4, cg_tol=1e-6)
    for inputs in (planes, bad):
        a, ka, sa = G.reconstruct_weighted(w, h, *inputs, ALPHA, confidence=True, **kw)
        b, kb, sb = G.reconstruct_weighted(w, h, *inputs, ALPHA, confidence=True, **kw)
        runs = [device_call(G, w, h, inputs, **kw), device_call(G, w, h, inputs, **kw)]
        side = H.stream(G)
        runs += [device_call(G, w, h, inputs, stream=side, **kw), device_call(G, w, h, inputs, stream=side, **kw)]
        G.poisson_forget_stream(side)                     # drops the confidence scratch with the solver's
        runs.append(device_call(G, w, h, inputs, stream=side, **kw))
        G.poisson_forget_stream(side)
        H.stream_destroy(G, side)
        for img, conf, st in [(b, kb, sb)] + runs:
            assert np.array_equal(img, a) and np.array_equal(conf, ka)
            assert (st.recon.cg_iters_total, st.recon.energy_last, st.scale_data, st.scale_grad) == (sa.recon.cg_iters_total, sa.recon.energy_last, sa.scale_data, sa.scale_grad)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_weighted_solve_beats_l1_and_l2_on_the_gpu(G, seed):
    """64x48, 16 passes, noise level 0.25 / 2.5 per 16x16 block, gradient outliers of sigma 20 with probability 0.0025 per
    pass-sample (recon_weighted_ref.heteroscedastic): the weighted L2 image is closer to the clean image than L1's (K = 10) and
    than a quarter of the natural-boundary L2's."""
    w, h = 64, 48
    clean, planes, _, _, _ = case(w, h, seed)
    u, gx, gy = planes[:3]
    wl2, _ = G.reconstruct_weighted(w, h, *planes, ALPHA, norm=G.RECON_L2, **TIGHT)
    l1, _ = G.reconstruct(w, h, u, gx, gy, ALPHA, irls_iters=K, **TIGHT)
    l2, _ = G.reconstruct(w, h, u, gx, gy, ALPHA, irls_iters=0, **TIGHT)
    e_w, e_l1, e_l2 = rel_l2(wl2, clean), rel_l2(l1, clean), rel_l2(l2, clean)
    print(f"seed {seed}: primal {rel_l2(u, clean):.4f}  L2 {e_l2:.4f}  L1 {e_l1:.4f}  weighted L2 {e_w:.4f}")
    assert e_w < e_l1 and e_w < 0.25 * e_l2


def test_session(G, scene_tmp):
    """cbox 64x64, reconnection shift, 8 passes of 4 spp: the session call equals the standalone device entry on the planes read()
    returns, bit for bit; refusals; a planted firefly whose variance says so moves the weighted image less than the L2 image."""
    w = h = 64
    sc = G.Scene(G.parse_scene(scene_variant(scene_tmp, "cbox/cbox_gdpt.xml", width=w, height=h)))
    ses = G.Progressive(sc, 32, shift=G.SHIFT_RECONNECT)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="2 passes"):
        ses.reconstruct_weighted()
    for _ in range(7):
        ses.add_pass(4)
    results = {}
    for name, kw in (("wl2", dict(norm=G.RECON_L2)), ("wl1", dict(norm=G.RECON_L1, irls_iters=5))):
        img, conf, st = ses.reconstruct_weighted(confidence=True, **kw)
        assert np.isfinite(img).all() and st.pixels_isolated == 0 and st.recon.cg_iters_total > 0
        results[name] = (img, conf, st)
    assert not np.array_equal(results["wl2"][0], results["wl1"][0])
    means, _, asm = ses.read()
    src = [H.upload(G, means[k]) for k in ("img", "cx0", "cy0", "cx1", "cy1")]
    dst = [H.alloc(G, 8 * w * h * 3) for _ in range(3)]
    G.assemble_device(w, h, src, dst)
    c, cx, cy = [H.to_host(G, p, (h, w, 3)) for p in dst]
    for p in src + dst:
        H.free(G, p)
    planes = [c, cx, cy, asm["c"], asm["cx"], asm["cy"]]
    for name, kw in (("wl2", dict(norm=G.RECON_L2)), ("wl1", dict(norm=G.RECON_L1, irls_iters=5))):
        img, conf, st = device_call(G, w, h, planes, **kw)
        assert np.array_equal(img, results[name][0]) and np.array_equal(conf, results[name][1])
        assert (st.scale_data, st.scale_grad, st.rows_dropped) == (results[name][2].scale_data, results[name][2].scale_grad, results[name][2].rows_dropped)
    # device destinations through the session
    out = H.alloc(G, 8 * w * h * 3)
    kp = [H.alloc(G, 8 * w * h) for _ in range(3)]
    ses.reconstruct_weighted(out_ptr=out, confidence_ptrs=kp)
    assert np.array_equal(H.to_host(G, out, (h, w, 3)), results["wl2"][0])
    assert np.array_equal(np.stack([H.to_host(G, p, (h, w)) for p in kp], axis=2), results["wl2"][1])
    for p in [out] + kp:
        H.free(G, p)
    ses.close()
    # the firefly: +100 in cx at one interior pixel, and what one such pass of K adds to the variance of the mean
    planted, pvar = np.array(cx, copy=True), np.array(asm["cx"], copy=True)
    planted[40, 30] += 100.0
    pvar[40, 30] += 100.0 ** 2
    base, _ = G.reconstruct_weighted(w, h, *planes, ALPHA)
    hit, _ = G.reconstruct_weighted(w, h, c, planted, cy, asm["c"], pvar, asm["cy"], ALPHA)
    l2, _ = G.reconstruct(w, h, c, cx, cy, ALPHA, norm=G.RECON_L2)
    l2p, _ = G.reconstruct(w, h, c, planted, cy, ALPHA, norm=G.RECON_L2)
    assert np.array_equal(base, results["wl2"][0])
    dw, d2 = np.abs(hit - base).max(), np.abs(l2p - l2).max()
    print(f"planted firefly: max deviation weighted L2 {dw:.5f}, L2 {d2:.4f}")
    assert dw < d2
    # an Integrator::Path session has no gradients
    psc = G.Scene(G.parse_scene(scene_variant(scene_tmp, "cbox/cbox_gdpt.xml", width=32, height=32, integrator="path")))
    pses = G.Progressive(psc, 8, path=True)
    pses.add_pass(4), pses.add_pass(4)
    with pytest.raises(G.GdptError, match="Path"):
        pses.reconstruct_weighted()
    pses.close()


def test_refusals(G):
    w = h = 4
    z = np.zeros((h, w, 3))
    p = [H.upload(G, z) for _ in range(7)]
    for bad in range(6):
        with pytest.raises(G.GdptError, match="alias"):
            G.reconstruct_weighted_device(w, h, *p[:6], p[bad], ALPHA)
    for missing in (3, 4, 5):
        args = list(p[:6])
        args[missing] = 0
        with pytest.raises(G.GdptError, match="variance"):
            G.reconstruct_weighted_device(w, h, *args, p[6], ALPHA)
    for kw in (dict(conf_floor=-1.0), dict(conf_floor=float("nan")), dict(dataCost=0.0), dict(dataCost=float("inf"))):
        with pytest.raises(G.GdptError):
            G.reconstruct_weighted_device(w, h, *p, **kw)
    with pytest.raises(G.GdptError):
        G.reconstruct_weighted_device(1, 4, *p)
    st = G.reconstruct_weighted_device(w, h, *p, ALPHA, norm=G.RECON_L1, irls_iters=2)       # all-zero inputs: nothing to solve, no NaN
    assert np.array_equal(H.to_host(G, p[6], (h, w, 3)), z) and st.recon.cg_iters_total == 0
    for q in p:
        H.free(G, q)


def read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = b"PF\n%d %d\n-1\n" % (w, h)
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], dtype="<f4").reshape(h, w, 3)


def test_cli_weighted(G, tmp_path):
    exe = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
    xml = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
    out, kap = tmp_path / "o.pfm", tmp_path / "k.pfm"
    r = subprocess.run([exe, "--spp", "16", "--pass-spp", "4", "--reconstruct", "wl2", "--confidence", str(kap), "-o", str(out), "--film", "48x32", xml],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    sc = G.Scene(G.parse_scene(xml, film=(48, 32)))
    ses = G.Progressive(sc, 16)
    ses.run(pass_spp=4)
    img, conf, _ = ses.reconstruct_weighted(confidence=True)
    assert np.array_equal(read_pfm(out, 48, 32), img.astype(np.float32))
    assert np.array_equal(read_pfm(kap, 48, 32), conf.astype(np.float32))
    r = subprocess.run([exe, "--spp", "16", "--pass-spp", "4", "--reconstruct", "wl1", "--irls-iters", "3", "--conf-floor", "0.2", "-o", str(out), "--film", "48x32", xml],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img1, _ = ses.reconstruct_weighted(norm=G.RECON_L1, irls_iters=3, conf_floor=0.2)
    assert np.array_equal(read_pfm(out, 48, 32), img1.astype(np.float32)) and not np.array_equal(img1, img)
    ses.close()
    r = subprocess.run([exe, "--spp", "16", "--reconstruct", "wl2", "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pass-spp" in r.stderr
    r = subprocess.run([exe, "--spp", "16", "--pass-spp", "4", "--confidence", str(kap), "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
