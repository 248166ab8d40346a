"""The host side of the variance smoothing (include/gdpt.h: gdpt_variance_smooth*, gdpt_progressive_denoise_smoothed), without a GPU:
the struct layouts of the Python mirror against the header, the documented defaults, the refusals, which come before any device call
and name their field, and the argument errors of the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_struct_layout_matches_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(GdptVarSmoothParams), offsetof(GdptVarSmoothParams, reserved), '
                   'sizeof(GdptVarSmoothStats), offsetof(GdptVarSmoothStats, sum_var_in), offsetof(GdptVarSmoothStats, sum_var_out), '
                   'offsetof(GdptVarSmoothStats, smooth_ms), offsetof(GdptVarSmoothStats, radius), GDPT_VAR_SMOOTH_MAX_RADIUS, GDPT_DENOISE_PLAIN, '
                   'GDPT_DENOISE_GUIDED, GDPT_DENOISE_DEMOD); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P, S = G.GdptVarSmoothParams, G.GdptVarSmoothStats
    assert got[:2] == [C.sizeof(P), P.reserved.offset] == [16, 4]
    assert got[2:7] == [C.sizeof(S), S.sum_var_in.offset, S.sum_var_out.offset, S.smooth_ms.offset, S.radius.offset] == [40, 8, 16, 24, 32]
    assert got[7:] == [G.VAR_SMOOTH_MAX_RADIUS, G.DENOISE_PLAIN, G.DENOISE_GUIDED, G.DENOISE_DEMOD] == [4, 0, 1, 2]


def test_default_params(G):
    p = G.GdptVarSmoothParams(7, (C.c_int32 * 3)(5, 5, 5))
    G.lib().gdpt_var_smooth_default_params(C.byref(p))
    assert (p.radius, list(p.reserved)) == (2, [0, 0, 0])
    q = G.var_smooth_params(radius=4)
    assert (q.radius, list(q.reserved)) == (4, [0, 0, 0])
    assert G.var_smooth_params().radius == 2
    G.lib().gdpt_var_smooth_default_params(None)          # a null block is ignored


def test_refused_arguments_name_their_field(G):
    a, b, c, d, e = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000      # never dereferenced: every call below is refused on the host
    dev = G.variance_smooth_device
    dm = G.nlm_demod()
    bad_p = G.var_smooth_params()
    bad_p.reserved[2] = 1
    bad_d = G.nlm_demod()
    bad_d.reserved[0] = 1
    for args, kw, match in (((4, 3, 0, b, e), {}, "img is null"), ((4, 3, a, 0, e), {}, "var is null"), ((4, 3, a, b, 0), {}, "var_out is null"),
                            ((4, 3, a, b, a), {}, "var_out must not alias"), ((4, 3, a, b, b), {}, "var_out must not alias"),
                            ((4, 3, a, b, c), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=dm), "var_out must not alias"),
                            ((4, 3, a, b, d), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=dm), "var_out must not alias"),
                            ((0, 3, a, b, e), {}, "width"), ((4, 0, a, b, e), {}, "height"), ((4, -1, a, b, e), {}, "height"),
                            ((4, 3, a, b, e), dict(radius=-1), "radius"), ((4, 3, a, b, e), dict(radius=5), "radius"),
                            ((4, 3, a, b, e), dict(params=bad_p), "reserved"),
                            # the planes and the block go together
                            ((4, 3, a, b, e), dict(demod=dm, num_channels=8), "feat is null"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, demod=dm, num_channels=8), "feat_var is null"),
                            ((4, 3, a, b, e), dict(feat_var_ptr=d, demod=dm, num_channels=8), "feat is null"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8), "demod is null"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, num_channels=8), "demod is null"),
                            # the block is checked as the demodulated filter checks it
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=G.nlm_demod(albedo_channel=6, coverage_channel=-1)), "albedo_channel"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=7, demod=dm), "coverage_channel"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=G.nlm_demod(coverage_channel=1)), "coverage_channel"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=G.nlm_demod(floor=0.0)), "floor"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=G.nlm_demod(floor=np.nan)), "floor"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=17, demod=dm), "num_channels"),
                            ((4, 3, a, b, e), dict(feat_ptr=c, feat_var_ptr=d, num_channels=8, demod=bad_d), "reserved")):
        with pytest.raises(G.GdptError, match=match):
            dev(*args, **kw)
    # the host entry refuses the same
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    for kw, match in ((dict(radius=5), "radius"), (dict(params=bad_p), "reserved"), (dict(feat=p, feat_var=0.0 * p, demod=G.nlm_demod(floor=-1.0)), "floor"),
                      (dict(demod=dm), "feat is null"), (dict(feat=p[:7], feat_var=0.0 * p[:7]), "coverage_channel")):
        with pytest.raises(G.GdptError, match=match):
            G.variance_smooth(f, 0.01 * f, **kw)
    with pytest.raises(G.GdptError, match="one shape"):
        G.variance_smooth(f, np.ones((3, 5, 3)))
    with pytest.raises(G.GdptError, match="one shape"):
        G.variance_smooth(f, 0.01 * f, feat=np.ones((8, 3, 5)), feat_var=np.ones((8, 3, 5)))
    with pytest.raises(G.GdptError, match="go together"):
        G.variance_smooth(f, 0.01 * f, feat=p)


def test_the_session_entry_refuses_on_the_host(G):
    L = G.lib()

    def call(session, kind, smooth=None, nlm=None, guide=None, demod=None, out=0x1000, features=None):
        rc = L.gdpt_progressive_denoise_smoothed(session, kind, smooth, nlm, guide, demod, 4, 1, out, None, None, features, None, None, None)
        return rc, L.gdpt_last_error().decode()

    rc, msg = call(None, 0)
    assert rc != 0 and "null session" in msg
    fake = 0x7000                                          # never dereferenced: the parameter blocks are checked first
    bad_p = G.var_smooth_params(radius=9)
    for kw, match in ((dict(kind=0, out=None), "out is null"), (dict(kind=3), "kind"), (dict(kind=-1), "kind"),
                      (dict(kind=0, smooth=C.byref(bad_p)), "radius"), (dict(kind=1, nlm=C.byref(G.nlm_params(window_radius=11))), "window_radius"),
                      (dict(kind=0, guide=C.byref(G.nlm_guide())), "guide must be null"), (dict(kind=0, demod=C.byref(G.nlm_demod())), "demod must be null"),
                      (dict(kind=1, demod=C.byref(G.nlm_demod())), "demod must be null"), (dict(kind=0, features=0x2000), "features"),
                      (dict(kind=1, guide=C.byref(G.nlm_guide(k_f=0.0))), "k_f"),
                      (dict(kind=2, guide=C.byref(G.nlm_guide(num_channels=7, groups=[(3, 3, 1e-3)]))), "num_channels"),
                      (dict(kind=2, demod=C.byref(G.nlm_demod(floor=0.0))), "floor")):
        rc, msg = call(fake, **kw)
        assert rc != 0 and match in msg, (kw, msg)


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.variance_smooth(f, 0.01 * f)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.variance_smooth(f, 0.01 * f, feat=p, feat_var=0.0 * p, radius=4)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.variance_smooth_device(4, 3, 0x1000, 0x2000, 0x5000, radius=0)


CLI_ERRORS = [(["--nlm-var-smooth", "2"], "--nlm-var-smooth needs --denoised"),
              (["--pass-spp", "4", "--nlm-var-smooth", "2"], "--nlm-var-smooth needs --denoised"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-var-smooth", "5"], "--nlm-var-smooth takes a radius from 0 to 4"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-var-smooth", "-1"], "--nlm-var-smooth takes a radius from 0 to 4"),
              (["--denoised", "d.pfm", "--nlm-var-smooth", "2"], "--denoised needs --pass-spp"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-var-smooth", "2", "--nlm-demodulate", "--nlm-guide", "albedo"], "the albedo is already divided out")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.pfm", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
