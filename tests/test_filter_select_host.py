"""The host side of the per-pixel filter selection (include/gdpt.h: gdpt_filter_select*), without a GPU: the struct layouts of the
Python mirror against the header, the documented defaults, the refusals, which come before any device call and name their field,
and the argument errors of the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT


def test_struct_layout_matches_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(GdptSelectParams), offsetof(GdptSelectParams, reserved), '
                   'sizeof(GdptSelectStats), offsetof(GdptSelectStats, chosen), offsetof(GdptSelectStats, sum_e), offsetof(GdptSelectStats, sum_mse), '
                   'offsetof(GdptSelectStats, sum_sq_out), offsetof(GdptSelectStats, select_ms), offsetof(GdptSelectStats, radius), '
                   'offsetof(GdptSelectStats, num_candidates), GDPT_SELECT_MAX_CANDIDATES, GDPT_SELECT_MAX_RADIUS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P, S = G.GdptSelectParams, G.GdptSelectStats
    assert got[:2] == [C.sizeof(P), P.reserved.offset] == [16, 4]
    assert got[2:10] == [C.sizeof(S), S.chosen.offset, S.sum_e.offset, S.sum_mse.offset, S.sum_sq_out.offset, S.select_ms.offset, S.radius.offset,
                         S.num_candidates.offset] == [168, 8, 72, 136, 144, 152, 160, 164]
    assert got[10:] == [G.SELECT_MAX_CANDIDATES, G.SELECT_MAX_RADIUS] == [8, 8]


def test_default_params(G):
    p = G.GdptSelectParams(7, (C.c_int32 * 3)(5, 5, 5))
    G.lib().gdpt_select_default_params(C.byref(p))
    assert (p.radius, list(p.reserved)) == (4, [0, 0, 0])
    q = G.select_params(radius=8)
    assert (q.radius, list(q.reserved)) == (8, [0, 0, 0])
    assert G.select_params().radius == 4
    G.lib().gdpt_select_default_params(None)          # a null block is ignored


def test_refused_arguments_name_their_field(G):
    # addresses that are never dereferenced: every call below is refused on the host
    fa, fb, t = [0x1000, 0x2000], [0x3000, 0x4000], [0x5000, 0x6000]
    ua, va, ub, vb, out, sel, mse, E = 0x7000, 0x8000, 0x9000, 0xa000, 0xb000, 0xc000, 0xd000, 0xe000
    bad_p = G.select_params()
    bad_p.reserved[1] = 1

    def dev(w=4, h=3, fa=fa, fb=fb, t=t, ua=ua, va=va, ub=ub, vb=vb, out=out, **kw):
        return G.filter_select_device(w, h, fa, fb, t, ua, va, ub, vb, out, **kw)

    nine = [0x100000 + 0x1000 * i for i in range(9)]
    for kw, match in ((dict(fa=[], fb=[], t=[]), "n must be in"), (dict(fa=nine, fb=[x + 0x100000 for x in nine], t=[x + 0x200000 for x in nine]), "n must be in"),
                      (dict(fa=[0x1000, 0]), r"FA\[1\] is null"), (dict(fb=[0, 0x4000]), r"FB\[0\] is null"), (dict(t=[0x5000, 0]), r"T\[1\] is null"),
                      (dict(ua=0), "uA is null"), (dict(va=0), "vA is null"), (dict(ub=0), "uB is null"), (dict(vb=0), "vB is null"),
                      (dict(out=0), "out is null"),
                      (dict(radius=-1), "radius"), (dict(radius=9), "radius"), (dict(params=bad_p), "reserved"),
                      (dict(w=0), "width"), (dict(h=0), "height"), (dict(h=-2), "height"),
                      (dict(out=fa[1]), "out must not alias an input"), (dict(out=t[0]), "out must not alias an input"),
                      (dict(out=vb), "out must not alias an input"),
                      (dict(out=fa[1] + 8), "out must not alias an input"), (dict(E_ptr=t[0] - 8 * 2 * 12 + 8), "E must not alias an input"),
                      (dict(sel_ptr=out + 24 * 12 - 4), "sel must not alias out"),   # (overlaps at an offset: byte ranges are compared)
                      (dict(sel_ptr=fb[0]), "sel must not alias an input"),
                      (dict(mse_ptr=ua), "mse must not alias an input"), (dict(E_ptr=t[1]), "E must not alias an input"),
                      (dict(sel_ptr=out), "sel must not alias out"), (dict(mse_ptr=out), "mse must not alias out"),
                      (dict(sel_ptr=sel, mse_ptr=sel), "mse must not alias sel"), (dict(E_ptr=out), "E must not alias out"),
                      (dict(mse_ptr=mse, E_ptr=mse), "E must not alias mse"), (dict(sel_ptr=E, E_ptr=E), "E must not alias sel")):
        with pytest.raises(G.GdptError, match=match):
            dev(**kw)
    with pytest.raises(G.GdptError, match="one address per candidate"):
        dev(fa=[0x1000])
    # the array arguments themselves
    L = G.lib()
    arr = (C.c_void_p * 2)(0x1000, 0x2000)
    for args, match in (((None, arr, arr), "FA is null"), ((arr, None, arr), "FB is null"), ((arr, arr, None), "T is null")):
        assert L.gdpt_filter_select_device(4, 3, 2, *args, ua, va, ub, vb, None, out, None, None, None, None, None) != 0
        assert match in L.gdpt_last_error().decode()
    # the host entry refuses the same
    f = np.ones((3, 4, 3))
    for kw, match in ((dict(radius=9), "radius"), (dict(params=bad_p), "reserved")):
        with pytest.raises(G.GdptError, match=match):
            G.filter_select([f, f], [f, f], [f, f], f, 0.01 * f, f, 0.01 * f, **kw)
    with pytest.raises(G.GdptError, match="n must be in"):
        G.filter_select([f] * 9, [f] * 9, [f] * 9, f, f, f, f)
    with pytest.raises(G.GdptError, match="one image per candidate"):
        G.filter_select([f], [f, f], [f, f], f, f, f, f)
    with pytest.raises(G.GdptError, match="one shape"):
        G.filter_select([f], [f], [np.ones((3, 5, 3))], f, f, f, f)
    with pytest.raises(G.GdptError, match="one shape"):
        G.filter_select([f], [f], [f], f, np.ones((3, 4)), f, f)


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.filter_select([f, f], [f, f], [f, f], f, 0.01 * f, f, 0.01 * f)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.filter_select_device(4, 3, [0x1000], [0x2000], [0x3000], 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, radius=0)


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
GROUP = ["--pass-spp", "4", "--sample-devices", "0,0", "--denoised", "d.pfm"]
NOT_COMBINED = "--select is not combined with"
CLI_ERRORS = [(["--select", "mean,atrous"], "--select needs --denoised"),
              (["--denoised", "d.pfm", "--select", "mean"], "--denoised needs --pass-spp"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--select", "mean,atrous"], "--select needs --sample-devices with two or more entries"),
              (["--pass-spp", "4", "--sample-devices", "0", "--denoised", "d.pfm", "--select", "mean,atrous"], "--select needs --sample-devices with two or more entries"),
              ([*GROUP, "--select", "mean,median"], "--select takes mean, nlm, guided, demod, regress, atrous and atrous-demod, each once"),
              ([*GROUP, "--select", "atrous,atrous"], "each once"), ([*GROUP, "--select", "mean,"], "each once"),
              ([*GROUP, "--select", "mean,nlm,guided,demod,regress,atrous,atrous-demod,mean"], "each once"),
              ([*GROUP, "--select", "mean,nlm", "--nlm-k", "1.0"], NOT_COMBINED), ([*GROUP, "--select", "mean,nlm", "--nlm-window", "4"], NOT_COMBINED),
              ([*GROUP, "--select", "mean,guided", "--nlm-guide", "normal"], NOT_COMBINED), ([*GROUP, "--select", "mean,demod", "--nlm-demodulate"], NOT_COMBINED),
              ([*GROUP, "--select", "mean,nlm", "--nlm-levels", "2"], NOT_COMBINED), ([*GROUP, "--select", "mean,regress", "--nlm-regress", "albedo"], NOT_COMBINED),
              ([*GROUP, "--select", "mean,regress", "--nlm-ridge", "0.1"], NOT_COMBINED), ([*GROUP, "--select", "mean,atrous", "--atrous-levels", "3"], NOT_COMBINED),
              ([*GROUP, "--select", "mean,atrous", "--atrous-k", "1.0"], NOT_COMBINED),
              ([*GROUP, "--select", "mean,atrous", "--select-radius", "9"], "--select-radius takes a radius from 0 to 8"),
              ([*GROUP, "--select", "mean,atrous", "--select-radius", "-1"], "--select-radius takes a radius from 0 to 8"),
              ([*GROUP, "--select", "mean,guided", "--nlm-kf", "-1"], "--nlm-kf must be > 0"),
              ([*GROUP, "--select", "mean,guided", "--nlm-depth-tau", "-1"], "--nlm-depth-tau must be > 0"),
              ([*GROUP, "--select", "mean,demod", "--nlm-albedo-floor", "-1"], "--nlm-albedo-floor must be > 0"),
              ([*GROUP, "--select", "mean,nlm", "--nlm-var-smooth", "5"], "--nlm-var-smooth takes a radius from 0 to 4"),
              ([*GROUP, "--select-radius", "2"], "--select-radius, --select-map and --select-mse need --select"),
              ([*GROUP, "--select-map", "m.pfm"], "need --select"), ([*GROUP, "--select-mse", "e.pfm"], "need --select"),
              # without --select the flags it takes over keep their own rules
              ([*GROUP, "--nlm-kf", "0.5"], "--nlm-depth-tau and --nlm-kf need --nlm-guide"), ([*GROUP, "--nlm-albedo-floor", "0.01"], "--nlm-albedo-floor needs --nlm-demodulate")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.pfm", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
