"""The host side of the collaborative form of the first-order feature regression (include/gdpt.h: gdpt_denoise_nlm_collab*), without a
GPU: the header's prototypes and the blocks' layout against the Python mirror, the export of the entry points, the refusals, which
come before any device call and name their field (the regression's, and a coefficient film that overlaps an input or out), the
session entry's, and the argument errors of the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from test_nlm_regress_host import REFUSED

EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_the_header_declares_the_entries_and_the_blocks_match(G, tmp_path):
    proto, src = tmp_path / "proto.c", tmp_path / "sz.c"
    proto.write_text(f'#include "{ROOT}/include/gdpt.h"\n'
                   'typedef int (*dev_t)(int, int, const double *, const double *, const double *, const double *, const GdptNlmParams *, '
                   'const GdptNlmGuide *, const GdptNlmRegress *, double *, double *, void *, GdptNlmStats *);\n'
                   'typedef int (*host_t)(int, int, const double *, const double *, const double *, const double *, const GdptNlmParams *, '
                   'const GdptNlmGuide *, const GdptNlmRegress *, double *, double *, GdptNlmStats *);\n'
                   'typedef int (*ses_t)(GdptProgressive *, const GdptNlmParams *, const GdptNlmGuide *, const GdptNlmRegress *, int, int, '
                   'double *, double *, double *, GdptNlmStats *);\n'
                   'dev_t a = gdpt_denoise_nlm_collab_device; host_t b = gdpt_denoise_nlm_collab; ses_t c = gdpt_progressive_denoise_collab;\n')
    # the prototypes are what the Python mirror passes (a mismatch is an error of the compiler's)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "proto.o"), str(proto)])
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(GdptNlmRegress), sizeof(GdptNlmStats), offsetof(GdptNlmStats, sum_var_out), '
                   'offsetof(GdptNlmStats, error_out)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    regress, stats, var_out, error_out = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    S = G.GdptNlmStats
    assert (regress, stats, var_out, error_out) == (C.sizeof(G.GdptNlmRegress), C.sizeof(S), S.sum_var_out.offset, S.error_out.offset)


def test_the_library_exports_the_entry_points(G):
    lib = C.CDLL(G.library_path())
    for name in ("gdpt_denoise_nlm_collab_device", "gdpt_denoise_nlm_collab", "gdpt_progressive_denoise_collab"):
        assert hasattr(lib, name), name
    for name in ("denoise_nlm_collab", "denoise_nlm_collab_device"):
        assert callable(getattr(G, name)), name
    assert callable(G.Progressive.denoise_collab)


@pytest.mark.parametrize("channels,block,match", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_blocks_name_their_field(G, channels, block, match):
    """The regression's blocks (tests/test_nlm_regress_host.py), refused by the same checks."""
    a, b, c, d, e = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000      # never dereferenced: every call below is refused on the host
    guide = G.nlm_guide(num_channels=channels, groups=[(0, 3, 1e-3)])
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm_collab_device(4, 3, a, b, c, d, e, guide=guide, regress=block(G))
    f, p = np.ones((3, 4, 3)), np.ones((channels, 3, 4))
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm_collab(f, 0.01 * f, p, 0.0 * p, guide=guide, regress=block(G))


def test_refused_arguments_name_their_field(G):
    a, b, c, d, e, g = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    dev = G.denoise_nlm_collab_device
    none, one = G.nlm_guide(groups=[]), G.nlm_regress(channels=[6])
    for args, kw, match in (((4, 3, a, b, 0, d, e), {}, "feat is null"), ((4, 3, a, b, c, 0, e), {}, "feat_var is null"),
                            ((4, 3, a, b, 0, d, e), dict(guide=none, regress=one), "feat is null"),      # (no group: a regressor needs the planes)
                            ((4, 3, a, b, c, 0, e), dict(guide=none, regress=one), "feat_var is null"),
                            ((4, 3, a, b, 0, d, e), dict(regress=G.nlm_regress(channels=[])), "feat is null"),      # (no regressor: a group does)
                            # everything the guided entry refuses
                            ((4, 3, 0, b, c, d, e), {}, "img"), ((4, 3, a, 0, c, d, e), {}, "var is null"), ((4, 3, a, b, c, d, 0), {}, "out is null"),
                            ((4, 3, a, b, c, d, a), {}, "out must not alias"), ((4, 3, a, b, c, d, c), {}, "out must not alias"),
                            ((4, 3, a, b, c, d, d), {}, "out must not alias"),
                            ((0, 3, a, b, c, d, e), {}, "width"), ((4, 0, a, b, c, d, e), {}, "height"),
                            ((4, 3, a, b, c, d, e), dict(window_radius=11), "window_radius"), ((4, 3, a, b, c, d, e), dict(patch_radius=4), "patch_radius"),
                            ((4, 3, a, b, c, d, e), dict(k=0.0), "k must be"), ((4, 3, a, b, c, d, e), dict(epsilon=0.0), "epsilon"),
                            ((4, 3, a, b, c, d, e), dict(guide=G.nlm_guide(k_f=0.0)), "k_f"),
                            ((4, 3, a, b, c, d, e), dict(guide=G.nlm_guide(alpha_f=-1.0)), "alpha_f"),
                            ((4, 3, a, b, c, d, e), dict(guide=G.nlm_guide(num_channels=17)), "num_channels"),
                            ((4, 3, a, b, c, d, e), dict(guide=G.nlm_guide(groups=[(0, 3, 0.0)])), "tau"),
                            ((4, 3, a, b, c, d, e), dict(guide=G.nlm_guide(groups=[(6, 3, 1e-3)])), "first_channel")):
        with pytest.raises(G.GdptError, match=match):
            dev(*args, **kw)
    # The coefficient film: 3 (1 + 6) planes of 12 doubles = 2016 bytes at the default block; img, var and out are 288 bytes, the
    # feature films 8 planes = 768 bytes. Any shared byte is refused, whichever side the film starts on.
    for coef in (a, b, c, d, e, a + 280, e + 280, c + 760, d + 760, a - 2008, e - 2008, c - 8):
        with pytest.raises(G.GdptError, match="coef must not overlap"):
            dev(4, 3, a, b, c, d, e, coef_ptr=coef)
    # ... and a film that only touches is past the argument checks: without a device, that is the next refusal
    import torch
    if not torch.cuda.is_available():
        for coef in (a + 288, e + 288, c + 768, a - 2016, g):
            with pytest.raises(G.GdptError, match="no HIP device"):
                dev(4, 3, a, b, c, d, e, coef_ptr=coef)
    # with fewer regressors the film is smaller: 3 planes at m = 0
    with pytest.raises(G.GdptError, match="coef must not overlap"):
        dev(4, 3, a, b, c, d, e, coef_ptr=a - 280, regress=G.nlm_regress(channels=[]))
    bad = G.nlm_regress()
    bad.reserved[1] = 1
    with pytest.raises(G.GdptError, match="regress reserved"):
        dev(4, 3, a, b, c, d, e, coef_ptr=g, regress=bad)
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="regress reserved"):
        G.denoise_nlm_collab(f, 0.01 * f, p, 0.0 * p, regress=bad)
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_collab(f, 0.01 * f, np.ones((8, 3, 5)), np.ones((8, 3, 5)))
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_collab(f, np.ones((3, 5, 3)), p, p)


def test_the_session_entry_refuses_a_null_session(G):
    assert G.lib().gdpt_progressive_denoise_collab(None, None, None, None, 4, 0, None, None, None, None) != 0
    assert b"gdpt_progressive_denoise_collab: null session" in G.lib().gdpt_last_error()


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_collab(f, 0.01 * f, p, 0.0 * p, coef=True)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_collab_device(4, 3, 0x1000, 0x2000, 0, 0, 0x5000, guide=G.nlm_guide(groups=[]), regress=G.nlm_regress(channels=[]))


BASE = ["--pass-spp", "4", "--denoised", "d.pfm"]
REGRESS = ["--nlm-regress", "albedo,normal"]
CLI_ERRORS = [([*BASE, "--nlm-collaborative"], "--nlm-collaborative needs --nlm-regress"),
              (["--nlm-collaborative"], "--nlm-collaborative needs --nlm-regress"),
              ([*BASE, "--nlm-collaborative", "--nlm-guide", "albedo,normal"], "--nlm-collaborative needs --nlm-regress"),
              ([*BASE, "--nlm-collaborative", "--nlm-ridge", "0.1"], "--nlm-collaborative needs --nlm-regress"),
              # everything --nlm-regress refuses beside it
              ([*REGRESS, "--nlm-collaborative"], "--nlm-regress needs --denoised"),
              ([*BASE, "--nlm-collaborative", "--nlm-regress", "albedo,depth"], "--nlm-depth-scale"),
              ([*BASE, "--nlm-collaborative", "--nlm-regress", "albedo,colour"], "albedo, normal and depth"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--nlm-ridge", "-1"], "--nlm-ridge must be > 0"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--nlm-demodulate"], "not combined with --nlm-demodulate, --nlm-var-smooth or --nlm-levels"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--nlm-var-smooth", "1"], "not combined with --nlm-demodulate, --nlm-var-smooth or --nlm-levels"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--nlm-levels", "2"], "not combined with --nlm-demodulate, --nlm-var-smooth or --nlm-levels"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--nlm-joint"], "--nlm-joint is not combined with"),
              ([*BASE, *REGRESS, "--nlm-collaborative", "--atrous-levels", "3"], "--atrous-levels is not combined with"),
              (["--denoised", "d.pfm", *REGRESS, "--nlm-collaborative"], "--denoised needs --pass-spp")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.pfm", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
