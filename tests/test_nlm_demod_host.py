"""The host side of the albedo-demodulated non-local-means filter (include/gdpt.h: gdpt_denoise_nlm_demod*), without a GPU: the
struct layout of the Python mirror against the header, the documented defaults, the refusals, which come before any device call and
name their field, and the argument errors of the CLI."""
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
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(GdptNlmDemod), offsetof(GdptNlmDemod, coverage_channel), '
                   'offsetof(GdptNlmDemod, floor), offsetof(GdptNlmDemod, reserved)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    size, cov, floor, reserved = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    D = G.GdptNlmDemod
    assert (size, cov, floor, reserved) == (C.sizeof(D), D.coverage_channel.offset, D.floor.offset, D.reserved.offset) == (24, 4, 8, 16)


def test_default_demod(G):
    d = G.GdptNlmDemod(5, 5, 0.5, (C.c_int32 * 2)(7, 7))
    G.lib().gdpt_nlm_default_demod(C.byref(d))
    assert (d.albedo_channel, d.coverage_channel, d.floor, list(d.reserved)) == (0, 7, 1e-3, [0, 0])
    q = G.nlm_demod(albedo_channel=2, coverage_channel=-1, floor=0.01)
    assert (q.albedo_channel, q.coverage_channel, q.floor, list(q.reserved)) == (2, -1, 0.01, [0, 0])
    q = G.nlm_demod(floor=0.5)
    assert (q.albedo_channel, q.coverage_channel, q.floor) == (0, 7, 0.5)
    G.lib().gdpt_nlm_default_demod(None)          # a null block is ignored


# (number of planes, keywords of nlm_demod, what the message names)
REFUSED = [(8, dict(albedo_channel=-1), "albedo_channel"), (8, dict(albedo_channel=6, coverage_channel=-1), "albedo_channel"),
           (5, dict(albedo_channel=3, coverage_channel=-1), "albedo_channel"), (2, dict(coverage_channel=-1), "albedo_channel"),
           (8, dict(coverage_channel=-2), "coverage_channel"), (8, dict(coverage_channel=8), "coverage_channel"),
           (7, dict(), "coverage_channel"),                    # the default block's plane 7 on seven planes
           (8, dict(coverage_channel=0), "coverage_channel"), (8, dict(coverage_channel=2), "coverage_channel"),
           (8, dict(albedo_channel=4, coverage_channel=5), "coverage_channel"),
           (8, dict(floor=0.0), "floor"), (8, dict(floor=-1e-3), "floor"), (8, dict(floor=np.nan), "floor"), (8, dict(floor=np.inf), "floor"),
           (17, dict(), "num_channels"), (-1, dict(), "num_channels")]


@pytest.mark.parametrize("channels,kw,match", REFUSED, ids=[f"{n}-" + "-".join(f"{k}={v}" for k, v in kw.items()) for n, kw, _ in REFUSED])
def test_refused_blocks_name_their_field(G, channels, kw, match):
    a, b, c, d, e = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000      # never dereferenced: every call below is refused on the host
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm_demod_device(4, 3, a, b, c, d, channels, e, demod=G.nlm_demod(**kw))
    if channels >= 1:
        f, p = np.ones((3, 4, 3)), np.ones((channels, 3, 4))
        with pytest.raises(G.GdptError, match=match):
            G.denoise_nlm_demod(f, 0.01 * f, p, 0.0 * p, demod=G.nlm_demod(**kw))


def test_refused_arguments_name_their_field(G):
    a, b, c, d, e, g = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    dev = G.denoise_nlm_demod_device
    ok = G.nlm_demod(coverage_channel=-1)
    for args, kw, match in (((4, 3, a, b, 0, d, 8, e), {}, "feat is null"), ((4, 3, a, b, c, 0, 8, e), {}, "feat_var is null"),
                            ((4, 3, a, b, 0, d, 3, e), dict(demod=ok), "feat is null"),          # (no guide: the planes are needed all the same)
                            ((4, 3, 0, b, c, d, 8, e), {}, "img"), ((4, 3, a, b, c, d, 8, 0), {}, "out is null"),
                            ((4, 3, a, b, c, d, 8, c), {}, "out must not alias"), ((4, 3, a, b, c, d, 8, d), {}, "out must not alias"),
                            ((4, 3, a, b, c, d, 8, e), dict(var_out_ptr=c), "var_out must not alias"),
                            ((4, 3, a, b, c, d, 8, e), dict(var_out_ptr=d), "var_out must not alias"),
                            ((0, 3, a, b, c, d, 8, e), {}, "width"), ((4, 3, a, b, c, d, 8, e), dict(window_radius=11), "window_radius"),
                            # a guide is checked as the guided entry checks it, and must speak of the same planes
                            ((4, 3, a, b, c, d, 8, e), dict(guide=G.nlm_guide(k_f=0.0)), "k_f"),
                            ((4, 3, a, b, c, d, 8, e), dict(guide=G.nlm_guide(num_channels=7, groups=[(3, 3, 1e-3)])), "num_channels"),
                            ((4, 3, a, b, c, d, 8, e), dict(guide=G.nlm_guide(groups=[(6, 3, 1e-3)])), "first_channel")):
        with pytest.raises(G.GdptError, match=match):
            dev(*args, **kw)
    bad = G.nlm_demod()
    bad.reserved[1] = 1
    with pytest.raises(G.GdptError, match="reserved"):
        dev(4, 3, a, b, c, d, 8, e, var_out_ptr=g, demod=bad)
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="reserved"):
        G.denoise_nlm_demod(f, 0.01 * f, p, 0.0 * p, demod=bad)
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_demod(f, 0.01 * f, np.ones((8, 3, 5)), np.ones((8, 3, 5)))
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_demod(f, np.ones((3, 5, 3)), p, p)
    assert G.lib().gdpt_progressive_denoise_demod(None, None, None, None, 4, 0, None, None, None, None, None) != 0
    assert b"null session" in G.lib().gdpt_last_error()


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f, p = np.ones((3, 4, 3)), np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_demod(f, 0.01 * f, p, 0.0 * p)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_demod_device(4, 3, 0x1000, 0x2000, 0x3000, 0x4000, 8, 0x5000, guide=G.nlm_guide(groups=[(3, 3, 1e-3)]))


CLI_ERRORS = [(["--nlm-demodulate"], "--nlm-demodulate needs --denoised"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-demodulate", "--nlm-guide", "albedo,normal"], "the albedo is already divided out"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-demodulate", "--nlm-guide", "normal,albedo"], "--nlm-guide albedo"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-albedo-floor", "0.01"], "--nlm-albedo-floor needs --nlm-demodulate"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-demodulate", "--nlm-albedo-floor", "-0.5"], "--nlm-albedo-floor must be > 0"),
              (["--denoised", "d.pfm", "--nlm-demodulate"], "--denoised needs --pass-spp"),
              (["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-demodulate", "--nlm-guide", "normal,depth"], "--nlm-depth-tau")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.pfm", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
