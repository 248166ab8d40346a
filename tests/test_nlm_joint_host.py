"""The host side of the joint non-local-means filter (include/gdpt.h: gdpt_denoise_nlm_joint*, gdpt_progressive_denoise_reconstruct),
without a GPU: the struct layout of the Python mirror against the header, the defaults, the refusals, which come before any device
call and name their field, and the argument errors of the CLI."""
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
                   'int main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(GdptNlmJointStats), sizeof(GdptNlmStats), offsetof(GdptNlmJointStats, guide), '
                   'offsetof(GdptNlmJointStats, sum_var_in), offsetof(GdptNlmJointStats, sum_var_out), GDPT_NLM_JOINT_MAX); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    size, inner, guide, var_in, var_out, cap = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    S = G.GdptNlmJointStats
    assert (size, inner, guide, var_in, var_out) == (C.sizeof(S), C.sizeof(G.GdptNlmStats), S.guide.offset, S.sum_var_in.offset, S.sum_var_out.offset) \
        == (136, 72, 0, 72, 104)
    assert cap == G.NLM_JOINT_MAX == 4


def test_the_library_exports_the_entry_points(G):
    lib = C.CDLL(G.library_path())
    for name in ("gdpt_denoise_nlm_joint_device", "gdpt_denoise_nlm_joint", "gdpt_progressive_denoise_reconstruct"):
        assert hasattr(lib, name), name


A, B, O, VO = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced: every call below is refused on the host
FT, FV = 0x50000, 0x60000
CP, CV, CO, CVO = [0x100000, 0x110000], [0x120000, 0x130000], [0x140000, 0x150000], [0x160000, 0x170000]


def dev(G, w=4, h=3, img=A, var=B, comp=CP, comp_var=CV, out=O, comp_out=CO, **kw):
    return G.denoise_nlm_joint_device(w, h, img, var, comp, comp_var, out, comp_out, **kw)


def test_defaults(G):
    """Without planes the builders' default is no feature term, with them the library's default guide; the parameters are the
    filter's. Valid arguments get as far as the device check (or, on a GPU machine, are not tried here)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    with pytest.raises(G.GdptError, match="no HIP device"):
        dev(G)
    with pytest.raises(G.GdptError, match="no HIP device"):
        dev(G, comp=[], comp_var=[], comp_out=[])                       # n = 0 is a call like any other
    with pytest.raises(G.GdptError, match="no HIP device"):
        dev(G, feat_ptr=FT, feat_var_ptr=FV, var_out_ptr=VO, comp_var_out_ptrs=[CVO[0], None])
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_joint(f, 0.01 * f, [f, f], [0.01 * f, 0.01 * f])


def test_raw_null_blocks_mean_the_defaults(G):
    """params == NULL and guide == NULL are the library's defaults: the default guide has two groups, so it asks for the planes."""
    tab = lambda ptrs: (C.c_void_p * 2)(*ptrs)      # noqa: E731
    rc = G.lib().gdpt_denoise_nlm_joint_device(4, 3, A, B, None, None, 2, tab(CP), tab(CV), None, None, O, None, tab(CO), None, None, None)
    assert rc != 0 and b"gdpt_denoise_nlm_joint_device: feat is null" in G.lib().gdpt_last_error()


def refusals(G):
    film = 4 * 3 * 3 * 8
    yield dict(img=0), "img is null"
    yield dict(var=0), "var is null"
    yield dict(out=0), "out is null"
    yield dict(w=0), "width"
    yield dict(h=0), "height"
    yield dict(comp=CP * 3, comp_var=CV * 3, comp_out=CO * 3), r"n must be in \[0, 4\]"
    yield dict(comp=[CP[0], 0]), r"comp\[1\] is null"
    yield dict(comp_var=[0, CV[1]]), r"comp_var\[0\] is null"
    yield dict(comp_out=[CO[0], 0]), r"comp_out\[1\] is null"
    # what the guided entry refuses in its blocks
    yield dict(window_radius=11), "window_radius"
    yield dict(patch_radius=4), "patch_radius"
    yield dict(k=0.0), "k must be"
    yield dict(alpha=-1.0), "alpha"
    yield dict(epsilon=0.0), "epsilon"
    yield dict(feat_ptr=FT), "feat_var is null"
    yield dict(feat_var_ptr=FV, guide=G.nlm_guide()), "feat is null"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(k_f=0.0)), "k_f"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(alpha_f=-1.0)), "alpha_f"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(num_channels=17)), "num_channels"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(groups=[(0, 3, 0.0)])), "tau"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(groups=[(6, 3, 1e-3)])), "first_channel"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, guide=G.nlm_guide(groups=[(0, 0, 1e-3)])), r"groups\[0\].num_channels"
    # byte ranges: every output against every input and every earlier output, partial overlaps included
    yield dict(out=A), r"out must not alias an input \(img\)"
    yield dict(out=B + film - 8), r"out must not alias an input \(var\)"
    yield dict(out=CP[1] - film + 8), r"out must not alias an input \(comp\[1\]\)"
    yield dict(var_out_ptr=CV[0]), r"var_out must not alias an input \(comp_var\[0\]\)"
    yield dict(var_out_ptr=O + 8), "var_out must not alias out"
    yield dict(comp_out=[A + 16, CO[1]]), r"comp_out\[0\] must not alias an input \(img\)"
    yield dict(comp_out=[CO[0], CO[0]]), r"comp_out\[1\] must not alias comp_out\[0\]"
    yield dict(comp_out=[CO[0], O]), r"comp_out\[1\] must not alias out"
    yield dict(comp_var_out_ptrs=[CVO[0], CP[0]]), r"comp_var_out\[1\] must not alias an input \(comp\[0\]\)"
    yield dict(comp_var_out_ptrs=[CVO[0], CVO[0] + film - 8]), r"comp_var_out\[1\] must not alias comp_var_out\[0\]"
    yield dict(comp_var_out_ptrs=[CO[1], None]), r"comp_out\[1\] must not alias comp_var_out\[0\]"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, out=FT + 4 * 3 * 8 * 8 - 8), r"out must not alias an input \(feat\)"
    yield dict(feat_ptr=FT, feat_var_ptr=FV, comp_out=[FV, CO[1]]), r"comp_out\[0\] must not alias an input \(feat_var\)"


def test_refused_arguments_name_their_field(G):
    for kw, match in refusals(G):
        with pytest.raises(G.GdptError, match=match):
            dev(G, **kw)
    bad = G.nlm_params()
    bad.reserved[0] = 1
    with pytest.raises(G.GdptError, match="reserved"):
        dev(G, params=bad)
    g = G.nlm_guide(groups=[])
    g.reserved[1] = 1
    with pytest.raises(G.GdptError, match="guide reserved"):
        dev(G, guide=g)
    tab = (C.c_void_p * 2)(*CP)
    assert G.lib().gdpt_denoise_nlm_joint_device(4, 3, A, B, None, None, 2, None, tab, None, C.byref(G.nlm_guide(groups=[])), O, None, tab, None, None, None) != 0
    assert b"comp is null" in G.lib().gdpt_last_error()
    assert G.lib().gdpt_denoise_nlm_joint_device(4, 3, A, B, None, None, -1, None, None, None, None, O, None, None, None, None, None) != 0
    assert b"n must be in [0, 4]" in G.lib().gdpt_last_error()


def test_host_entry_refusals(G):
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_joint(f, np.ones((3, 5, 3)), [], [])
    with pytest.raises(G.GdptError, match="one length"):
        G.denoise_nlm_joint(f, 0.01 * f, [f], [])
    with pytest.raises(G.GdptError, match="shaped like img"):
        G.denoise_nlm_joint(f, 0.01 * f, [np.ones((3, 5, 3))], [0.01 * f])
    with pytest.raises(G.GdptError, match=r"n must be in \[0, 4\]"):
        G.denoise_nlm_joint(f, 0.01 * f, [f] * 5, [0.01 * f] * 5)
    with pytest.raises(G.GdptError, match="window_radius"):
        G.denoise_nlm_joint(f, 0.01 * f, [f], [0.01 * f], window_radius=-1)


def test_session_entry_refusals(G):
    L = G.lib()
    tail = (None, None, None, None)
    assert L.gdpt_progressive_denoise_reconstruct(None, None, None, 0, None, 0.04, None, 0, None, *tail) != 0
    assert b"gdpt_progressive_denoise_reconstruct: null session" in L.gdpt_last_error()
    assert L.gdpt_progressive_denoise_reconstruct(0x1000, None, None, 0, None, 0.04, None, 0, None, *tail) != 0
    assert b"out is null" in L.gdpt_last_error()
    bad = G.nlm_params(window_radius=11)
    assert L.gdpt_progressive_denoise_reconstruct(0x1000, C.byref(bad), None, 0, None, 0.04, None, 0, 0x2000, *tail) != 0
    assert b"window_radius" in L.gdpt_last_error()
    g3 = G.nlm_guide(num_channels=3, groups=[(0, 3, 1e-3)])
    assert L.gdpt_progressive_denoise_reconstruct(0x1000, None, C.byref(g3), 4, None, 0.04, None, 0, 0x2000, *tail) != 0
    assert b"num_channels must be GDPT_FEATURE_CHANNELS" in L.gdpt_last_error()
    sp = G.var_smooth_params(5)
    assert L.gdpt_progressive_denoise_reconstruct(0x1000, None, None, 0, C.byref(sp), 0.04, None, 0, 0x2000, *tail) != 0
    assert b"radius" in L.gdpt_last_error()


BASE = ["--pass-spp", "4", "--denoised", "d.pfm", "--nlm-joint"]
CLI_ERRORS = [(["--pass-spp", "4", "--nlm-joint"], "--nlm-joint needs --denoised"),
              ([*BASE, "--nlm-demodulate"], "--nlm-joint is not combined with --nlm-demodulate, --nlm-regress, --nlm-levels, --atrous-levels or --select"),
              ([*BASE, "--nlm-regress", "albedo"], "--nlm-joint is not combined with"),
              ([*BASE, "--nlm-levels", "2"], "--nlm-joint is not combined with"),
              ([*BASE, "--atrous-levels", "3"], "--nlm-joint is not combined with"),
              ([*BASE, "--select", "mean,nlm"], "--nlm-joint is not combined with"),
              ([*BASE, "--gpus", "2"], "--nlm-joint is a single-device option"),
              ([*BASE, "--reconstruct", "l1"], "--nlm-joint is not combined with --reconstruct l1"),
              (["--denoised", "d.pfm", "--nlm-joint"], "--denoised needs --pass-spp")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.pfm", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)


def test_cli_refuses_a_path_scene(tmp_path):
    """--nlm-joint on an Integrator::Path scene ends with status 2 once the scene is parsed, before any device is touched."""
    from helpers import scene_variant
    xml = scene_variant(str(tmp_path), "cbox/cbox_gdpt.xml", width=8, height=8, integrator="path")
    r = subprocess.run([EXE, *BASE, "-o", str(tmp_path / "o.pfm"), xml], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2 and "--nlm-joint needs a GradPath scene" in r.stderr, (r.returncode, r.stderr)
