"""The host side of the feature render and the guided filter (include/gdpt.h: gdpt_features_render*, gdpt_denoise_nlm_guided*),
without a GPU: the struct layouts of the Python mirror against the header, the documented defaults, and the refusals, which come
before any device call (and before a handle or an address is looked at) and name their field."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import ROOT

A, B, F, FV, O, VO, SCENE = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000     # never dereferenced


def test_struct_layouts_match_the_header(G, tmp_path):
    structs = {"GdptNlmFeatureGroup": G.GdptNlmFeatureGroup, "GdptNlmGuide": G.GdptNlmGuide}
    lines = ['printf("channels %d %d %d\\n", GDPT_FEATURE_CHANNELS, GDPT_NLM_MAX_GROUPS, GDPT_NLM_MAX_CHANNELS);']
    for name, s in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in s._fields_:
            lines.append(f'printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{" ".join(lines)} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    seen = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *vals = line.split()
        seen[key] = [int(v) for v in vals]
    assert seen["channels"] == [G.FEATURE_CHANNELS, G.NLM_MAX_GROUPS, G.NLM_MAX_CHANNELS] == [8, 4, 16]
    for name, s in structs.items():
        assert seen[name] == [C.sizeof(s)], name
        for field, _ in s._fields_:
            assert seen[f"{name}.{field}"] == [getattr(s, field).offset], (name, field)
    assert C.sizeof(G.GdptNlmFeatureGroup) == 16 and C.sizeof(G.GdptNlmGuide) == 8 + 4 * 16 + 16 + 8


def test_default_guide(G):
    g = G.GdptNlmGuide()
    C.memset(C.byref(g), 0x5A, C.sizeof(g))
    G.lib().gdpt_nlm_default_guide(C.byref(g))
    assert (g.num_channels, g.num_groups, g.k_f, g.alpha_f, list(g.reserved)) == (8, 2, 0.6, 1.0, [0, 0])
    assert [(q.first_channel, q.num_channels, q.tau) for q in g.groups] == [(0, 3, 1e-3), (3, 3, 1e-3), (0, 0, 0.0), (0, 0, 0.0)]
    h = G.nlm_guide(groups=[(0, 3, 1e-3), (3, 3, 1e-3), (6, 1, 0.25)], k_f=0.8)
    assert (h.num_channels, h.num_groups, h.k_f, h.alpha_f) == (8, 3, 0.8, 1.0)
    assert (h.groups[2].first_channel, h.groups[2].num_channels, h.groups[2].tau) == (6, 1, 0.25)
    assert G.nlm_guide(groups=[]).num_groups == 0
    with pytest.raises(G.GdptError, match="at most 4"):
        G.nlm_guide(groups=[(0, 1, 1.0)] * 5)
    G.lib().gdpt_nlm_default_guide(None)           # a null block is ignored


def guide_with(G, **kw):
    reserved = kw.pop("reserved", None)
    ngroups = kw.pop("num_groups", None)
    g = G.nlm_guide(**kw)
    if reserved is not None:
        g.reserved[reserved] = 1
    if ngroups is not None:
        g.num_groups = ngroups
    return g


NAN, INF = float("nan"), float("inf")
REFUSED_GUIDES = [
    (dict(num_groups=-1), "num_groups"), (dict(num_groups=5), "num_groups"),
    (dict(num_channels=-1), "num_channels"), (dict(num_channels=17, groups=[]), "num_channels"),
    (dict(groups=[(0, 0, 1e-3)]), r"groups\[0\]\.num_channels"), (dict(groups=[(0, 3, 1e-3), (2, -1, 1e-3)]), r"groups\[1\]\.num_channels"),
    (dict(groups=[(-1, 2, 1e-3)]), r"groups\[0\]\.first_channel"), (dict(groups=[(6, 3, 1e-3)]), r"groups\[0\]\.first_channel"),
    (dict(num_channels=3, groups=[(0, 3, 1e-3), (3, 1, 1e-3)]), r"groups\[1\]\.first_channel"),
    (dict(groups=[(0, 3, 0.0)]), r"groups\[0\]\.tau"), (dict(groups=[(0, 3, -1e-3)]), "tau"), (dict(groups=[(0, 3, NAN)]), "tau"),
    (dict(groups=[(0, 3, 1e-3), (3, 3, INF)]), r"groups\[1\]\.tau"),
    (dict(k_f=0.0), "k_f"), (dict(k_f=-0.6), "k_f"), (dict(k_f=NAN), "k_f"), (dict(k_f=INF), "k_f"),
    (dict(alpha_f=-1.0), "alpha_f"), (dict(alpha_f=NAN), "alpha_f"), (dict(alpha_f=INF), "alpha_f"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"),
]


@pytest.mark.parametrize("kw,match", REFUSED_GUIDES, ids=[f"{n}-{list(kw)[-1]}" for n, (kw, _) in enumerate(REFUSED_GUIDES)])
def test_refused_guides_name_their_field(G, kw, match):
    g = guide_with(G, **dict(kw))
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm_guided_device(4, 3, A, B, F, FV, O, guide=g)
    f = np.ones((3, 4, 3))
    planes = np.ones((max(g.num_channels, 0), 3, 4))
    out = np.empty_like(f)
    rc = G.lib().gdpt_denoise_nlm_guided(4, 3, f.ctypes.data, f.ctypes.data, planes.ctypes.data, planes.ctypes.data, None, C.byref(g),
                                         out.ctypes.data, None, None)
    assert rc != 0
    import re
    assert re.search(match, G.lib().gdpt_last_error().decode())
    assert G.lib().gdpt_progressive_denoise_guided(SCENE, None, C.byref(g), 4, 0, O, None, None, None, None) != 0
    assert re.search(match, G.lib().gdpt_last_error().decode())


def test_refused_guided_arguments_name_their_field(G):
    dev = G.denoise_nlm_guided_device
    for args, kw, match in (((4, 3, 0, B, F, FV, O), {}, "img"), ((4, 3, A, 0, F, FV, O), {}, "var is null"), ((4, 3, A, B, F, FV, 0), {}, "out is null"),
                            ((4, 3, A, B, 0, FV, O), {}, "feat is null"), ((4, 3, A, B, F, 0, O), {}, "feat_var is null"),
                            ((4, 3, A, B, F, FV, A), {}, "out must not alias"), ((4, 3, A, B, F, FV, B), {}, "out must not alias"),
                            ((4, 3, A, B, F, FV, F), {}, "out must not alias"), ((4, 3, A, B, F, FV, FV), {}, "out must not alias"),
                            ((4, 3, A, B, F, FV, O), dict(var_out_ptr=A), "var_out must not alias"), ((4, 3, A, B, F, FV, O), dict(var_out_ptr=O), "var_out must not alias"),
                            ((4, 3, A, B, F, FV, O), dict(var_out_ptr=F), "var_out must not alias"), ((4, 3, A, B, F, FV, O), dict(var_out_ptr=FV), "var_out must not alias"),
                            ((0, 3, A, B, F, FV, O), {}, "width"), ((4, 0, A, B, F, FV, O), {}, "height"),
                            ((4, 3, A, B, F, FV, O), dict(window_radius=11), "window_radius"), ((4, 3, A, B, F, FV, O), dict(k=0.0), "k must")):
        with pytest.raises(G.GdptError, match=match):
            dev(*args, **kw)
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_guided(np.ones((3, 4, 3)), np.ones((3, 4, 3)), np.ones((8, 3, 5)), np.ones((8, 3, 5)))
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm_guided(np.ones((3, 4, 3)), np.ones((3, 4, 3)), np.ones((6, 3, 4)), np.ones((6, 3, 4)))
    lib = G.lib()
    assert lib.gdpt_progressive_denoise_guided(None, None, None, 4, 0, O, None, None, None, None) != 0 and b"session" in lib.gdpt_last_error()
    assert lib.gdpt_progressive_denoise_guided(SCENE, None, None, 4, 0, None, None, None, None, None) != 0 and b"out is null" in lib.gdpt_last_error()
    g = G.nlm_guide(num_channels=6, groups=[(0, 3, 1e-3)])
    assert lib.gdpt_progressive_denoise_guided(SCENE, None, C.byref(g), 4, 0, O, None, None, None, None) != 0
    assert b"num_channels must be GDPT_FEATURE_CHANNELS" in lib.gdpt_last_error()


def features_call(G, params=None, window=None, scene=SCENE, mean=A, var=B, host=False):
    p = G.GdptRenderParams(4, G.RNG_SAMPLE, 0, 0, 0, 0, 0, 0)
    for k, v in (params or {}).items():
        setattr(p, k, v)
    win = G.GdptSampleWindow(*window) if window is not None else None
    opt = lambda x: C.c_void_p(x) if x else None      # noqa: E731
    args = [opt(scene), C.byref(p), C.byref(win) if win is not None else None, opt(mean), opt(var)]
    if host:
        return G.lib().gdpt_features_render(*args, None)
    return G.lib().gdpt_features_render_device(*args, None, None)


REFUSED_FEATURES = [
    (dict(scene=0), "scene is null"), (dict(mean=0), "mean is null"), (dict(var=0), "var is null"), (dict(var=A), "must not alias"),
    (dict(params=dict(rng_scheme=0)), "rng_scheme: GDPT_RNG_TILE"), (dict(params=dict(rng_scheme=1)), "rng_scheme"),
    (dict(params=dict(shift_mode=1)), "shift_mode"), (dict(params=dict(reserved=1)), "reserved"),
    (dict(params=dict(row_begin=-1, row_end=4)), "row_begin"), (dict(params=dict(row_begin=4, row_end=4)), "row_begin"),
    (dict(params=dict(row_begin=5, row_end=2)), "row_begin"),
    (dict(window=(0, 0)), "stream_spp"), (dict(window=(-4, 0)), "stream_spp"), (dict(window=(8, -1)), "first_sample"),
    (dict(window=(8, 5)), "first_sample"), (dict(window=(3, 0)), "stream_spp"),
]


@pytest.mark.parametrize("kw,match", REFUSED_FEATURES, ids=[f"{n}-{m.split()[0].rstrip(':')}" for n, (_, m) in enumerate(REFUSED_FEATURES)])
def test_refused_feature_renders_name_their_field(G, kw, match):
    """Each is refused on the values of the arguments alone: the scene handle below is an address that is never read."""
    for host in (False, True):
        assert features_call(G, host=host, **kw) != 0
        assert match in G.lib().gdpt_last_error().decode(), G.lib().gdpt_last_error()


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f = np.ones((3, 4, 3))
    planes = np.ones((8, 3, 4))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_guided(f, 0.01 * f, planes, 0.01 * planes)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_guided_device(4, 3, A, B, F, FV, O, var_out_ptr=VO)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_guided_device(4, 3, A, B, 0, 0, O, guide=G.nlm_guide(groups=[]))       # no group: no feature planes needed
    for host in (False, True):          # (a handle can only come from a device: the device is asked for before the handle is read)
        assert features_call(G, host=host, window=(8, 2)) != 0
        assert b"no HIP device" in G.lib().gdpt_last_error()
