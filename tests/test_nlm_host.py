"""The host side of the non-local-means filter (include/gdpt.h: gdpt_denoise_nlm*), without a GPU: the struct layouts of the Python
mirror against the header, the documented defaults, and the refusals, which come before any device call and name their field."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import ROOT


def test_struct_layouts_match_the_header(G, tmp_path):
    structs = ["GdptNlmParams", "GdptNlmStats"]
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    sizes = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in structs:
        assert int(sizes[s]) == C.sizeof(getattr(G, s)), s


def test_default_params(G):
    p = G.GdptNlmParams(1, 1, 1.0, 5.0, 1.0, (C.c_int32 * 2)(7, 7))
    G.lib().gdpt_nlm_default_params(C.byref(p))
    assert (p.window_radius, p.patch_radius, p.k, p.alpha, p.epsilon, list(p.reserved)) == (10, 3, 0.45, 1.0, 1e-10, [0, 0])
    q = G.nlm_params(window_radius=4, k=0.7)
    assert (q.window_radius, q.patch_radius, q.k, q.alpha, q.epsilon) == (4, 3, 0.7, 1.0, 1e-10)
    G.lib().gdpt_nlm_default_params(None)          # a null block is ignored


REFUSED = [(dict(window_radius=-1), "window_radius"), (dict(window_radius=11), "window_radius"),
           (dict(patch_radius=-1), "patch_radius"), (dict(patch_radius=4), "patch_radius"),
           (dict(k=0.0), "k must"), (dict(k=-0.5), "k must"), (dict(k=np.nan), "k must"), (dict(k=np.inf), "k must"),
           (dict(alpha=-1.0), "alpha"), (dict(alpha=np.nan), "alpha"), (dict(alpha=np.inf), "alpha"),
           (dict(epsilon=0.0), "epsilon"), (dict(epsilon=-1e-10), "epsilon"), (dict(epsilon=np.nan), "epsilon"), (dict(epsilon=np.inf), "epsilon")]


@pytest.mark.parametrize("kw,match", REFUSED, ids=[f"{list(kw)[0]}={list(kw.values())[0]}" for kw, _ in REFUSED])
def test_refused_parameters_name_their_field(G, kw, match):
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm(f, f.copy(), **kw)
    with pytest.raises(G.GdptError, match=match):
        G.denoise_nlm_device(4, 3, 0x1000, 0x2000, 0x3000, **kw)      # (refused before an address is looked at)


def test_refused_arguments_name_their_field(G):
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000      # never dereferenced: every call below is refused on the host
    dev = G.denoise_nlm_device
    for args, kw, match in (((4, 3, 0, b, c), {}, "img"), ((4, 3, a, 0, c), {}, "var is null"), ((4, 3, a, b, 0), {}, "out is null"),
                            ((4, 3, a, b, a), {}, "out must not alias"), ((4, 3, a, b, b), {}, "out must not alias"),
                            ((4, 3, a, b, c), dict(var_out_ptr=a), "var_out must not alias"), ((4, 3, a, b, c), dict(var_out_ptr=b), "var_out must not alias"),
                            ((4, 3, a, b, c), dict(var_out_ptr=c), "var_out must not alias"),
                            ((0, 3, a, b, c), {}, "width"), ((4, 0, a, b, c), {}, "height"), ((-1, 3, a, b, c), {}, "width")):
        with pytest.raises(G.GdptError, match=match):
            dev(*args, **kw)
    p = G.nlm_params()
    p.reserved[1] = 1
    with pytest.raises(G.GdptError, match="reserved"):
        dev(4, 3, a, b, c, var_out_ptr=d, params=p)
    f = np.ones((3, 4, 3))
    out = np.empty_like(f)
    rc = G.lib().gdpt_denoise_nlm(4, 3, f.ctypes.data, f.ctypes.data, C.byref(p), out.ctypes.data, None, None)
    assert rc != 0 and b"reserved" in G.lib().gdpt_last_error()
    with pytest.raises(G.GdptError, match="one shape"):
        G.denoise_nlm(f, np.ones((3, 5, 3)))
    assert G.lib().gdpt_progressive_denoise(None, None, 0, None, None, None) != 0
    with pytest.raises(G.GdptError, match="unknown knob"):
        G.debug_knobs.set(nlm_directt=1)
    with G.debug_knobs(nlm_direct=1):
        pass
    G.debug_knobs.reset()


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm(f, 0.01 * f)
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.denoise_nlm_device(4, 3, 0x1000, 0x2000, 0x3000, var_out_ptr=0x4000)
