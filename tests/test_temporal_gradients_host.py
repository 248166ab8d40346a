"""The host side of the gradient push (include/gdpt.h: gdpt_temporal_push_gradients*), without a GPU: the struct layouts of the Python
mirror against the header as the C compiler lays them out, the documented defaults, the Python builder, the refusals, which come
before any device call and name their field, and the argument errors of the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_gradients_ref as TG
import temporal_ref as T
from helpers import ROOT

EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_struct_layout_matches_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    fields = [("GdptTemporalGradParams", f) for f in ("j_max", "cos_min", "reserved")] + \
             [("GdptTemporalGradStats", f) for f in ("base", "pixels_gradient_reset", "sum_gradient_history")]
    body = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\n'
                   f'int main(){{printf("%zu %zu ", sizeof(GdptTemporalGradParams), sizeof(GdptTemporalGradStats)); {body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P, S = G.GdptTemporalGradParams, G.GdptTemporalGradStats
    assert got[:2] == [C.sizeof(P), C.sizeof(S)] == [32, 56]
    assert got[2:] == [getattr(P if s == "GdptTemporalGradParams" else S, f).offset for s, f in fields] == [0, 8, 16, 0, 40, 48]


def test_the_library_exports_the_entry_points(G):
    lib = C.CDLL(G.library_path())
    for name in ("gdpt_temporal_default_grad_params", "gdpt_temporal_push_gradients_device", "gdpt_temporal_push_gradients"):
        assert hasattr(lib, name), name


def test_default_params_and_the_builder(G):
    p = G.GdptTemporalGradParams(9.0, 9.0, (C.c_int32 * 4)(7, 7, 7, 7))
    G.lib().gdpt_temporal_default_grad_params(C.byref(p))
    assert (p.j_max, p.cos_min, list(p.reserved)) == (4.0, 0.02, [0, 0, 0, 0])
    G.lib().gdpt_temporal_default_grad_params(None)          # a null block is ignored
    q = G.temporal_grad_params(j_max=1.0, cos_min=0.5)
    assert (q.j_max, q.cos_min, list(q.reserved)) == (1.0, 0.5, [0, 0, 0, 0])
    assert (TG.GRAD_DEFAULTS["j_max"], TG.GRAD_DEFAULTS["cos_min"]) == (4.0, 0.02)


def a_camera(G, W=4, H=3):
    return T.gdpt_camera(G, T.camera(W, H, T.look_at((0.3, -0.2, 0.1), (0.5, 0.1, 1.0)), T.FOV))


# addresses that are never dereferenced: every call below is refused on the host
IMG, VAR, FEAT, OUT, VOUT, LEN, GLEN = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
GIN = [0x8000, 0x9000, 0xA000, 0xB000]            # gx, gx_var, gy, gy_var
GOUT = [0xC000, 0xD000, 0xE000, 0xF000]           # gx_out, gx_var_out, gy_out, gy_var_out
GIN_NAMES, GOUT_NAMES = ("gx", "gx_var", "gy", "gy_var"), ("gx_out", "gx_var_out", "gy_out", "gy_var_out")


def push(t, cam, img=IMG, var=VAR, feat=FEAT, gin=GIN, out=OUT, vout=VOUT, gout=GOUT, **kw):
    return t.push_gradients_device(cam, img, var, feat, gin, out, vout, gout, **kw)


REFUSED = [(dict(j_max=0.999), "j_max"), (dict(j_max=np.nan), "j_max"), (dict(j_max=np.inf), "j_max"), (dict(j_max=-4.0), "j_max"),
           (dict(cos_min=0.0), "cos_min"), (dict(cos_min=-0.1), "cos_min"), (dict(cos_min=1.0001), "cos_min"), (dict(cos_min=np.nan), "cos_min"),
           (dict(tau_z=-1e-9), "tau_z"), (dict(tau_n=1.0001), "tau_n"), (dict(s_min=0.0), "s_min"), (dict(max_history=0), "max_history")]


@pytest.mark.parametrize("kw,match", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_params_name_their_field(G, kw, match):
    t = G.Temporal(4, 3)
    with pytest.raises(G.GdptError, match=match):
        push(t, a_camera(G), **kw)
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match=match):
        t.push_gradients(a_camera(G), f, 0.01 * f, np.ones((8, 3, 4)), f, 0.01 * f, f, 0.01 * f, **kw)


def test_refused_arguments_name_their_field(G):
    t, cam = G.Temporal(4, 3), a_camera(G)
    L = G.lib()
    nothing = [None] * 7
    for fn in (L.gdpt_temporal_push_gradients_device, L.gdpt_temporal_push_gradients):
        assert fn(None, C.byref(cam), *nothing, None, None, *([None] * 8), None) != 0 and b"handle is null" in L.gdpt_last_error()
    # what the plain push refuses
    for kw, match in ((dict(img=0), "img is null"), (dict(var=0), "var is null"), (dict(feat=0), "feat is null"), (dict(out=0), "out is null"),
                      (dict(vout=0), "var_out is null"), (dict(out=IMG), "out must not alias"), (dict(vout=OUT), "var_out must not alias"),
                      (dict(len_ptr=VAR), "len must not alias")):
        with pytest.raises(G.GdptError, match=match):
            push(t, cam, **kw)
    with pytest.raises(G.GdptError, match="camera is null"):
        push(t, None)
    with pytest.raises(G.GdptError, match="camera width"):
        push(t, a_camera(G, 5, 3))
    # every new pointer, by name
    for i, name in enumerate(GIN_NAMES):
        with pytest.raises(G.GdptError, match=f": {name} is null"):
            push(t, cam, gin=GIN[:i] + [0] + GIN[i + 1:])
    for i, name in enumerate(GOUT_NAMES):
        with pytest.raises(G.GdptError, match=f": {name} is null"):
            push(t, cam, gout=GOUT[:i] + [0] + GOUT[i + 1:])
    # every output against every input and every other output
    inputs = [IMG, VAR, FEAT] + GIN
    for i, name in enumerate(GOUT_NAMES):
        for a in inputs:
            with pytest.raises(G.GdptError, match=f": {name} must not alias an input"):
                push(t, cam, gout=GOUT[:i] + [a] + GOUT[i + 1:])
        for b in [OUT, VOUT, LEN] + GOUT[:i]:
            with pytest.raises(G.GdptError, match=f": {name} must not alias another output"):
                push(t, cam, gout=GOUT[:i] + [b] + GOUT[i + 1:], len_ptr=LEN)
    for a in inputs:
        with pytest.raises(G.GdptError, match=": glen must not alias an input"):
            push(t, cam, glen_ptr=a)
    for b in [OUT, VOUT, LEN] + GOUT:
        with pytest.raises(G.GdptError, match=": glen must not alias another output"):
            push(t, cam, glen_ptr=b, len_ptr=LEN)
    for a in GIN:                                    # the primal's outputs against the new inputs
        for kw, name in ((dict(out=a), "out"), (dict(vout=a), "var_out"), (dict(len_ptr=a), "len")):
            with pytest.raises(G.GdptError, match=f": {name} must not alias an input"):
                push(t, cam, **kw)
    gp = G.temporal_grad_params()
    gp.reserved[3] = 1
    with pytest.raises(G.GdptError, match="temporal gradient reserved"):
        push(t, cam, grad_params=gp)
    p = G.temporal_params()
    p.reserved[0] = 1
    with pytest.raises(G.GdptError, match="temporal reserved"):
        push(t, cam, params=p)
    with pytest.raises(G.GdptError, match="four addresses"):
        push(t, cam, gin=GIN[:3])
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="handle's film"):
        t.push_gradients(cam, f, 0.01 * f, np.ones((8, 3, 4)), f, 0.01 * f, np.ones((3, 5, 3)), 0.01 * f)


def test_frame_refuses_gradients_of_a_path_session(G):
    t = G.Temporal(4, 3)
    with pytest.raises(G.GdptError, match="needs path=False"):
        t.frame(None, a_camera(G), 0, 1, 4, 2, path=True, gradients=True)
    with pytest.raises(G.GdptError, match="reconstruct needs gradients=True"):
        t.frame(None, a_camera(G), 0, 1, 4, 2, path=False, reconstruct="l2")
    with pytest.raises(G.GdptError, match="'l2', 'wl2' or 'wl1'"):
        t.frame(None, a_camera(G), 0, 1, 4, 2, path=False, gradients=True, reconstruct="l1")

    class PathScene:                                  # what frame() reads of a scene before it touches a device
        desc = G.parse_scene(os.path.join(ROOT, "scenes", "cbox", "cbox_old.xml"))
    assert PathScene.desc.desc.integrator == G.INTEGRATOR_PATH
    with pytest.raises(G.GdptError, match="Integrator::Path"):
        t.frame(PathScene, a_camera(G), 0, 1, 4, 2, path=False, gradients=True)


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.Temporal(4, 3).push_gradients(a_camera(G), f, 0.01 * f, np.ones((8, 3, 4)), f, 0.01 * f, f, 0.01 * f)
    with pytest.raises(G.GdptError, match="no HIP device"):
        push(G.Temporal(4, 3), a_camera(G), len_ptr=LEN, glen_ptr=GLEN)


FRAMES = ["--frames", "2", "--pass-spp", "2"]
CLI_ERRORS = [(["--temporal-gradients"], "--temporal-gradients needs --temporal", None),
              ([*FRAMES, "--temporal-gradients"], "--temporal-gradients needs --temporal", None),
              ([*FRAMES, "--reconstruct", "l2"], "--frames takes --reconstruct only with --temporal-gradients", None),
              ([*FRAMES, "--temporal", "--reconstruct", "wl2"], "--frames takes --reconstruct only with --temporal-gradients", None),
              ([*FRAMES, "--temporal", "--temporal-gradients", "--reconstruct", "l1"], "--reconstruct l2 | wl2 | wl1 (not l1)", None),
              ([*FRAMES, "--temporal", "--temporal-gradients"], "--temporal-gradients needs a GradPath scene", "cbox_old.xml"),
              ([*FRAMES, "--temporal", "--temporal-gradients", "--reconstruct", "wl2"], "--temporal-gradients needs a GradPath scene", "cbox_old.xml")]


@pytest.mark.parametrize("args,msg,scene", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg, scene):
    """exit status 2; the Integrator::Path refusal needs the scene parsed, and comes before any device call"""
    xml = os.path.join(ROOT, "scenes", "cbox", scene) if scene else "no_such_scene.xml"
    r = subprocess.run([EXE, *args, "-o", "o.exr", xml], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
