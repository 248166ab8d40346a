"""The host side of temporal reprojection and of the camera setter (include/gdpt.h: gdpt_temporal_*, gdpt_scene_set_camera), without
a GPU: the struct layout of the Python mirror against the header as the C compiler lays it out, the documented defaults, the Python
builder, the matrix M against numpy, the refusals, which come before any device call and name their field, and the argument errors
of the CLI. (The setter's refusals that need an uploaded scene stand in test_gpu_temporal.py: no scene exists without a device.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as T
from helpers import ROOT

EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_struct_layout_matches_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    fields = [("GdptTemporalParams", f) for f in ("tau_z", "tau_n", "s_min", "max_history", "reserved")] + \
             [("GdptTemporalStats", f) for f in ("pixels_left_out", "pixels_background", "pixels_reset", "sum_history", "push_ms")]
    body = "".join(f'printf("%zu ", offsetof({s}, {f}));' for s, f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\n'
                   f'int main(){{printf("%zu %zu ", sizeof(GdptTemporalParams), sizeof(GdptTemporalStats)); {body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    P, S = G.GdptTemporalParams, G.GdptTemporalStats
    assert got[:2] == [C.sizeof(P), C.sizeof(S)] == [40, 40]
    assert got[2:] == [getattr(P if s == "GdptTemporalParams" else S, f).offset for s, f in fields] == [0, 8, 16, 24, 28, 0, 8, 16, 24, 32]


def test_the_library_exports_the_entry_points(G):
    lib = C.CDLL(G.library_path())
    for name in ("gdpt_scene_set_camera", "gdpt_temporal_default_params", "gdpt_temporal_create", "gdpt_temporal_free", "gdpt_temporal_reset",
                 "gdpt_temporal_world_to_sample", "gdpt_temporal_push_device", "gdpt_temporal_push"):
        assert hasattr(lib, name), name


def test_default_params_and_the_builder(G):
    p = G.GdptTemporalParams(9.0, 9.0, 9.0, 9, (C.c_int32 * 3)(7, 7, 7))
    G.lib().gdpt_temporal_default_params(C.byref(p))
    assert (p.tau_z, p.tau_n, p.s_min, p.max_history, list(p.reserved)) == (0.05, 0.9, 1e-3, 32, [0, 0, 0])
    G.lib().gdpt_temporal_default_params(None)          # a null block is ignored
    q = G.temporal_params(tau_z=0.1, tau_n=-0.5, s_min=0.25, max_history=4)
    assert (q.tau_z, q.tau_n, q.s_min, q.max_history, list(q.reserved)) == (0.1, -0.5, 0.25, 4, [0, 0, 0])
    assert tuple(T.DEFAULTS[k] for k in ("tau_z", "tau_n", "s_min", "max_history")) == (0.05, 0.9, 1e-3, 32)


def a_camera(G, W=4, H=3):
    return T.gdpt_camera(G, T.camera(W, H, T.look_at((0.3, -0.2, 0.1), (0.5, 0.1, 1.0)), T.FOV))


def test_world_to_sample_against_numpy_and_its_refusals(G):
    cam = T.camera(33, 9, T.look_at((0.3, -0.2, 0.1), (0.5, 0.1, 1.0)), T.FOV)
    M, want = G.temporal_world_to_sample(T.gdpt_camera(G, cam)), T.world_to_sample(cam)
    assert np.abs(M - want).max() <= 1e-12 * np.abs(want).max()
    # a world point in front of the camera lands where its pixel is
    org, d = T.rays(cam)
    s = M @ np.append(org + 7.0 * d[4, 20], 1.0)
    assert s[3] > 0 and abs(s[0] / s[3] * 33 - 20.5) < 1e-9 and abs(s[1] / s[3] * 9 - 4.5) < 1e-9
    L = G.lib()
    out = (C.c_double * 16)()
    assert L.gdpt_temporal_world_to_sample(None, out) != 0 and b"camera is null" in L.gdpt_last_error()
    assert L.gdpt_temporal_world_to_sample(C.byref(a_camera(G)), None) != 0 and b"M is null" in L.gdpt_last_error()
    for field, value, match in (("sample_to_cam", np.nan, "sample_to_cam has a non-finite"), ("cam_to_world", np.inf, "cam_to_world has a non-finite")):
        bad = a_camera(G)
        getattr(bad, field)[5] = value
        with pytest.raises(G.GdptError, match=match):
            G.temporal_world_to_sample(bad)
    bad = a_camera(G)
    for i in range(16):
        bad.cam_to_world[i] = 0.0
    with pytest.raises(G.GdptError, match="cam_to_world is singular"):
        G.temporal_world_to_sample(bad)


def test_create_and_reset_refusals(G):
    L = G.lib()
    h = C.c_void_p()
    assert L.gdpt_temporal_create(4, 3, 0, None, None) != 0 and b"out is null" in L.gdpt_last_error()
    for args, match in (((0, 3, 0), "width"), ((4, 0, 0), "height"), ((1 << 15, 1 << 15, 0), "too large"), ((4, 3, -1), "device")):
        assert L.gdpt_temporal_create(*args, None, C.byref(h)) != 0 and match.encode() in L.gdpt_last_error(), args
    assert L.gdpt_temporal_reset(None) != 0 and b"handle is null" in L.gdpt_last_error()
    L.gdpt_temporal_free(None)                           # a null handle is ignored
    t = G.Temporal(4, 3)                                 # makes no device call
    t.reset()
    t.close()


# (keywords of temporal_params, what the message names)
REFUSED = [(dict(tau_z=-1e-9), "tau_z"), (dict(tau_z=np.nan), "tau_z"), (dict(tau_z=np.inf), "tau_z"),
           (dict(tau_n=-1.0001), "tau_n"), (dict(tau_n=1.0001), "tau_n"), (dict(tau_n=np.nan), "tau_n"),
           (dict(s_min=0.0), "s_min"), (dict(s_min=-0.1), "s_min"), (dict(s_min=1.0001), "s_min"), (dict(s_min=np.nan), "s_min"),
           (dict(max_history=0), "max_history"), (dict(max_history=-3), "max_history")]


@pytest.mark.parametrize("kw,match", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_params_name_their_field(G, kw, match):
    a, b, c, d, e = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000      # never dereferenced: every call below is refused on the host
    t = G.Temporal(4, 3)
    with pytest.raises(G.GdptError, match=match):
        t.push_device(a_camera(G), a, b, c, d, e, **kw)
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match=match):
        t.push(a_camera(G), f, 0.01 * f, np.ones((8, 3, 4)), **kw)


def test_refused_arguments_name_their_field(G):
    a, b, c, d, e, g = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    t, cam = G.Temporal(4, 3), a_camera(G)
    L = G.lib()
    assert L.gdpt_temporal_push_device(None, C.byref(cam), a, b, c, None, d, e, None, None) != 0 and b"handle is null" in L.gdpt_last_error()
    assert L.gdpt_temporal_push(None, C.byref(cam), a, b, c, None, d, e, None, None) != 0 and b"handle is null" in L.gdpt_last_error()
    for args, kw, match in (((None, a, b, c, d, e), {}, "camera is null"), ((cam, 0, b, c, d, e), {}, "img is null"), ((cam, a, 0, c, d, e), {}, "var is null"),
                            ((cam, a, b, 0, d, e), {}, "feat is null"), ((cam, a, b, c, 0, e), {}, "out is null"), ((cam, a, b, c, d, 0), {}, "var_out is null"),
                            ((cam, a, b, c, a, e), {}, "out must not alias"), ((cam, a, b, c, b, e), {}, "out must not alias"),
                            ((cam, a, b, c, c, e), {}, "out must not alias"),
                            ((cam, a, b, c, d, a), {}, "var_out must not alias"), ((cam, a, b, c, d, b), {}, "var_out must not alias"),
                            ((cam, a, b, c, d, c), {}, "var_out must not alias"), ((cam, a, b, c, d, d), {}, "var_out must not alias"),
                            ((cam, a, b, c, d, e), dict(len_ptr=a), "len must not alias"), ((cam, a, b, c, d, e), dict(len_ptr=b), "len must not alias"),
                            ((cam, a, b, c, d, e), dict(len_ptr=c), "len must not alias"), ((cam, a, b, c, d, e), dict(len_ptr=d), "len must not alias"),
                            ((cam, a, b, c, d, e), dict(len_ptr=e), "len must not alias"),
                            ((a_camera(G, 5, 3), a, b, c, d, e), {}, "camera width"), ((a_camera(G, 4, 2), a, b, c, d, e), {}, "camera height")):
        with pytest.raises(G.GdptError, match=match):
            t.push_device(*args, **kw)
    bad = a_camera(G)
    bad.sample_to_cam[0] = np.nan
    with pytest.raises(G.GdptError, match="sample_to_cam has a non-finite"):
        t.push_device(bad, a, b, c, d, e, len_ptr=g)
    p = G.temporal_params()
    p.reserved[2] = 1
    with pytest.raises(G.GdptError, match="temporal reserved"):
        t.push_device(cam, a, b, c, d, e, params=p)
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="handle's film"):
        t.push(cam, f, 0.01 * f, np.ones((8, 3, 5)))
    with pytest.raises(G.GdptError, match="handle's film"):
        t.push(cam, np.ones((3, 5, 3)), 0.01 * f, np.ones((8, 3, 4)))


def test_set_camera_refuses_null_arguments(G):
    L = G.lib()
    assert L.gdpt_scene_set_camera(None, C.byref(a_camera(G))) != 0 and b"scene is null" in L.gdpt_last_error()
    assert L.gdpt_scene_set_camera(None, None) != 0 and b"scene is null" in L.gdpt_last_error()


def test_valid_arguments_need_a_device(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-GPU error path is covered on the CPU runner")
    f = np.ones((3, 4, 3))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.Temporal(4, 3).push(a_camera(G), f, 0.01 * f, np.ones((8, 3, 4)))
    with pytest.raises(G.GdptError, match="no HIP device"):
        G.Temporal(4, 3).push_device(a_camera(G), 0x1000, 0x2000, 0x3000, 0x4000, 0x5000)


ONE_DEVICE = "--frames, --orbit and --temporal are single-device options"
NEED_FRAMES = "--orbit, --temporal and --temporal-max-history need --frames"
CLI_ERRORS = [(["--orbit", "2"], NEED_FRAMES), (["--temporal"], NEED_FRAMES), (["--temporal-max-history", "4"], NEED_FRAMES),
              (["--pass-spp", "2", "--orbit", "2", "--temporal"], NEED_FRAMES),
              (["--frames", "2", "--gpus", "2"], ONE_DEVICE), (["--frames", "2", "--orbit", "2", "--gpus", "2"], ONE_DEVICE),
              (["--frames", "2", "--temporal", "--pass-spp", "2", "--gpus", "2"], ONE_DEVICE),
              (["--frames", "2", "--pass-spp", "2", "--sample-devices", "0,1"], ONE_DEVICE),
              (["--frames", "2", "--orbit", "2", "--pass-spp", "2", "--sample-devices", "0,1"], ONE_DEVICE),
              (["--frames", "2", "--temporal", "--pass-spp", "2", "--sample-devices", "0,1"], ONE_DEVICE),
              (["--frames", "2", "--pass-spp", "2", "--denoised", "d.exr", "--select", "mean,nlm"], ONE_DEVICE),
              (["--frames", "2", "--temporal", "--pass-spp", "2", "--denoised", "d.exr", "--select", "mean,nlm"], ONE_DEVICE),
              (["--frames", "2", "--orbit", "1", "--pass-spp", "2", "--denoised", "d.exr", "--select", "mean,nlm"], ONE_DEVICE),
              (["--frames", "0"], "--frames takes a number of frames >= 1"), (["--frames", "2"], "--frames needs --pass-spp"),
              (["--frames", "2", "--pass-spp", "2", "--temporal-max-history", "0"], "--temporal-max-history takes a number of frames >= 1"),
              (["--frames", "2", "--pass-spp", "2", "--temporal-max-history", "3"], "--temporal-max-history needs --temporal"),
              (["--frames", "2", "--pass-spp", "2", "--denoised", "d.exr"], "--frames writes --denoised only with --temporal and --atrous-levels"),
              (["--frames", "2", "--pass-spp", "2", "--temporal", "--denoised", "d.exr"], "--frames writes --denoised only with --temporal and --atrous-levels"),
              (["--frames", "2", "--pass-spp", "2", "--variance", "v.exr"], "--frames is combined with")]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(args, msg):
    r = subprocess.run([EXE, *args, "-o", "o.exr", "no_such_scene.xml"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (r.returncode, r.stderr)
