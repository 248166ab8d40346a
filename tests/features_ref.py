"""Restatement of the feature render of include/gdpt.h (gdpt_features_render*), sample by sample from the CPU oracle's pieces:
pcg_init / pcg_next_double, sample_primary, intersect, texture_eval, and the fold of the definition. Not collected by pytest;
tests/test_gpu_features.py holds the kernel against it.

    samples(osc, desc, spp, window, rows) -> (spp, 8, H, W) values, (spp, H, W) shape ids (-1: a miss)
    fold(values)                           -> (8, H, W) means, (8, H, W) variances of the means
    render(...)                            -> fold(samples(...)[0])"""
import numpy as np

import oracle_py as O

CHANNELS = 8
MAT_DISNEY_CLEARCOAT = 6


def sample(osc, desc, x, y, stream):
    """The eight values of the sample of pixel (x, y) that draws from `stream`, and the shape it hit (-1: none)."""
    w, h = desc.camera.width, desc.camera.height
    state, inc = O.pcg_init(stream)
    rx, state = O.pcg_next_double(state, inc)
    ry, state = O.pcg_next_double(state, inc)
    org, dirv = osc.sample_primary((x + rx) / w, (y + ry) / h)
    v = osc.intersect(org, dirv, 0.0, float("inf"), ray_diff=(0.0, 0.25 / max(w, h)))
    out = np.zeros(CHANNELS)
    if v is None:
        return out, -1
    m = desc.materials[v.material_id]
    if m.type == MAT_DISNEY_CLEARCOAT:
        out[0:3] = 1.0
    else:
        out[0:3] = osc.texture_eval(m.tex[0], list(v.uv), v.uv_screen_size, channels=3)
    out[3:6] = list(v.frame_n)
    d = np.array(list(v.position)) - org
    out[6] = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    out[7] = 1.0
    return out, v.shape_id


def samples(osc, desc, spp, window=None, rows=None):
    w, h = desc.camera.width, desc.camera.height
    stream_spp, first = window if window is not None else (spp, 0)
    y0, y1 = rows if rows is not None else (0, h)
    vals, shapes = np.zeros((spp, CHANNELS, h, w)), np.full((spp, h, w), -1, dtype=np.int64)
    for y in range(y0, y1):
        for x in range(w):
            for s in range(spp):
                vals[s, :, y, x], shapes[s, y, x] = sample(osc, desc, x, y, (y * w + x) * stream_spp + first + s)
    return vals, shapes


def fold(vals):
    """d = x - mean; mean += d / i; M2 += d (x - mean), in sample order; var = M2 / (n (n - 1)), 0 for n = 1."""
    n = vals.shape[0]
    mean, m2 = np.zeros(vals.shape[1:]), np.zeros(vals.shape[1:])
    for i in range(1, n + 1):
        x = vals[i - 1]
        d = x - mean
        mean = mean + d / float(i)
        m2 = m2 + d * (x - mean)
    var = m2 / float(n * (n - 1)) if n > 1 else np.zeros_like(m2)
    return mean, var


def render(osc, desc, spp, window=None, rows=None):
    return fold(samples(osc, desc, spp, window, rows)[0])
