"""CPU: adaptive sampling's host side (PT_FLAG_ADAPTIVE).  pt_create / pt_build touch no GPU and pt_render_adaptive / pt_adaptive_mask
refuse a bad call before any device call, so the validation runs here.  The numpy restatement of the selection criterion (include/pt_api.h)
that test_gpu_adaptive.py checks the device against is itself checked here on hand-computed edge cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

PT_ERR_ARG, PT_ERR_STATE = -1, -3
F = np.float32


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- the numpy restatement (f32, every operation correctly rounded, in the order of include/pt_api.h)
def luminance(rgb):
    rgb = np.asarray(rgb, np.float32)
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def fold_moments(samples):
    """Q after accumulating `samples` ([S, ...rows, cols, 4] finalised samples) in sample order, one f32 add of L * L per sample"""
    q = np.zeros(samples.shape[1:-1], np.float32)
    for s in range(samples.shape[0]):
        lum = luminance(samples[s])
        q = q + lum * lum
    return q


def criterion(acc, q, rel_error, abs_floor=0.0, min_samples=2, max_samples=0):
    """active mask of the pixels of `acc` ([..., 4] f32) and `q` ([...] f32)"""
    acc = np.asarray(acc, np.float32)
    q = np.asarray(q, np.float32)
    n = acc[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = luminance(acc) / n
        v = q / n - m * m
        v = np.where(v > F(0), v, F(0))
        e2 = v / n
        t = F(rel_error) * np.where(m > F(abs_floor), m, F(abs_floor))
        ni = n.astype(np.int64)
        capped = np.full(n.shape, max_samples == 0) | (ni < max_samples)
        return (ni < min_samples) | (capped & (e2 > t * t))


def _px(rgb, n, q):
    """one pixel: acc = (rgb, n), moments q"""
    return np.array([[list(rgb) + [n]]], np.float32), np.array([[q]], np.float32)


def test_criterion_edge_cases():
    # n < min_samples: active whatever the noise (n = 0 included, where m is 0/0)
    a, q = _px((0, 0, 0), 0, 0)
    assert criterion(a, q, 0.5, min_samples=2)[0, 0]
    a, q = _px((3, 3, 3), 3, 3)              # three equal samples of luminance 1: no noise
    assert criterion(a, q, 0.5, min_samples=4)[0, 0]
    assert not criterion(a, q, 0.5, min_samples=3)[0, 0]
    # v < 0 from rounding: a constant pixel whose Q / n falls one ulp below m * m is clamped to zero, so it is converged for any rel_error
    lum = luminance(np.array([0.3, 0.3, 0.3], np.float32))
    n = 7
    S = F(0)
    Q = F(0)
    acc = np.zeros(3, np.float32)
    for _ in range(n):
        acc = acc + np.float32(0.3)
        Q = Q + lum * lum
    S = luminance(acc)
    m = S / F(n)
    v = Q / F(n) - m * m
    assert v != 0, "the case needs a rounding residue"
    a, q = np.array([[list(acc) + [n]]], np.float32), np.array([[Q]], np.float32)
    assert criterion(a, q, 0.0, min_samples=2)[0, 0] == bool(v > 0)
    # a variance known exactly: samples of luminance 0 and 2 (rgb all equal, so L = rgb * (0.2126 + 0.7152 + 0.0722) rounded)
    a, q = _px((4, 4, 4), 4, 8)              # two samples of 2, two of 0 => S ~ 4, m ~ 1, Q / n = 2, v ~ 1, e2 ~ 1/4
    e2 = ((F(8) / F(4)) - (luminance(np.array([4, 4, 4], np.float32)) / F(4)) ** 2) / F(4)
    # t * t just above / just below e2
    rel_hi = float(np.sqrt(np.float64(e2)) * 1.001)
    rel_lo = float(np.sqrt(np.float64(e2)) * 0.999)
    assert not criterion(a, q, rel_hi, min_samples=2)[0, 0]
    assert criterion(a, q, rel_lo, min_samples=2)[0, 0]
    # the max_samples cap: a noisy pixel at the cap is done, one sample below it is not
    assert not criterion(a, q, rel_lo, min_samples=2, max_samples=4)[0, 0]
    assert criterion(a, q, rel_lo, min_samples=2, max_samples=5)[0, 0]
    assert criterion(a, q, rel_lo, min_samples=2, max_samples=0)[0, 0]
    # min_samples wins over the cap
    assert criterion(a, q, 1e9, min_samples=5, max_samples=5)[0, 0]
    # abs_floor: a dark pixel's error is measured against the floor instead of its own mean
    a, q = _px((0.004, 0.004, 0.004), 4, F(0.002) * F(0.002) * 2)   # mean luminance ~ 1e-3, noise ~ 1e-3: relative error ~ 0.5
    assert criterion(a, q, 0.1, abs_floor=0.0)[0, 0]
    assert not criterion(a, q, 0.1, abs_floor=0.05)[0, 0]
    # vectorised over a frame: each pixel on its own
    acc = np.concatenate([_px((0, 0, 0), 0, 0)[0], _px((3, 3, 3), 3, 3)[0]], axis=1)
    qq = np.array([[0, 3]], np.float32)
    assert criterion(acc, qq, 0.5, min_samples=3).tolist() == [[True, False]]


def test_fold_moments_is_sequential_f32():
    rng = np.random.default_rng(5)
    s = rng.random((5, 2, 3, 4), dtype=np.float32) * F(7)
    q = fold_moments(s)
    want = np.zeros((2, 3), np.float32)
    for k in range(5):
        lum = (F(0.2126) * s[k, ..., 0] + F(0.7152) * s[k, ..., 1]) + F(0.0722) * s[k, ..., 2]
        want = (want + lum * lum).astype(np.float32)
    assert np.array_equal(q.view(np.uint32), want.view(np.uint32))


def test_new_names_exported(api):
    for name in ("pt_render_adaptive", "pt_adaptive_mask", "pt_read_moments", "pt_write_moments"):
        assert name in api.EXPORTS
        assert hasattr(C.CDLL(api._build.LIB_PATH), name)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert re.search(r"PT_FLAG_ADAPTIVE\s*=\s*32u", hdr) and api.FLAG_ADAPTIVE == 32
    hpp = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for m in ("render_adaptive", "adaptive_mask", "read_moments", "write_moments"):
        assert m in hpp


def _renderer(api, flags):
    from path_tracer_amd import scenes
    return api.Renderer(scenes.cornell_box(16, 8), 16, 8, max_bounces=2, flags=flags)


def _call(api, r, fn, crit, n=1):
    L = api.lib()
    na = C.c_uint32(7)
    if fn == "render":
        return L.pt_render_adaptive(r.ctx, crit, n, C.byref(na)), na.value
    mask = np.zeros(16 * 8, np.uint8)
    return L.pt_adaptive_mask(r.ctx, crit, mask.ctypes.data_as(C.c_void_p), C.byref(na)), na.value


@pytest.mark.parametrize("fn", ["render", "mask"])
def test_without_the_flag_is_a_state_error(api, fn):
    r = _renderer(api, 0)
    good = C.byref(api.Adaptive(0.1, 0.0, 4, 0))
    assert _call(api, r, fn, good)[0] == PT_ERR_STATE
    assert "PT_FLAG_ADAPTIVE" in api.lib().pt_last_error(r.ctx).decode()
    assert _call(api, r, fn, None)[0] == PT_ERR_STATE     # the flag is looked at first
    L = api.lib()
    q = np.zeros(16 * 8, np.float32)
    assert L.pt_read_moments(r.ctx, q.ctypes.data_as(C.c_void_p)) == PT_ERR_STATE
    assert L.pt_write_moments(r.ctx, q.ctypes.data_as(C.c_void_p)) == PT_ERR_STATE
    with pytest.raises(api.PtError) as e:
        r.render_adaptive(1, 0.1) if fn == "render" else r.adaptive_mask(0.1)
    assert e.value.code == PT_ERR_STATE


BAD = [
    (-0.1, 0.0, 4, 0), (float("nan"), 0.0, 4, 0), (float("inf"), 0.0, 4, 0),
    (0.1, -1.0, 4, 0), (0.1, float("nan"), 4, 0), (0.1, float("inf"), 4, 0),
    (0.1, 0.0, 0, 0), (0.1, 0.0, 1, 0), (0.1, 0.0, 8, 7), (0.1, 0.0, 8, 1),
]


@pytest.mark.parametrize("fn", ["render", "mask"])
@pytest.mark.parametrize("bad", BAD)
def test_invalid_criterion_is_an_argument_error(api, fn, bad):
    r = _renderer(api, api.FLAG_ADAPTIVE)
    rc, na = _call(api, r, fn, C.byref(api.Adaptive(*bad)))
    assert rc == PT_ERR_ARG, (bad, rc, api.lib().pt_last_error(r.ctx).decode())
    assert na == 7, "n_active is written only on success"


@pytest.mark.parametrize("fn", ["render", "mask"])
def test_null_arguments(api, fn):
    r = _renderer(api, api.FLAG_ADAPTIVE)
    assert _call(api, r, fn, None)[0] == PT_ERR_ARG
    L = api.lib()
    assert L.pt_render_adaptive(None, None, 1, None) == PT_ERR_ARG
    assert L.pt_adaptive_mask(None, None, None, None) == PT_ERR_ARG
    assert L.pt_read_moments(r.ctx, None) == PT_ERR_ARG
    assert L.pt_write_moments(r.ctx, None) == PT_ERR_ARG


def test_too_many_samples_is_an_argument_error(api):
    r = _renderer(api, api.FLAG_ADAPTIVE)
    crit = C.byref(api.Adaptive(0.1, 0.0, 4, 0))
    assert _call(api, r, "render", crit, n=0xffffffff - (1 << 24) + 1)[0] == PT_ERR_ARG


def test_python_wrapper_validates_the_moments_shape(api):
    r = _renderer(api, api.FLAG_ADAPTIVE)
    with pytest.raises(api.PtError):
        r.write_moments(np.zeros(5, np.float32))
