"""CPU: adaptive lightmap baking without a GPU: the symbols; the texel criterion evaluated on the host (pt_lightmap_adaptive_mask with
on_device = 0) bit for bit against the numpy restatement of tests/lightmap_adaptive_common.py on states whose covered texels sit on the
criterion's edges; every refusal include/pt_api.h promises before any device call, in its order; the Python wrappers' shape checks; and the
texel filter with per-texel counts (pt_lightmap_denoise_counts on the host) against pt_lightmap_denoise and the frame filter's restatement.
No GPU is touched (the kernels and the bake: tests/test_gpu_lightmap_adaptive.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_common as DC
import lightmap_adaptive_common as LA
import lightmap_common as LC
import lightmap_denoise_common as LD
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, HIP, STATE, LIMIT = -1, -2, -3, -5
OFF = 1e30          # reach * reach overflows: the term is off


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_RENDERERS = {}


def renderer(api, kind):
    if kind not in _RENDERERS:
        _RENDERERS[kind] = api.Renderer(LA.scene(kind)[0], 48, 32)
    return _RENDERERS[kind]


def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_bake_lightmap_adaptive", "pt_lightmap_adaptive_mask", "pt_lightmap_denoise_counts"):
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    for method in ("bake_lightmap_adaptive", "lightmap_adaptive_mask", "set_lightmap_counts", "denoise_lightmap"):
        assert callable(getattr(api.Renderer, method))
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for name in ("bake_lightmap_adaptive(", "lightmap_adaptive_mask(", "denoise_lightmap_counts(", "lightmap_means("):
        assert name in wrapper, name
    # the two items left the filter's out-of-scope list, and the new limits are stated
    assert "Out of scope: per-texel sample counts" not in header
    assert "adaptive directional bakes" in header


# ---- the criterion on the host
@pytest.mark.parametrize("kind, w, h", LA.MAPS)
def test_host_selection_is_the_definition(api, kind, w, h):
    r = renderer(api, kind)
    model = LA.scene(kind)[1]
    cov = LA.covered(kind, w, h)
    assert cov.any() and (kind in ("quad",) or not cov.all())
    for offset in (range(len(LA.EDGES)) if cov.sum() < len(LA.EDGES) else (0, 5)):
        state = LA.edge_state(cov, seed=3 + offset, offset=offset)
        sums, sumsq, counts, names = state
        if cov.sum() >= len(LA.EDGES):
            LA.check_edges_are_meaningful(state, cov)
        for crit in LA.CRITS:
            want = LA.active(sums, sumsq, counts, cov, **crit)
            got = r.lightmap_adaptive_mask(model, 0, sums, sumsq, counts, on_device=False, **crit)
            assert np.array_equal(got, want), (kind, w, h, offset, crit, names[got != want])
            assert not got[~cov].any()


def test_the_single_texel_map_meets_every_edge(api):
    """1 x 1: the one covered texel takes each edge in turn, and the restatement's answers differ between them"""
    cov = LA.covered("quad", 1, 1)
    assert cov.shape == (1, 1) and cov.all()
    answers = {bool(LA.active(*LA.edge_state(cov, offset=o)[:3], cov, **LA.EDGE_CRIT)[0, 0]) for o in range(len(LA.EDGES))}
    assert answers == {True, False}


# ---- errors
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bake(r, prm, crit, sums, sumsq, counts, cov=None, n=None):
    return r.L.pt_bake_lightmap_adaptive(r.ctx, None if prm is None else C.byref(prm), None if crit is None else C.byref(crit), _p(sums), _p(sumsq), _p(counts), _p(cov),
                                         None if n is None else C.byref(n))


def _mask(r, on_device, model, w, h, crit, sums, sumsq, counts, mask, n):
    return r.L.pt_lightmap_adaptive_mask(r.ctx, on_device, model, 0, w, h, None if crit is None else C.byref(crit), _p(sums), _p(sumsq), _p(counts), _p(mask),
                                         None if n is None else C.byref(n))


BAD_CRITS = [(-1.0, 0.0, 2, 0), (np.nan, 0.0, 2, 0), (np.inf, 0.0, 2, 0), (0.1, -1.0, 2, 0), (0.1, np.nan, 2, 0), (0.1, np.inf, 2, 0), (0.1, 0.0, 1, 0), (0.1, 0.0, 0, 0),
             (0.1, 0.0, 4, 3)]


def test_bake_arguments_are_refused_in_order_before_any_device_call_and_nothing_changes(api):
    r = renderer(api, "box")
    model = LA.scene("box")[1]
    w, h, n = 12, 8, 4
    cov = LA.covered("box", w, h)
    first = tuple(np.argwhere(cov)[0]); hole = tuple(np.argwhere(~cov)[0])
    sums = np.full((h, w, 3), 3, F); sq = np.full((h, w), 3, F); counts = np.full((h, w), 5, np.uint32); cv = np.full((h, w), 7, np.uint8)
    n_active = C.c_uint32(77)
    good = lambda **kw: api.LightmapParams(*[kw.get(k, v) for k, v in (("model", model), ("instance", 0), ("w", w), ("h", h), ("first_sample", 0), ("n_samples", n),
                                                                         ("key_base", 0), ("bias", 0.25))])
    crit = api.Adaptive(0.1, 0.0, 2, 0)
    error = lambda: r.L.pt_last_error(r.ctx).decode()
    call = lambda prm, c, a, b, d: _bake(r, prm, c, a, b, d, cv, n_active)
    # 1. what pt_bake_lightmap_moments refuses
    assert call(None, crit, sums, sq, counts) == ARG and call(good(), crit, None, sq, counts) == ARG
    assert call(good(), crit, sums, None, counts) == ARG and "sumsq" in error()
    for prm, code in ((good(model=-1), ARG), (good(model=6), ARG), (good(instance=1), ARG), (good(w=0), ARG), (good(h=0), ARG), (good(n_samples=0), ARG),
                      (good(bias=np.nan), ARG), (good(model=0), STATE), (good(w=16385, h=1), LIMIT), (good(key_base=0xFFFFFFFF), ARG)):
        assert call(prm, crit, sums, sq, counts) == code, (prm.model, prm.w, prm.h, prm.n_samples, code)
    reserved = good()
    reserved.reserved[1] = 1
    assert call(reserved, crit, sums, sq, counts) == ARG
    # ... which come before 2., a NULL crit or counts and a first sample
    assert call(good(model=0), None, sums, sq, None) == STATE and call(good(w=16385, h=1), None, sums, sq, None) == LIMIT
    assert call(good(), None, sums, sq, counts) == ARG and call(good(), crit, sums, sq, None) == ARG
    assert call(good(first_sample=1), crit, sums, sq, counts) == ARG and "first_sample" in error()
    # ... which come before 3., an invalid criterion
    assert call(good(first_sample=1), api.Adaptive(-1.0, 0.0, 2, 0), sums, sq, counts) == ARG and "first_sample" in error()
    for bad in BAD_CRITS:
        assert call(good(), api.Adaptive(*bad), sums, sq, counts) == ARG and "pt_adaptive" in error(), bad
    # 4. the limit, on covered texels only, and after 3.
    over = counts.copy()
    over[first] = (1 << 24) - n + 1
    assert call(good(), crit, sums, sq, over) == LIMIT and "2^24" in error()
    assert call(good(), api.Adaptive(0.1, 0.0, 1, 0), sums, sq, over) == ARG
    assert call(good(n_samples=(1 << 24) + 1 - 5 + 1), crit, sums, sq, counts) == LIMIT
    # the context needs no PT_FLAG_ADAPTIVE for any of this
    assert not (r.cfg.flags & api.FLAG_ADAPTIVE)
    assert (sums == 3).all() and (sq == 3).all() and (counts == 5).all() and (cv == 7).all() and n_active.value == 77
    # exactly 2^24 - n_samples passes the argument checks (what follows is the device's: a bake, or no device to run it on), and an
    # uncovered texel's count never raises the limit
    edge = counts.copy()
    edge[first] = (1 << 24) - n
    edge[hole] = 0xFFFFFFFF
    assert call(good(), crit, sums.copy(), sq.copy(), edge) in (0, HIP)


def test_mask_arguments_are_refused(api):
    r = renderer(api, "box")
    model = LA.scene("box")[1]
    w, h = 12, 8
    cov = LA.covered("box", w, h)
    sums, sumsq, counts, _ = LA.edge_state(cov)
    mask = np.full((h, w), 7, np.uint8); n = C.c_uint32(77)
    crit = api.Adaptive(0.25, 0.5, 4, 32)
    for on_device in (0, 1):
        for m, ww, hh, code in ((-1, w, h, ARG), (6, w, h, ARG), (0, w, h, STATE), (model, 0, h, ARG), (model, 16385, 1, LIMIT)):
            assert _mask(r, on_device, m, ww, hh, crit, sums, sumsq, counts, mask, n) == code
        assert _mask(r, on_device, model, w, h, None, sums, sumsq, counts, mask, n) == ARG
        assert _mask(r, on_device, model, w, h, crit, None, sumsq, counts, mask, n) == ARG
        assert _mask(r, on_device, model, w, h, crit, sums, None, counts, mask, n) == ARG
        assert _mask(r, on_device, model, w, h, crit, sums, sumsq, None, mask, n) == ARG
        assert _mask(r, on_device, model, w, h, crit, sums, sumsq, counts, mask, None) == ARG
        for bad in BAD_CRITS:
            assert _mask(r, on_device, model, w, h, api.Adaptive(*bad), sums, sumsq, counts, mask, n) == ARG, bad
        over = counts.copy()
        over[tuple(np.argwhere(cov)[3])] = (1 << 24) + 1
        assert _mask(r, on_device, model, w, h, crit, sums, sumsq, over, mask, n) == LIMIT
    assert (mask == 7).all() and n.value == 77
    # 2^24 itself is a count, the uncovered texels' 2^32 - 1 raise nothing, and the mask may be declined
    at = counts.copy()
    at[tuple(np.argwhere(cov)[3])] = 1 << 24
    assert (counts[~cov] == 0xFFFFFFFF).all()
    assert _mask(r, 0, model, w, h, crit, sums, sumsq, at, None, n) == 0 and 0 < n.value < cov.sum()


def test_python_wrappers_validate_shapes(api):
    r = renderer(api, "box")
    model = LA.scene("box")[1]
    w, h = 12, 8
    sums = np.zeros((h, w, 3), F); sq = np.zeros((h, w), F); counts = np.ones((h, w), np.uint32); cov = np.ones((h, w), np.uint8)
    for kw in (dict(sums=sums[:-1]), dict(sumsq=sq[:, :-1]), dict(counts=counts.reshape(w, h)), dict(sums=np.zeros((h, w), F))):
        with pytest.raises(api.PtError) as e:
            r.bake_lightmap_adaptive(model, 0, w, h, 4, 0.1, **kw)
        assert e.value.code == ARG and "bake_lightmap_adaptive" in str(e.value)
    for args in ((sums.reshape(-1, 3), sq, counts), (sums, sq[:-1], counts), (sums, sq, counts[:, 1:]), (sums, None, counts), (sums, sq, None)):
        with pytest.raises(api.PtError) as e:
            r.lightmap_adaptive_mask(model, 0, *args, 0.1)
        assert e.value.code == ARG
    with pytest.raises(api.PtError):
        r.denoise_lightmap(model, 0, sums, 0, counts=counts[:-1], on_device=False)
    for args in ((sums[..., :2], counts, cov), (sums, counts[:-1], cov), (sums, counts, cov[:, :-1])):
        with pytest.raises(api.PtError):
            r.set_lightmap_counts(model, 0, *args)


# ---- the filter with a count per texel
def _mixed_counts(cov, seed):
    rng = np.random.default_rng(seed)
    counts = rng.choice(np.array([4, 8, 12, 16, 1 << 24], np.uint32), cov.shape)
    counts[~cov] = 0          # never read
    return counts


@pytest.mark.parametrize("kind, w, h", [("box", 37, 19), ("box", 48, 32), ("quad", 1, 1)])
def test_uniform_counts_are_the_plain_filter(api, kind, w, h):
    r = renderer(api, kind)
    model = LA.scene(kind)[1]
    cov = LA.covered(kind, w, h)
    sums, sumsq = LD.synthetic(w, h, 12, seed=7)
    counts = np.where(cov, 12, 0).astype(np.uint32)
    for sq in (sumsq, None):
        for it in (1, 5):
            want, want_area = r.denoise_lightmap(model, 0, sums, 12, sumsq=sq, iterations=it, on_device=False, want_area=True)
            got, area = r.denoise_lightmap(model, 0, sums, 0, sumsq=sq, iterations=it, on_device=False, want_area=True, counts=counts)
            assert_bit_equal(got, want, f"{kind} {w}x{h} uniform counts, moments {sq is not None}, {it} levels")
            assert_bit_equal(area, want_area, "texel area")
    assert w * h == 1 or np.abs(got - sums / F(12))[cov].max() > 0


@pytest.mark.parametrize("kind, w, h", [("box", 37, 19), ("box", 48, 32)])
@pytest.mark.parametrize("moments", [True, False])
def test_mixed_counts_without_reach_are_the_frame_filter(api, kind, w, h, moments):
    """reach switched off: pt_post_denoise's definition (tests/denoise_common.py) on accum = (sum, counts), w = 0 where uncovered"""
    r = renderer(api, kind)
    sc, model = LA.scene(kind)
    m = sc.models[model]
    table = LC.texels(m.positions, m.normals, m.uvs, m.matrices[0], w, h)
    cov = table[0] != LC.MISS
    counts = _mixed_counts(cov, seed=11)
    assert len(np.unique(counts[cov])) == 5
    unit, unit_sq = LD.synthetic(w, h, 1, seed=5)
    sums = (unit * counts.astype(F)[..., None]).astype(F); sumsq = (unit_sq * counts.astype(F)).astype(F)
    sq = sumsq if moments else None
    acc, pos, nrm, mdl = LD.frame_images(table, sums, 1)
    acc[..., 3] = np.where(cov, counts.astype(F), F(0))
    want = DC.filtered(acc, pos, nrm, mdl, None, sq, 4, 0.0, 0, 0.0)
    got = r.denoise_lightmap(model, 0, sums, 0, sumsq=sq, iterations=4, reach=OFF, on_device=False, counts=counts)
    assert_bit_equal(got, want[..., :3], f"{kind} {w}x{h} mixed counts, moments {moments}: reach off")
    # and the counts matter: one count for all gives another map
    flat = r.denoise_lightmap(model, 0, sums, 8, sumsq=sq, iterations=4, reach=OFF, on_device=False)
    assert (flat != got).any()


def test_filter_counts_arguments_are_refused(api):
    r = renderer(api, "box")
    model = LA.scene("box")[1]
    w, h = 12, 8
    cov = LA.covered("box", w, h)
    sums, sumsq = LD.synthetic(w, h, 16, seed=1)
    counts = np.where(cov, 16, 0).astype(np.uint32)
    out = np.full((h, w, 3), 7, F)
    prm = lambda n=0: api.LightmapDenoiseParams(model, 0, w, h, n, api.DenoiseParams(0, 0.0, 0, 0.0), 0.0)
    call = lambda on_device, p, c: r.L.pt_lightmap_denoise_counts(r.ctx, on_device, C.byref(p), _p(sums), _p(sumsq), _p(c), _p(out), None)
    zero = counts.copy(); zero[tuple(np.argwhere(cov)[2])] = 0
    over = counts.copy(); over[tuple(np.argwhere(cov)[2])] = (1 << 24) + 1
    for on_device in (0, 1):
        assert call(on_device, prm(16), counts) == ARG and "n_samples" in r.L.pt_last_error(r.ctx).decode()
        assert call(on_device, prm(), None) == ARG
        assert call(on_device, prm(), zero) == ARG and "count" in r.L.pt_last_error(r.ctx).decode()
        assert call(on_device, prm(), over) == ARG
    assert (out == 7).all()
    # an uncovered texel's count of 0 (or anything) is fine
    assert call(0, prm(), counts) == 0 and not (out == 7).all()
    junk = counts.copy(); junk[~cov] = 0xFFFFFFFF
    out2 = out.copy()
    assert call(0, prm(), junk) == 0
    assert_bit_equal(out, out2, "uncovered counts are not read")
