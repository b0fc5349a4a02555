"""CPU: reflection probes (pt_probe_radiance_dir, pt_bake_probe_radiance, pt_probe_radiance_prefilter, pt_set_probe_grid_radiance,
pt_get_probe_grid_radiance_info, pt_probe_grid_specular) without a GPU: the symbols, every refusal include/pt_api.h promises before any device
call and their order, each with "nothing changed" checked, the texel direction, the host prefilter and the host lookup against the numpy
restatement of tests/probe_radiance_common.py bit for bit, the furnace, the lobe's width, the exact cases and the lifetime of radiance.  No
GPU is touched (the bake, the device prefilter and lookup and the view: tests/test_gpu_probe_radiance.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lightmap_common as LC
import probe_depth_common as PD
import probe_grid_common as PG
import probe_radiance_common as PR
from conftest import ROOT, assert_bit_equal

F = np.float32
ARG, STATE, LIMIT = -1, -3, -5
NEW_SYMBOLS = ["pt_bake_probe_radiance", "pt_probe_radiance_prefilter", "pt_set_probe_grid_radiance", "pt_get_probe_grid_radiance_info",
               "pt_probe_grid_specular"]
ALPHAS5 = (0.1, 0.2, 0.4, 0.7, 1.0)
ALPHAS8 = (0.05, 0.1, 0.15, 0.25, 0.4, 0.6, 0.8, 1.0)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _renderer(api):
    sc, _ = LC.cornell_atlas_scene()
    return api.Renderer(sc, 48, 32), sc


def _alpha8(alphas):
    return (C.c_float * 8)(*(list(alphas) + [0.0] * (8 - len(alphas))))


def _rad_struct(api, res=4, alphas=(0.2, 0.5), n_levels=None, reserved=(0, 0, 0, 0, 0, 0)):
    return api.ProbeRadiance(res, len(alphas) if n_levels is None else n_levels, _alpha8(alphas), (C.c_uint32 * 6)(*reserved))


def _filter_struct(api, res=4, n_probes=2, alphas=(0.2, 0.5), n_levels=None, reserved=(0, 0, 0, 0, 0)):
    return api.ProbeRadianceFilter(res, n_probes, len(alphas) if n_levels is None else n_levels, _alpha8(alphas), (C.c_uint32 * 5)(*reserved))


# ---------------------------------------------------------------------------------------------------------------- exports and refusals
def test_symbols_are_exported_bound_and_declared(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert f"int {name}(pt_ctx* ctx" in header, name
    assert "pt_probe_radiance_dir" in api.EXPORTS and "int pt_probe_radiance_dir(uint32_t res" in header
    assert "typedef struct pt_probe_radiance_params" in header and C.sizeof(api.ProbeRadianceParams) == 32
    assert "typedef struct pt_probe_radiance_filter" in header and C.sizeof(api.ProbeRadianceFilter) == 64
    assert "typedef struct pt_probe_radiance" in header and C.sizeof(api.ProbeRadiance) == 64
    methods = ("bake_probe_radiance", "probe_radiance_prefilter", "set_probe_grid_radiance", "set_probe_grid_radiance_sums", "probe_grid_radiance_info",
               "probe_grid_specular", "probe_radiance_dir")
    wrapper = open(os.path.join(ROOT, "include", "ptmi.hpp")).read()
    for method in methods:
        assert callable(getattr(api.Renderer, method))
        assert method + "(" in wrapper, method


def test_setter_refusals_and_their_order_change_nothing(api):
    r, _ = _renderer(api)
    L = r.L
    table = np.ones((24, 2, 16, 4), F)
    assert L.pt_set_probe_grid_radiance(r.ctx, C.byref(_rad_struct(api)), _p(table)) == STATE                              # no grid yet
    assert L.pt_set_probe_grid_radiance(r.ctx, None, None) == STATE                                                         # not even to clear
    assert L.pt_set_probe_grid_radiance(r.ctx, C.byref(_rad_struct(api, reserved=(0, 0, 0, 0, 0, 1))), _p(table)) == ARG   # reserved before the grid
    assert L.pt_set_probe_grid_radiance(r.ctx, None, _p(table)) == ARG                                                      # r before the grid
    g = PG.random_grid((3, 2, 4), 5, invalid=0.2, bias=0.25)
    g.set_on(r)
    assert L.pt_probe_grid_specular(r.ctx, 0, 0, None, None, None, None, None, None) == STATE                               # a grid, no radiance
    depth = PD.random_depth(g, 4, 6, vis_floor=0.05, facing=True)
    depth.set_on(r)
    rad = PR.random_radiance(g, 4, (0.2, 0.5), 7)
    rad.set_on(r)
    P, n, d, a = PR.query(g, 64, 6)
    before, diffuse = r.probe_grid_specular(P, n, d, a), r.probe_grid_lookup(P, n)
    info, dinfo, rinfo, scene = r.probe_grid_info(), r.probe_grid_depth_info(), r.probe_grid_radiance_info(), r.scene_info().as_dict()
    assert rinfo == (4, (float(F(0.2)), 0.5))
    assert_bit_equal(before[0], PR.specular(g, depth, rad, P, n, d, a)[0], "the radiance that is set")
    good = np.ones((24, 2, 16, 4), F)
    one = np.zeros(4, F)                 # never read past the checks: each of these is refused before a value is

    def bad(value, which=1):
        t = good.copy()
        t[17, 1, 9, which] = value
        return t
    nan, inf = float("nan"), float("inf")
    refusals = [
        (None, good, ARG),
        (dict(reserved=(1, 0, 0, 0, 0, 0)), good, ARG), (dict(reserved=(0, 0, 0, 0, 0, 7)), good, ARG),
        (dict(), None, ARG),
        (dict(res=1), one, LIMIT), (dict(res=17), one, LIMIT), (dict(res=0), one, LIMIT), (dict(res=0xFFFFFFFF), one, LIMIT),
        (dict(n_levels=0), one, LIMIT), (dict(n_levels=9), one, LIMIT),
        (dict(alphas=(0.0, 0.5)), one, ARG), (dict(alphas=(-0.1, 0.5)), one, ARG), (dict(alphas=(0.5, 0.5)), one, ARG), (dict(alphas=(0.5, 0.2)), one, ARG),
        (dict(alphas=(0.5, 1.5)), one, ARG), (dict(alphas=(nan, 0.5)), one, ARG), (dict(alphas=(0.5, inf)), one, ARG), (dict(alphas=(0.5, nan)), one, ARG),
        (dict(), bad(nan), ARG), (dict(), bad(inf, 0), ARG), (dict(), bad(-1.0), ARG), (dict(), bad(-inf, 2), ARG), (dict(), bad(nan, 3), ARG),
        # where several apply: r, the reserved words, the pointer, res, the levels, the alphas, the values last
        (dict(reserved=(0, 1, 0, 0, 0, 0), res=17), None, ARG), (dict(res=17), None, ARG), (dict(res=17, n_levels=9), one, LIMIT),
        (dict(res=17, alphas=(0.5, 0.2)), one, LIMIT), (dict(n_levels=9, alphas=(0.5, 0.2)), one, LIMIT), (dict(alphas=(0.5, 0.2)), bad(nan), ARG),
    ]
    for kw, tab, code in refusals:
        vs = None if kw is None else C.byref(_rad_struct(api, **kw))
        assert L.pt_set_probe_grid_radiance(r.ctx, vs, _p(tab)) == code, (kw, code)
        now = r.probe_grid_info()
        assert now[2:] == info[2:] and np.array_equal(now[0], info[0]) and r.probe_grid_depth_info() == dinfo
        assert r.probe_grid_radiance_info() == rinfo and r.scene_info().as_dict() == scene
        after = r.probe_grid_specular(P, n, d, a)
        assert_bit_equal(after[0], before[0], f"specular lookup after the refused call {kw}")
        assert np.array_equal(after[1], before[1])
        assert_bit_equal(r.probe_grid_lookup(P, n)[0], diffuse[0], f"lookup after the refused call {kw}")
    # an invalid node's values are checked as well ...
    first_invalid = int(np.flatnonzero(~g.valid.reshape(-1))[0])
    t = good.copy(); t[first_invalid, 0, 0, 0] = nan
    assert L.pt_set_probe_grid_radiance(r.ctx, C.byref(_rad_struct(api)), _p(t)) == ARG
    # ... a table above 2^31 bytes is refused before a value is read (256^3 nodes would be needed for a legal one: res 16, 8 levels here)
    big = PG.Grid((0, 0, 0), (1, 1, 1), (256, 256, 2), np.zeros((2, 256, 256, 9, 3), F))
    big.set_on(r)
    assert L.pt_set_probe_grid_radiance(r.ctx, C.byref(_rad_struct(api, res=16, alphas=ALPHAS8)), _p(one)) == LIMIT
    assert r.probe_grid_radiance_info() == (0, ())
    # zeros and alpha's upper end are legal; the lookup's own refusals
    g.set_on(r)
    zero = good.copy(); zero[3, 1, 2] = 0.0
    assert L.pt_set_probe_grid_radiance(r.ctx, C.byref(_rad_struct(api, alphas=(1.0,))), _p(zero[:, :1].copy())) == 0
    assert r.probe_grid_radiance_info() == (4, (1.0,))
    assert L.pt_get_probe_grid_radiance_info(r.ctx, None) == 0 and L.pt_get_probe_grid_radiance_info(None, None) == ARG
    out = np.zeros((2, 3), F); lit = np.zeros(2, np.uint8); q = np.zeros((2, 3), F); al = np.zeros(2, F)
    for k in range(6):
        args = [_p(q), _p(q), _p(q), _p(al), _p(out), _p(lit)]
        args[k] = None
        assert L.pt_probe_grid_specular(r.ctx, 0, 2, *args) == ARG
    assert L.pt_probe_grid_specular(r.ctx, 0, 0, None, None, None, None, None, None) == 0
    assert L.pt_probe_grid_specular(None, 0, 0, None, None, None, None, None, None) == ARG


def test_bake_refusals_are_the_depth_bakes_with_res(api):
    r, _ = _renderer(api)
    L = r.L
    pos = np.zeros((2, 3), F); sums = np.zeros((2, 16, 3), F); counts = np.zeros((2, 16), np.uint32)

    def prm(first=0, n=4, key=0, res=4, reserved=(0, 0, 0, 0)):
        return C.byref(api.ProbeRadianceParams(first, n, key, res, (C.c_uint32 * 4)(*reserved)))
    calls = [
        ((2, None, prm(), _p(sums), _p(counts)), ARG), ((2, _p(pos), None, _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(), None, _p(counts)), ARG), ((2, _p(pos), prm(), _p(sums), None), ARG),
        ((2, _p(pos), prm(n=0), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(key=0xFFFFFFFF), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(first=0xFFFFFFFF, n=2), _p(sums), _p(counts)), ARG),
        ((2, _p(pos), prm(res=1), _p(sums), _p(counts)), LIMIT), ((2, _p(pos), prm(res=17), _p(sums), _p(counts)), LIMIT),
        ((2, _p(pos), prm(res=0), _p(sums), _p(counts)), LIMIT),
        ((2, _p(pos), prm(reserved=(1, 0, 0, 0)), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(reserved=(0, 0, 0, 9)), _p(sums), _p(counts)), ARG),
        # the order: the census' own, then res, the reserved words
        ((2, _p(pos), prm(n=0, res=17), _p(sums), _p(counts)), ARG), ((2, _p(pos), prm(res=17, reserved=(1, 0, 0, 0)), _p(sums), _p(counts)), LIMIT),
    ]
    for args, code in calls:
        assert L.pt_bake_probe_radiance(r.ctx, *args) == code, code
    bad = pos.copy(); bad[1, 2] = np.nan
    assert L.pt_bake_probe_radiance(r.ctx, 2, _p(bad), prm(), _p(sums), _p(counts)) == ARG
    assert L.pt_bake_probe_radiance(r.ctx, 2, _p(bad), prm(res=17), _p(sums), _p(counts)) == ARG                 # the position before res
    assert L.pt_bake_probe_radiance(r.ctx, 0, None, None, None, None) == 0
    assert not sums.any() and not counts.any()
    # the direction hook
    t = np.arange(3, dtype=np.uint32); d = np.zeros((3, 3), F); om = np.zeros(3, F)
    for res in (0, 1, 17):
        assert L.pt_probe_radiance_dir(res, 3, _p(t), _p(d), _p(om)) == LIMIT
    assert L.pt_probe_radiance_dir(4, 3, None, _p(d), _p(om)) == ARG and L.pt_probe_radiance_dir(4, 3, _p(t), None, _p(om)) == ARG
    assert L.pt_probe_radiance_dir(4, 3, _p(t), _p(d), None) == ARG
    past = np.array([0, 16, 1], np.uint32)
    assert L.pt_probe_radiance_dir(4, 3, _p(past), _p(d), _p(om)) == ARG and not d.any() and not om.any()          # a texel past the map: nothing written
    assert L.pt_probe_radiance_dir(4, 0, None, None, None) == 0


def test_prefilter_refusals_and_their_order(api):
    r, _ = _renderer(api)
    L = r.L
    sums = np.ones((2, 16, 3), F); counts = np.ones((2, 16), np.uint32); table = np.full((2, 2, 16, 4), 7.0, F)
    nan, inf = float("nan"), float("inf")
    ok = (_p(sums), _p(counts), _p(table))
    calls = [
        (None, ok, ARG),
        (dict(reserved=(1, 0, 0, 0, 0)), ok, ARG), (dict(reserved=(0, 0, 0, 0, 3)), ok, ARG),
        (dict(res=1), ok, LIMIT), (dict(res=17), ok, LIMIT), (dict(res=0), ok, LIMIT),
        (dict(n_levels=0), ok, LIMIT), (dict(n_levels=9), ok, LIMIT),
        (dict(alphas=(0.0, 0.5)), ok, ARG), (dict(alphas=(0.5, 0.5)), ok, ARG), (dict(alphas=(0.7, 0.5)), ok, ARG), (dict(alphas=(0.5, 1.25)), ok, ARG),
        (dict(alphas=(nan, 0.5)), ok, ARG), (dict(alphas=(0.5, inf)), ok, ARG), (dict(alphas=(-0.5, 0.5)), ok, ARG),
        (dict(), (None, _p(counts), _p(table)), ARG), (dict(), (_p(sums), None, _p(table)), ARG), (dict(), (_p(sums), _p(counts), None), ARG),
        (dict(res=16, n_probes=1 << 17, alphas=ALPHAS8), ok, LIMIT),                  # 2^17 * 8 * 256 * 16 bytes = 2^32
        # the order: f, the reserved words, res, the levels, the alphas, the pointers, the size
        (dict(reserved=(1, 0, 0, 0, 0), res=17), ok, ARG), (dict(res=17, n_levels=9), ok, LIMIT), (dict(n_levels=9, alphas=(0.7, 0.5)), ok, LIMIT),
        (dict(alphas=(0.7, 0.5)), (None, None, None), ARG), (dict(res=17), (None, None, None), LIMIT),
        (dict(res=16, n_probes=1 << 17, alphas=ALPHAS8), (None, None, None), ARG),
    ]
    for on_device in (0, 1):            # refused before any device call: the same answers without a GPU
        for kw, ptrs, code in calls:
            fs = None if kw is None else C.byref(_filter_struct(api, **kw))
            assert L.pt_probe_radiance_prefilter(r.ctx, on_device, fs, *ptrs) == code, (kw, code)
            assert (table == 7.0).all()
        assert L.pt_probe_radiance_prefilter(r.ctx, on_device, C.byref(_filter_struct(api, n_probes=0)), None, None, None) == 0
    assert L.pt_probe_radiance_prefilter(None, 0, C.byref(_filter_struct(api)), *ok) == ARG


# ---------------------------------------------------------------------------------------------------------------------- the direction
@pytest.mark.parametrize("R", [2, 3, 8, 16])
def test_direction_is_the_restatement(api, R):
    r, _ = _renderer(api)
    d, om = r.probe_radiance_dir(R)
    wd, wom = PR.oct_dir(R)
    assert_bit_equal(d, wd, f"R {R}: directions")
    assert_bit_equal(om, wom, f"R {R}: omega")
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 2e-7
    assert np.abs(d.astype(np.float64) - PD.oct_centre_directions(R)).max() < 2e-7
    some = np.array([R * R - 1, 0, R], np.uint32)
    ds, oms = r.probe_radiance_dir(R, some)
    assert_bit_equal(ds, wd[some], "a list of texels")
    assert_bit_equal(oms, wom[some], "a list of texels")


@pytest.mark.parametrize("R", list(range(2, 17)))
def test_texel_of_a_texels_direction_is_the_texel(api, R):
    r, _ = _renderer(api)
    d, _ = r.probe_radiance_dir(R)
    assert np.array_equal(r.probe_depth_texel(d, R), np.arange(R * R))
    assert np.array_equal(PD.oct_texel(PR.oct_dir(R)[0], R), np.arange(R * R))


def test_omega_sums_to_the_sphere(api):
    """omega * 4 / R^2 is the texel's solid angle to first order: summed over the map it approaches 4 pi as R grows (the midpoint rule over
    the octahedron's faces, whose odd error terms cancel between a texel and its mirror image).  Observed relative errors of the float64
    sum of the float32 omegas, computed here from the library's own (pt_probe_radiance_dir, which are the restatement's bit for bit):
    R = 2: -9.97e-2 (each of the four centres sits on the fold line), R = 4: +1.52e-2, R = 8: +5.1e-5, R = 16: +1.75e-6.  A property of the
    definition; the prefilter divides by its own weights' sum, so the error does not reach it."""
    r, _ = _renderer(api)
    errs = {}
    for R in (2, 4, 8, 16):
        om = r.probe_radiance_dir(R)[1]
        assert_bit_equal(om, PR.oct_dir(R)[1], f"R {R}: omega")
        total = om.astype(np.float64).sum() * 4.0 / (R * R)
        errs[R] = total / (4.0 * np.pi) - 1.0
        print(f"R = {R}: sum(omega) * 4 / R^2 = {total:.6f}, relative error {errs[R]:+.3e}")
    assert abs(errs[16]) < 1.0e-5 and abs(errs[8]) < 1.0e-4
    assert abs(errs[16]) < abs(errs[8]) / 4.0 and abs(errs[8]) < abs(errs[4]) / 4.0 and abs(errs[4]) < abs(errs[2]) / 4.0   # second order in 1 / R at the least


# ---------------------------------------------------------------------------------------------------------------------- the prefilter
@pytest.mark.parametrize("R", [2, 3, 16])
@pytest.mark.parametrize("alphas", [(0.3,), ALPHAS8], ids=["1-level", "8-levels"])
@pytest.mark.parametrize("n", [1, 5])
def test_host_prefilter_is_the_restatement(api, R, alphas, n):
    r, _ = _renderer(api)
    sums, counts = PR.random_maps(n, R, 100 + R + n, empty=0.3)
    assert (counts == 0).any() and (counts > 0).any()
    got = r.probe_radiance_prefilter(sums, counts, alphas, on_device=False)
    assert_bit_equal(got, PR.prefilter(sums, counts, alphas), f"R {R}, {len(alphas)} levels, {n} probes")
    assert (got[..., 3] == 0).all() and np.isfinite(got).all() and (got >= 0).all()
    if R > 2:
        assert (got[..., :3] > 0).all()            # every lobe reaches some filled texel


def test_prefilter_of_an_empty_map_is_zeros_and_empty_texels_are_not_read(api):
    r, _ = _renderer(api)
    sums, counts = PR.random_maps(2, 8, 7, empty=0.4)
    got = r.probe_radiance_prefilter(sums, counts, ALPHAS5, on_device=False)
    junk = sums.copy(); junk[counts == 0] = np.nan
    assert_bit_equal(r.probe_radiance_prefilter(junk, counts, ALPHAS5, on_device=False), got, "what an empty texel's sums hold")
    none = np.zeros_like(counts)
    out = r.probe_radiance_prefilter(junk, none, ALPHAS5, on_device=False)
    assert not out.any() and out.shape == (2, 5, 64, 4)


@pytest.mark.parametrize("R", [2, 5, 16])
def test_furnace_a_constant_map_comes_back(api, R):
    """A / Wt with every mean the same c is c up to the rounding of the two running sums, and the bound is worked out per output texel from
    the weights that texel actually adds, in the order it adds them.  With u = 2^-24 and S_k the running sum after the k-th add, the k-th add
    is off by at most u * S_k, so the sum of the positive terms w_1..w_n is off by at most u * (S_2 + ... + S_n): relative to S_n that is
    u * rho with rho = (S_2 + ... + S_n) / S_n, which is n - 1 at the worst and far less where the lobe's peak comes late in j's order.
    A adds the same weights times c, each product off by a further factor within 1 +- u, the mean c = sums / count by one more, the
    quotient by one more: |A / Wt - c| <= (2 rho + 3) u c to first order.  rho is computed here in binary64 from the restated weights.
    Observed: 1 ulp of c at R = 2, 5 at R = 5, 18 at R = 16, where the largest texel's bound is about 2, 14 and 128 ulps and no texel uses
    more than 0.44, 0.35 and 0.27 of its own.  (The rest is the adds' errors not lining up, which no a-priori bound may count on.)"""
    r, _ = _renderer(api)
    rng = np.random.default_rng(3)
    c = np.array([0.75, 3.1, 0.0123], F)
    counts = rng.integers(1, 9, (1, R * R)).astype(np.uint32)
    sums = (c[None, None, :] * counts[..., None].astype(F)).astype(F)
    means = sums / counts[..., None].astype(F)
    got = r.probe_radiance_prefilter(sums, counts, ALPHAS8, on_device=False)[0, :, :, :3]          # [level, texel, channel]
    lo, hi = means.min(axis=(0, 1)), means.max(axis=(0, 1))                                       # (c itself, up to the mean's own rounding)
    u = 2.0 ** -24
    worst_ulps = worst_share = worst_bound = 0.0
    for l, alpha in enumerate(ALPHAS8):
        w, take = PR.prefilter_weights(R, alpha)
        w = np.where(take, w.astype(np.float64), 0.0)
        running = np.cumsum(w, axis=1)                                                            # S_k of every output texel, j ascending
        adds = take & (np.cumsum(take, axis=1) > 1)                                               # the first term is stored, not added
        rho = np.where(adds, running, 0.0).sum(axis=1) / running[:, -1]
        bound = (2.0 * rho + 3.0) * u                                                             # [texel]
        rel = np.maximum((got[l] - hi) / hi, (lo - got[l]) / lo).max(axis=1)
        assert (rel <= bound).all(), (alpha, float((rel / bound).max()))
        worst_share = max(worst_share, float((rel / bound).max())); worst_bound = max(worst_bound, float(bound.max()) / u / 2.0)
        worst_ulps = max(worst_ulps, float(np.maximum((got[l] - hi) / np.spacing(hi), (lo - got[l]) / np.spacing(hi)).max()))
    print(f"R = {R}: the constant map comes back within {worst_ulps:.1f} ulps; at most {worst_share:.2f} of a texel's own bound, the largest of which is "
          f"about {worst_bound:.0f} ulps")


def test_a_bright_texel_spreads_wider_at_larger_alpha(api):
    r, _ = _renderer(api)
    R = 16
    counts = np.ones((1, R * R), np.uint32)
    sums = np.zeros((1, R * R, 3), F)
    bright = 5 * R + 9
    sums[0, bright] = 1000.0
    got = r.probe_radiance_prefilter(sums, counts, ALPHAS5, on_device=False)[0, :, :, 0]         # [level, texel]
    dirs = PR.oct_dir(R)[0].astype(np.float64)
    cosine = dirs @ dirs[bright]
    peak = got[:, bright]
    assert (np.diff(peak) < 0).all(), peak                                          # the peak sinks ...
    om = PR.oct_dir(R)[1].astype(np.float64)
    spread = (got * om * (1.0 - cosine)).sum(axis=1) / (got * om).sum(axis=1)       # the image's mean 1 - cos about the bright direction
    print("peak per level", peak, "mean 1 - cos per level", spread)
    assert (np.diff(spread) > 0).all(), spread                                      # ... and the image spreads, level by level
    far = got[:, (cosine < 0.5) & (cosine > 0.05)].mean(axis=1)
    assert (np.diff(far) > 0).all(), far                                            # ... into the skirt beyond 60 degrees
    half = [(got[l] > 0.5 * peak[l]).sum() for l in range(5)]
    assert all(half[l] <= half[l + 1] for l in range(4)) and half[0] < half[4], half
    assert (got[:, cosine < -1e-3] == 0).all()                                      # and nothing reaches the far hemisphere (nl <= 0)


# ------------------------------------------------------------------------------------------------------------------------- the lookup
@pytest.mark.parametrize("count", PG.COUNTS)
@pytest.mark.parametrize("alphas", [(0.35,), ALPHAS5], ids=["1-level", "5-levels"])
def test_host_lookup_is_the_restatement(api, count, alphas):
    r, _ = _renderer(api)
    checked = 0
    for bias, invalid in ((0.0, 0.0), (0.375, 0.25)):
        g = PG.random_grid(count, 11 + sum(count), invalid=invalid, bias=bias)
        g.set_on(r)
        P, n, d, a = PR.query(g, 300, 12)
        # alpha below, between, on and above the levels, and a NaN; a NaN direction and a zero one
        a[:8] = [0.0, -1.0, alphas[0], alphas[-1], 1.5, np.nan, np.inf, (alphas[0] + alphas[-1]) / 2]
        for k, al in enumerate(alphas):
            a[8 + k] = al
        d[20] = np.nan; d[21] = 0.0; n[22] = np.nan
        for R in (2, 5):
            rad = PR.random_radiance(g, R, alphas, 13 + R)
            for depth in (None, PD.random_depth(g, 4, 14, 0.05, True), PD.random_depth(g, 3, 15, 0.0, False, consistent=False)):
                r.set_probe_grid_depth(None)
                if depth is not None:
                    depth.set_on(r)
                rad.set_on(r)
                want, want_lit = PR.specular(g, depth, rad, P, n, d, a)
                got, lit = r.probe_grid_specular(P, n, d, a)
                assert_bit_equal(got, want, f"{count}, R {R}, bias {bias}, depth {depth is not None}")
                assert np.array_equal(lit, want_lit)
                checked += 1
    assert checked == 12


def test_level_selection_and_blend(api):
    r, _ = _renderer(api)
    g = PG.random_grid((1, 1, 1), 3)
    g.set_on(r)
    R = 4
    t = np.zeros((1, 3, R * R, 4), F)
    t[0, 0, :, :3] = 1.0; t[0, 1, :, :3] = 3.0; t[0, 2, :, :3] = 11.0
    PR.Radiance(t, (0.25, 0.5, 1.0)).set_on(r)
    a = np.array([0.0, 0.25, 0.375, 0.5, 0.75, 1.0, 2.0, np.nan, 0.3125], F)
    k = len(a)
    P = np.zeros((k, 3), F); n = np.tile(np.array([0, 0, 1], F), (k, 1)); d = np.tile(np.array([0, 0, -1], F), (k, 1))
    got, lit = r.probe_grid_specular(P, n, d, a)
    assert lit.all()
    assert got[:, 0].tolist() == [1.0, 1.0, 2.0, 3.0, 7.0, 11.0, 11.0, 1.0, 1.5]     # (1 - t) * lower + t * upper: swapped, 0.3125 gives 2.5


@pytest.mark.parametrize("count", PG.COUNTS)
def test_the_two_exact_cases(api, count):
    r, _ = _renderer(api)
    # a 1 x 1 x 1 grid with one level returns its table entry of the texel bit for bit, everywhere
    g1 = PG.random_grid((1, 1, 1), 41, bias=0.125)
    g1.set_on(r)
    for R in (2, 7):
        rad = PR.random_radiance(g1, R, (0.4,), 42 + R)
        rad.set_on(r)
        P, n, d, a = PR.query(g1, 200, 43)
        got, lit = r.probe_grid_specular(P, n, d, a)
        texel = PD.oct_texel(PR.reflect(d, n), R)
        assert lit.all()
        assert_bit_equal(got, rad.table[0, 0, texel, :3], f"1 x 1 x 1, R {R}")
    # a valid node's own position with t = 0 returns that node's entry: alpha on a level, whatever the depth
    g = PG.random_grid(count, 23 + sum(count))
    g.set_on(r)
    nodes = g.nodes().reshape(-1, 3)
    rad = PR.random_radiance(g, 4, ALPHAS5, 44)
    for depth in (None, PD.random_depth(g, 4, 24, 0.0, True)):
        if depth is not None:
            depth.set_on(r)
        rad.set_on(r)
        for level, alpha in ((0, 0.05), (2, ALPHAS5[2]), (4, 1.0), (4, 3.0)):
            d = PG.unit_normals(len(nodes), 45 + level); n = PG.unit_normals(len(nodes), 46)
            got, lit = r.probe_grid_specular(nodes, n, d, alpha)
            texel = PD.oct_texel(PR.reflect(d, n), 4)
            assert lit.all()
            assert_bit_equal(got, rad.table[np.arange(len(nodes)), level, texel, :3], f"{count}: nodes, level {level}, depth {depth is not None}")


def test_invalid_nodes_values_never_reach_the_result(api):
    r, _ = _renderer(api)
    g = PG.random_grid((3, 2, 4), 17, invalid=0.35)
    assert 4 < g.valid.sum() < 20
    g.set_on(r)
    P, n, d, a = PR.query(g, 400, 18)
    rad = PR.random_radiance(g, 4, ALPHAS5, 19)
    rad.set_on(r)
    got, lit = r.probe_grid_specular(P, n, d, a)
    assert_bit_equal(got, PR.specular(g, None, rad, P, n, d, a)[0], "with invalid nodes")
    other = rad.table.copy()
    dead = ~g.valid.reshape(-1)
    other[dead] = np.random.default_rng(20).uniform(0.0, 50.0, other[dead].shape).astype(F)
    PR.Radiance(other, ALPHAS5).set_on(r)
    again = r.probe_grid_specular(P, n, d, a)
    assert_bit_equal(again[0], got, "invalid nodes' values changed")
    assert np.array_equal(again[1], lit)
    # where every corner is invalid the lookup is not lit and returns zeros
    assert (got[lit == 0] == 0).all()
    none = PG.Grid(g.origin, g.cell, g.count, g.sh, np.zeros_like(g.valid))
    none.set_on(r); rad.set_on(r)
    got, lit = r.probe_grid_specular(P, n, d, a)
    assert not lit.any() and not got.any()


# ------------------------------------------------------------------------------------------------------------------------ the lifetime
def test_radiance_lives_with_its_grid(api):
    r, sc = _renderer(api)
    _, model = LC.cornell_atlas_scene()
    g = PG.random_grid((3, 2, 4), 37, invalid=0.2)
    g.set_on(r)
    assert r.probe_grid_radiance_info() == (0, ())
    rad = PR.random_radiance(g, 8, (0.25, 0.5), 38)
    rad.set_on(r)
    P, n, d, a = PR.query(g, 100, 39)
    before = r.probe_grid_specular(P, n, d, a)
    diffuse = r.probe_grid_lookup(P, n)
    assert r.probe_grid_radiance_info() == (8, (0.25, 0.5))
    assert_bit_equal(diffuse[0], PG.lookup(g, P, n)[0], "radiance leaves the diffuse lookup alone")

    def same(what):
        now = r.probe_grid_specular(P, n, d, a)
        assert_bit_equal(now[0], before[0], what)
        assert np.array_equal(now[1], before[1]) and r.probe_grid_radiance_info() == (8, (0.25, 0.5)), what
    r.rebuild(); same("pt_build")
    moved = np.array([[1, 0, 0, 0.5, 0, 1, 0, 0.25, 0, 0, 1, -0.5]], F).reshape(1, 3, 4)
    r.set_instances(model, moved); r.rebuild(); same("pt_set_instances")
    r.set_lightmap(model, 0, np.ones((2, 2, 3), F)); same("pt_set_lightmap")
    # depth set and cleared leaves radiance in place (and changes its weights in between)
    depth = PD.random_depth(g, 4, 40, 0.0, True)
    depth.set_on(r)
    assert r.probe_grid_radiance_info() == (8, (0.25, 0.5))
    assert_bit_equal(r.probe_grid_specular(P, n, d, a)[0], PR.specular(g, depth, rad, P, n, d, a)[0], "depth under radiance")
    r.set_probe_grid_depth(None); same("depth cleared")
    # clearing radiance: the lookup is refused again, the grid still there; clearing what is not there is fine
    r.set_probe_grid_radiance(None)
    assert r.probe_grid_radiance_info() == (0, ()) and r.probe_grid_info()[2] == (3, 2, 4)
    with pytest.raises(api.PtError):
        r.probe_grid_specular(P, n, d, a)
    r.set_probe_grid_radiance(None)
    # ANY pt_set_probe_grid drops radiance: the same grid again, and the clearing call
    rad.set_on(r); same("set again")
    g.set_on(r)
    assert r.probe_grid_radiance_info() == (0, ())
    rad.set_on(r)
    r.set_probe_grid(None, None, None)
    assert r.probe_grid_radiance_info() == (0, ())
    with pytest.raises(api.PtError):
        rad.set_on(r)                                                              # no grid: nothing to set radiance on
    # the wrapper's shape check, and through the sums
    g.set_on(r)
    with pytest.raises(api.PtError):
        r.set_probe_grid_radiance(np.ones((23, 2, 64, 4), F), (0.25, 0.5))
    with pytest.raises(api.PtError):
        r.set_probe_grid_radiance(np.ones((24, 2, 64, 4), F))                      # a table without its alphas
    sums, counts = PR.random_maps(24, 4, 50)
    table = r.set_probe_grid_radiance_sums(sums, counts, ALPHAS5, on_device=False)
    assert r.probe_grid_radiance_info() == (4, tuple(float(F(x)) for x in ALPHAS5))
    assert_bit_equal(table, PR.prefilter(sums, counts, ALPHAS5), "the table set from sums")
    assert_bit_equal(r.probe_grid_specular(P, n, d, a)[0], PR.specular(g, None, PR.Radiance(table, ALPHAS5), P, n, d, a)[0], "through the sums")


# ------------------------------------------------------------------------------------------------------- the restatements' own footing
def test_restated_view_without_radiance_is_the_probe_endings_view(oracle_mod):
    """probe_radiance_common.baked with rad None walks the chain that probe_depth_common.baked walks and must give its bits and its endings:
    the GPU tests' "without radiance" side rests on it.  Section 22's room with its panel made metal, with depth and without, K = 0 and 2."""
    import baked_common as BC
    import guides_follow_common as G
    from path_tracer_amd.scene_desc import GGX
    W, H, unlit = 37, 19, (0.25, 0.5, 0.125)
    sc, maps = BC.mapped_room(W, H)
    sc.models[BC.MAPPED_MODELS.index("panel")].material = GGX.new_metal((0.6, 0.9, 0.5), 0.6)
    orc = oracle_mod.Oracle(sc)
    grid = PG.room_grid()
    o, d = G.pinhole_rays(orc, W, H, 3)
    for depth in (None, PD.random_depth(grid, 4, 61, 0.0, True)):
        for hops in (0, 2):
            B, ending, on_metal = PR.baked(orc, sc, maps, grid, depth, None, o, d, hops, unlit)
            wantB, want_ending = PD.baked(orc, sc, maps, grid, depth, o, d, hops, unlit)
            assert_bit_equal(B, wantB, f"depth {depth is not None}, K = {hops}")
            assert np.array_equal(ending, want_ending) and on_metal.sum() > 100
            # with radiance the metal pixels that the specular lookup lights change, and nothing else does
            Bs, es, _ = PR.baked(orc, sc, maps, grid, depth, PR.random_radiance(grid, 8, ALPHAS5, 63), o, d, hops, unlit)
            shiny = np.isin(es, (PR.METAL_FRONT, PR.METAL_BACK))
            assert shiny.sum() > 100 and (on_metal | ~shiny).all() and np.array_equal(es[~shiny], ending[~shiny])
            assert np.array_equal(Bs[~shiny].view(np.uint32), B[~shiny].view(np.uint32))
            assert (on_metal & ~shiny & np.isin(es, (PG.UNLIT_UNMAPPED, PG.UNLIT_BACK))).any()     # metal that the grid does not light


def test_the_pictures_figure_is_what_the_derivation_gives(api, oracle_mod):
    """RADIANCE_FIGURE and DIFFUSE_FIGURE are typed in from probe_radiance_common's derivation at 4 096 paths a point.  Here the derivation
    runs again with 512 and must land on the constants within the noise it measures itself: three standard errors of the difference, the
    512-path run's sigma and the constant's (the same sigma over the root of 8) added in quadrature.  Observed: 0.1407 and 0.8954 against
    0.1469 and 0.9070, with sigmas of 0.018 and 0.027: a third of one standard error each."""
    sc = PR.e2e_scene()
    res, n_valid, sigma = PR.radiance_figure(oracle_mod.Oracle(sc), api.Renderer(sc, PG.E2E_W, PG.E2E_H), sc, paths=512)
    assert n_valid == 61
    for name, constant in (("radiance", PR.RADIANCE_FIGURE), ("diffuse", PR.DIFFUSE_FIGURE)):
        figure, tol = res[name][0], 3.0 * sigma[name] * np.sqrt(1.0 + 1.0 / 8.0)
        print(f"{name}: {figure:.4f} at 512 paths a point, the constant {constant:.4f}, one standard error {sigma[name]:.4f}, allowed {tol:.4f}")
        assert abs(figure - constant) <= tol
    assert sum(k for k, _, _ in res["radiance"][2].values()) == 43 and len(res["radiance"][2]) == 2
    assert res["diffuse"][0] - 3.0 * sigma["diffuse"] > 2.0 * PR.RADIANCE_FIGURE    # the diffuse metal misses the bound, beyond the noise
