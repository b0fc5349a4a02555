"""CPU: the options of the temporal stage (pt_temporal_options' rescue, length_rule, demodulate).  temporal_options_common restates their
definition (include/pt_api.h, steps 3, 3b, 4 and the demodulation) in numpy float32; pt_post_temporal_options(on_device = 0) evaluates the
library's per-pixel function (csrc/pt_temporal.h, the one the kernels run) on the host.  Here: the two agree bit for bit on cases that reach
every edge of the definition (a test of its own asserts that they do), both obey its closed forms, every refusal arrives before any device
call and changes nothing, and the plain calls refuse what they refused.  tests/test_gpu_temporal_options.py holds the device to the same."""
import ctypes as C
import os

import numpy as np
import pytest

import temporal_common as plain
from conftest import ROOT, assert_bit_equal
from temporal_options_common import F, MISS, fractions, options_case, plane, post_temporal, reproject

SIZES = [(1, 1), (5, 3), (16, 16), (37, 29)]
OPTIONS = [dict(rescue=1), dict(length_rule=1), dict(rescue=1, length_rule=1)]
IDS = ["rescue", "mean", "both"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def renderer(api):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    yield r
    r.close()


def both(renderer, prev, cur, what, **kw):
    """the restatement's and the host path's (H, M, variance), after asserting that they are the same bits"""
    want = post_temporal(prev, cur, **kw)
    got = renderer.post_temporal(prev, cur, on_device=False, **kw)
    for a, b, name in zip(got, want, ("history", "moments", "variance")):
        assert_bit_equal(a, b, f"{what}: {name}")
    return want


def modes(xprev, nprev, vel):
    return {"velocity": dict(xprev=xprev, nprev=nprev, velocity=vel), "rest": dict(xprev=xprev, nprev=nprev), "plain": dict(velocity=vel)}


def test_the_interface(api):
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for name in ("pt_frame_temporal_options", "pt_post_temporal_options"):
        assert name in api.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    struct = header.split("typedef struct pt_temporal_options")[1].split("} pt_temporal_options;")[0]
    names = [n for n, _ in api.TemporalOptions._fields_]
    assert names == ["rescue", "length_rule", "demodulate", "reserved"] and C.sizeof(api.TemporalOptions) == 16
    for n in names:
        assert f" {n};" in struct
    assert "PT_TEMPORAL_LENGTH_MIN = 0, PT_TEMPORAL_LENGTH_MEAN = 1" in header
    assert C.sizeof(api.TemporalParams) == 32 and api.TemporalParams._fields_[-1][0] == "reserved"     # the parameters are what they were
    assert (api.TEMPORAL_LENGTH_MIN, api.TEMPORAL_LENGTH_MEAN) == (0, 1)
    import inspect
    for f in (api.Renderer.frame_temporal, api.Renderer.post_temporal):
        sig = inspect.signature(f).parameters
        assert all(sig[n].default == 0 for n in ("rescue", "length_rule", "demodulate"))


# ---------------------------------------------------------------- the host path is the restatement
def test_with_no_option_the_restatement_is_the_plain_one(oracle_mod):
    for w, h in SIZES:
        prev, cur, xprev, nprev, vel = options_case(np.random.default_rng(7 * w + h), w, h)
        for kw in modes(xprev, nprev, vel).values():
            for a, b in zip(post_temporal(prev, cur, **kw), plain.post_temporal(prev, cur, **kw)):
                assert_bit_equal(a, b, f"{w}x{h}")


@pytest.mark.parametrize("opt", OPTIONS, ids=IDS)
@pytest.mark.parametrize("mode", ["velocity", "rest", "plain"])
@pytest.mark.parametrize("wh", SIZES)
def test_host_path_equals_the_restatement(oracle_mod, renderer, wh, mode, opt):
    w, h = wh
    rescued = 0
    for seed in range(3):
        make = options_case if seed < 2 else plain.random_case
        prev, cur, xprev, nprev, vel = make(np.random.default_rng(100 * w + seed), w, h)
        kw = dict(modes(xprev, nprev, vel)[mode], **opt)
        both(renderer, prev, cur, f"{w}x{h} {mode} seed {seed}", **kw)
        st = {}
        reproject(prev, cur, stats=st, **{k: v for k, v in kw.items()})
        rescued += int((st["rescue_taps"] > 0).sum())
        if seed == 0:   # other parameters than the defaults
            both(renderer, prev, cur, f"{w}x{h} {mode} parameters", alpha=0.5, alpha_moments=0.05, normal_min=-1.0, plane_max=0.5, sigma_normal=8,
                 sigma_plane=0.25, **kw)
    if w * h > 64 and opt.get("rescue"):
        assert rescued > 0


def test_the_cases_reach_the_edges(oracle_mod):
    """what the comparison above rests on; every line is a condition of the definition, none a measurement"""
    w, h = 37, 29
    seen = dict(one=0, several=0, none=0, minus=0, at_w=0, rest_model=0, nan=0, inf=0, out=0)
    for seed in range(2):
        prev, cur, xprev, nprev, vel = options_case(np.random.default_rng(100 * w + seed), w, h)
        st = {}
        cn, _, _ = reproject(prev, cur, xprev, nprev, vel, rescue=1, length_rule=1, stats=st)
        lost, k = st["lost"], st["rescue_taps"]
        seen["one"] += int((lost & (k == 1)).sum()); seen["several"] += int((lost & (k > 1)).sum())
        none = lost & (k == 0)
        seen["none"] += int(none.sum())
        assert (cn[none][:, 3] == 1).all() and np.array_equal(cn[none][:, :3], cur[0][none][:, :3])   # nine failures: a restart
        cx = st["centre"][0]
        seen["minus"] += int((lost & (cx == -1)).sum()); seen["at_w"] += int((lost & (cx == w)).sum())
        # no list, no rescue: NaN, infinite and out-of-frame velocities restart whatever stands around them
        unlisted = ~st["listed"]
        assert (k[unlisted] == 0).all() and (cn[unlisted][:, 3] == 1).all() and not lost[unlisted].any()
        seen["nan"] += int((unlisted & np.isnan(vel).any(-1)).sum()); seen["inf"] += int((unlisted & np.isinf(vel).any(-1)).sum())
        seen["out"] += int((unlisted & np.isfinite(vel).all(-1)).sum())
        # at rest: the pixel's own tap fails on the model word and a neighbour's record rescues it
        sr = {}
        reproject(prev, cur, xprev, nprev, None, rescue=1, stats=sr)
        seen["rest_model"] += int((sr["lost"] & (sr["rescue_taps"] > 0) & (prev[4] != cur[3]) & (prev[0][..., 3] > 0)).sum())
        # both ends of N stand in the history and come out of the mean rule
        for n in (65534, 65535):
            assert (prev[0][..., 3] == n).any()
        assert (cn[..., 3] == 65535).any()
    assert all(v > 0 for v in seen.values()), seen
    # tx and ty exactly 0.5: a power-of-two frame and half-pixel velocities
    prev, cur, xprev, nprev, vel = options_case(np.random.default_rng(1600), 16, 16)
    _, _, tx, ty, listed = fractions(16, 16, vel)
    assert (listed & (tx == F(0.5))).any() and (listed & (ty == F(0.5))).any() and (listed & (tx == F(0.5)) & (ty == F(0.5))).any()


def _uniform(w, h, n):
    pos, nrm, model = plane(w, h)
    rng = np.random.default_rng(w + h)
    H = np.concatenate([rng.random((h, w, 3)).astype(F), np.asarray(n, F).reshape(h, w, 1)], -1).astype(F)
    M = rng.random((h, w, 2)).astype(F)
    cur = (np.concatenate([rng.random((h, w, 3)).astype(F), np.ones((h, w, 1), F)], -1), pos, nrm, model)
    return (H, M, pos.copy(), nrm.copy(), model.copy()), cur


def test_mean_lengths_that_land_on_a_half(oracle_mod, renderer):
    """16 x 16, velocity half a pixel: fx = x - 0.5 exactly, two taps of weight 0.5.  Columns of N = 1, 2, 1, 2 .. give sN / sw = 1.5 exactly,
    which + 0.5 floors to 2: N = 3; and the closed form of the issue: between N = 1 and N = 9 the mean rule gives 6 where Nmin gives 2"""
    w = h = 16
    vel = np.zeros((h, w, 2), F); vel[..., 0] = F(0.5) / F(w)
    for lo, hi, mean_n in ((1, 2, 3), (1, 9, 6), (65534, 65535, 65535), (65535, 65535, 65535)):
        n = np.where(np.arange(w)[None, :] % 2 == 0, lo, hi) * np.ones((h, 1))
        prev, cur = _uniform(w, h, n)
        st = {}
        reproject(prev, cur, velocity=vel, length_rule=1, stats=st)
        inner = np.s_[:, 1:]
        if lo != hi:
            assert (st["mean_length"][inner] == F(lo + hi) / F(2)).all()                # exactly x.5 where lo + hi is odd
        Hm, _, _ = both(renderer, prev, cur, f"mean of {lo} and {hi}", velocity=vel, length_rule=1)
        Hn, _, _ = both(renderer, prev, cur, f"least of {lo} and {hi}", velocity=vel)
        assert (Hm[inner][..., 3] == mean_n).all() and (Hn[inner][..., 3] == min(lo + 1, 65535)).all()
        assert (Hm[:, 0, 3] == min(n[0, 0] + 1, 65535)).all()                           # the first column has one tap, of weight 0.5


def test_equal_lengths_one_ulp_below_are_not_frozen(oracle_mod, renderer):
    """the case the + 0.5f exists for: four taps of one N whose f32 fold gives sN / sw below N.  A bare floor would hand back N, not N + 1"""
    w = h = 16
    rng = np.random.default_rng(99)
    found = 0
    for n in (3, 7, 11, 25, 1000):
        vel = ((rng.random((h, w, 2)) * 0.98 + 0.01) / np.array([w, h])).astype(F)
        prev, cur = _uniform(w, h, np.full((h, w), n))
        st = {}
        reproject(prev, cur, velocity=vel, length_rule=1, stats=st)
        below = st["mean_length"] < F(n)
        found += int(below.sum())
        Hm, _, _ = both(renderer, prev, cur, f"equal N = {n}", velocity=vel, length_rule=1)
        Hn, _, _ = both(renderer, prev, cur, f"equal N = {n}, least", velocity=vel)
        assert_bit_equal(Hm, Hn, "taps of equal N: the two rules agree")
        assert (Hm[~st["restarted"]][:, 3] == n + 1).all()
    assert found > 0


def test_at_rest_with_every_tap_valid_the_options_change_no_bit(oracle_mod, renderer):
    w, h = 13, 9
    prev, cur = _uniform(w, h, np.random.default_rng(4).integers(1, 50, (h, w)))
    base = both(renderer, prev, cur, "plain")
    for opt in OPTIONS:
        for a, b in zip(both(renderer, prev, cur, str(opt), **opt), base):
            assert_bit_equal(a, b, str(opt))


def test_a_rest_pixel_is_rescued_by_its_neighbour(oracle_mod, renderer):
    """5 x 3, the frame smaller than a rescue window's reach: the centre pixel's record is of another model; at rest its 3 x 3 holds eight valid
    taps of weight 1, so the history is their mean in list order and N their least plus one"""
    w, h = 5, 3
    prev, cur = _uniform(w, h, np.arange(2, 17).reshape(h, w))
    prev[4][1, 2] = 7
    H, M, _ = both(renderer, prev, cur, "rescued", rescue=1)
    P, _, _ = both(renderer, prev, cur, "not rescued")
    assert P[1, 2, 3] == 1 and H[1, 2, 3] == prev[0][0, 1, 3] + 1
    s = np.zeros(3, F)
    for dy in (0, 1, 2):
        for dx in (1, 2, 3):
            if (dy, dx) != (1, 2):
                s = (s + prev[0][dy, dx, :3]).astype(F)
    a = F(1) / H[1, 2, 3]
    a = a if a > F(0.2) else F(0.2)
    assert_bit_equal(H[1, 2, :3], ((s / F(8)) * (F(1) - a) + cur[0][1, 2, :3] * a).astype(F), "the mean of eight")
    keep = np.ones((h, w), bool); keep[1, 2] = False
    assert_bit_equal(H[keep], P[keep], "nobody else walks")


# ---------------------------------------------------------------- refusals: before any device call, changing nothing
def _post(api, r, to, w=3, h=2, paths=(0, 1)):
    H = np.ones((h, w, 4), F); M = np.ones((h, w, 2), F); X = np.zeros((h, w, 4), F)
    n3 = np.zeros((h, w, 3), F); mdl = np.zeros((h, w), np.uint32)
    outs = [np.full((h, w, 4), 7, F), np.full((h, w, 2), 7, F), np.full((h, w), 7, F)]
    ins = [H, M, X, n3, mdl, H.copy(), X.copy(), n3.copy(), mdl.copy()]
    d = api.DenoiseParams(); tp = api.TemporalParams()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = [r.L.pt_post_temporal_options(r.ctx, dev, w, h, C.byref(tp), None if to is None else C.byref(to), C.byref(d), *[ptr(a) for a in ins], None, None, None,
                                       *[ptr(a) for a in outs]) for dev in paths]
    return rc, all((o == 7).all() for o in outs)


@pytest.mark.parametrize("words", [(2, 0, 0), (0, 2, 0), (0, 0, 2), (0xffffffff, 0, 0), (0, 7, 0), (1, 1, 9), (1, 1, 0, 1), None])
def test_a_word_above_one_is_refused(api, renderer, words):
    """and a non-zero reserved word, and NULL options"""
    to = None if words is None else api.TemporalOptions(*words)
    rc, untouched = _post(api, renderer, to)
    assert rc == [-1, -1] and untouched and "pt_temporal_options" in renderer.L.pt_last_error(renderer.ctx).decode()
    d = api.DenoiseParams(); tp = api.TemporalParams()
    assert renderer.L.pt_frame_temporal_options(renderer.ctx, 0, None, C.byref(tp), None if to is None else C.byref(to), C.byref(d), None, None, None, None) == -1
    assert renderer.L.pt_read_temporal(renderer.ctx, None, None, None) == -3      # and nothing became a history


def test_the_plain_calls_refuse_what_they_refused(api, renderer):
    """pt_temporal_params' reserved words stay reserved, and the parameters are checked before the options"""
    d = api.DenoiseParams(); ok = api.TemporalOptions(1, 1, 0)
    for words in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        tp = api.TemporalParams(0, 0, 0, 0, 0, words)
        for f in (renderer.L.pt_frame_temporal, renderer.L.pt_frame_temporal_options):
            args = (C.byref(tp), C.byref(d)) if f is renderer.L.pt_frame_temporal else (C.byref(tp), C.byref(ok), C.byref(d))
            assert f(renderer.ctx, 0, None, *args, None, None, None, None) == -1 and "reserved" in renderer.L.pt_last_error(renderer.ctx).decode()
    bad = api.TemporalParams(2.0)
    assert renderer.L.pt_frame_temporal_options(renderer.ctx, 0, None, C.byref(bad), C.byref(api.TemporalOptions(2)), C.byref(d), None, None, None, None) == -1
    assert "pt_temporal_params.alpha" in renderer.L.pt_last_error(renderer.ctx).decode()


def test_post_temporal_refuses_to_demodulate_and_honours_the_rest(api, renderer):
    for words in ((0, 0, 1), (1, 1, 1)):
        rc, untouched = _post(api, renderer, api.TemporalOptions(*words))
        assert rc == [-1, -1] and untouched and "demodulate" in renderer.L.pt_last_error(renderer.ctx).decode()
    with pytest.raises(api.PtError) as e:
        renderer.post_temporal(plain.empty_state(3, 2), (np.ones((2, 3, 4), F),) + plane(3, 2), demodulate=1)
    assert e.value.code == -1
    rc, untouched = _post(api, renderer, api.TemporalOptions(1, 1, 0), paths=(0,))
    assert rc[0] == 0 and not untouched          # the host path ran (the device path is tests/test_gpu_temporal_options.py's)
