"""numpy restatement of the texel criterion of include/pt_api.h (pt_bake_lightmap_adaptive): binary32, one rounding per operation, in the
header's order.  Also the synthetic states whose covered texels sit on the criterion's edges, and the maps the host and the GPU tests share.
Nothing here calls the library under test."""
import numpy as np

import lightmap_common as LC

F = np.float32
LIMIT_COUNT = 1 << 24


def terms(sums, sumsq, counts, rel_error, abs_floor):
    """(m, e2, t) of every texel, float32 [h, w]; a count of 0 gives NaNs, as in the library"""
    s = np.asarray(sums, F)
    with np.errstate(all="ignore"):
        n = np.asarray(counts, np.uint32).astype(F)
        S = (F(0.2126) * s[..., 0] + F(0.7152) * s[..., 1]) + F(0.0722) * s[..., 2]
        m = S / n
        v = np.asarray(sumsq, F) / n - m * m
        v = np.where(v > 0, v, F(0))
        e2 = v / n
        t = F(rel_error) * np.where(m > F(abs_floor), m, F(abs_floor))
    assert m.dtype == F and e2.dtype == F and t.dtype == F
    return m, e2, t


def active(sums, sumsq, counts, covered, rel_error, abs_floor=0.0, min_samples=2, max_samples=0):
    """bool [h, w]: the texels pt_bake_lightmap_adaptive selects"""
    c = np.asarray(counts, np.uint32)
    _, e2, t = terms(sums, sumsq, c, rel_error, abs_floor)
    with np.errstate(all="ignore"):
        noisy = e2 > t * t
    more = (c < min_samples) | (((max_samples == 0) | (c < max_samples)) & noisy)
    return np.asarray(covered, bool) & more


def relative_error(sums, sumsq, counts, abs_floor):
    """sqrt(e2) / max(m, abs_floor) per texel in binary64 from the binary32 terms: what a threshold is chosen from"""
    m, e2, _ = terms(sums, sumsq, counts, 1.0, abs_floor)
    return np.sqrt(e2.astype(np.float64)) / np.maximum(m.astype(np.float64), float(abs_floor))


# ---- the states on the criterion's edges.  EDGE_CRIT's rel_error is a power of two and "equal" has 16 samples, so that e2 == t * t can be hit
# exactly: t = m / 4 and t * t = fl(m * m) / 16 without a second rounding, e2 = v / 16 exactly, so Q = 32 * fl(m * m) makes v = fl(m * m).
EDGE_CRIT = dict(rel_error=0.25, abs_floor=0.5, min_samples=4, max_samples=32)
CRITS = [EDGE_CRIT, dict(EDGE_CRIT, max_samples=0), dict(EDGE_CRIT, rel_error=0.0), dict(EDGE_CRIT, abs_floor=0.0), dict(rel_error=0.0, abs_floor=0.0, min_samples=2, max_samples=0)]
EDGES = ["count_0", "below_min", "at_min_flat", "at_min_noisy", "below_max", "at_max", "v_negative", "under_floor", "over_floor", "equal", "just_above", "random"]


def _texel(edge, rng):
    """(rgb sums, Q, count) of one covered texel on `edge` under EDGE_CRIT"""
    mn, mx = EDGE_CRIT["min_samples"], EDGE_CRIT["max_samples"]
    lum = lambda c: (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]
    mean = rng.uniform(1.0, 2.0, 3).astype(F)

    def state(n, mean, spread):
        """n samples of colour `mean` whose luminance has variance `spread`"""
        l = lum(mean)
        return mean * F(n), (l * l + F(spread)) * F(n), n

    if edge == "count_0":
        return np.zeros(3, F), F(0), 0
    if edge == "below_min":
        return state(mn - 1, mean, 0.0)
    if edge == "at_min_flat":
        return state(mn, mean, 0.0)[0], F(0), mn                     # Q = 0: v is negative and clamps, the texel has converged
    if edge == "at_min_noisy":
        return state(mn, mean, 4.0)
    if edge == "below_max":
        return state(mx - 1, mean, 40.0)
    if edge == "at_max":
        return state(mx, mean, 40.0)
    if edge == "v_negative":
        s, q, n = state(16, mean, 0.0)
        return s, np.nextafter(q, F(0)) * F(0.999), n                # Q / n below m * m
    if edge == "under_floor":
        # m = 0.1 under the floor of 0.5: e2 = 0.04 / 16 lies between (0.25 * 0.1)^2 and (0.25 * 0.5)^2, so only the floor keeps it inactive
        return state(16, np.full(3, 0.1, F), 0.04)
    if edge == "over_floor":
        return state(16, mean, 8.0)                                  # m in [1, 2] is above the floor: e2 = 0.5 > (0.25 * m)^2
    s = mean * F(16)
    m = lum(s) / F(16)
    q = F(32) * (m * m)
    if edge == "equal":
        return s, q, 16
    if edge == "just_above":
        return s, np.nextafter(q, F(np.inf)), 16
    n = int(rng.integers(mn, mx))
    return state(n, mean, float(rng.uniform(0.0, 8.0)))


def edge_state(covered, seed=1, offset=0):
    """(sums [h, w, 3], sumsq [h, w], counts [h, w] uint32, edge name per texel [h, w] or ''): covered texel number i (row-major) sits on
    EDGES[(i + offset) % len(EDGES)]; uncovered texels hold garbage that must never be read: NaN sums and moments, a count of 2^32 - 1"""
    cov = np.asarray(covered, bool)
    h, w = cov.shape
    rng = np.random.default_rng(seed)
    sums = np.full((h, w, 3), np.nan, F); sumsq = np.full((h, w), np.nan, F); counts = np.full((h, w), 0xFFFFFFFF, np.uint32)
    names = np.full((h, w), "", object)
    for i, (j, k) in enumerate(np.argwhere(cov)):
        edge = EDGES[(i + offset) % len(EDGES)]
        s, q, n = _texel(edge, rng)
        sums[j, k] = s; sumsq[j, k] = q; counts[j, k] = n; names[j, k] = edge
    assert sums.dtype == F and sumsq.dtype == F
    return sums, sumsq, counts, names


def check_edges_are_meaningful(state, covered):
    """what each edge is there for, asserted on the RESTATEMENT under EDGE_CRIT and its variants"""
    sums, sumsq, counts, names = state
    want = active(sums, sumsq, counts, covered, **EDGE_CRIT)
    m, e2, t = terms(sums, sumsq, counts, EDGE_CRIT["rel_error"], EDGE_CRIT["abs_floor"])
    expect = {"count_0": True, "below_min": True, "at_min_flat": False, "at_min_noisy": True, "below_max": True, "at_max": False, "v_negative": False,
              "under_floor": False, "over_floor": True, "equal": False, "just_above": True}
    for edge, on in expect.items():
        at = names == edge
        assert (want[at] == on).all(), edge
    with np.errstate(all="ignore"):
        at = names == "equal"
        assert (e2[at] == (t * t)[at]).all() and (e2[at] > 0).all()
        at = names == "v_negative"
        assert ((np.asarray(sumsq, F) / counts.astype(F) - m * m)[at] < 0).all() and (e2[at] == 0).all()
        at = names == "under_floor"
        assert (m[at] < F(EDGE_CRIT["abs_floor"])).all() and (e2[at] > (F(EDGE_CRIT["rel_error"]) * m[at]) ** 2).all()
    # the variants each move some edge
    assert active(sums, sumsq, counts, covered, **dict(EDGE_CRIT, max_samples=0))[names == "at_max"].all()
    assert active(sums, sumsq, counts, covered, **dict(EDGE_CRIT, abs_floor=0.0))[names == "under_floor"].all()
    assert active(sums, sumsq, counts, covered, **dict(EDGE_CRIT, rel_error=0.0))[names == "equal"].all()
    assert not active(sums, sumsq, counts, covered, **dict(EDGE_CRIT, rel_error=0.0))[names == "v_negative"].any()
    assert not want[~np.asarray(covered, bool)].any()


# ---- the maps: (scene, model) by kind, their coverage
MAPS = [("box", 48, 32), ("box", 37, 19), ("quad", 1, 1), ("overlap", 10, 10)]
_SCENES = {}


def scene(kind):
    if kind not in _SCENES:
        _SCENES[kind] = {"box": LC.cornell_atlas_scene, "quad": lambda: (LC.quad_scene(), 0), "overlap": lambda: (LC.texel_case("overlap")[0], 0)}[kind]()
    return _SCENES[kind]


def covered(kind, w, h):
    sc, model = scene(kind)
    return LC.coverage(sc.models[model].uvs, w, h)[0] != LC.MISS
