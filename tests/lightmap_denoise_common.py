"""numpy restatement of the texel-space denoiser (include/pt_api.h, pt_lightmap_denoise): the texel area and the reach term, stated here, on
top of denoise_common's preparation, spatial variance and levels, which run unchanged with the neighbour rule widened by the reach test.  Also
the scenes, the synthetic sums and the case grid the CPU and the GPU tests share.  Nothing here calls the library under test."""
import contextlib

import numpy as np

import denoise_common as DC
import lightmap_common as LC

F = np.float32
D = np.float64
MISS = LC.MISS
_PLAIN = DC._neighbours


# ---- the definition
def texel_area(prim, positions, uvs, w, h):
    """area [h, w] float32: A3 / ((A2 * w) * h) of the owning triangle, 0 for an uncovered texel"""
    pos = np.asarray(positions, F).reshape(-1, 3, 3)
    uv = np.asarray(uvs, F).reshape(-1, 3, 2).astype(D)
    a, b = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    X = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    A3 = np.sqrt((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]) + X[:, 2] * X[:, 2])
    A2 = np.abs(LC._edge(uv[:, 0, 0], uv[:, 0, 1], uv[:, 1, 0], uv[:, 1, 1], uv[:, 2, 0], uv[:, 2, 1])).astype(F)
    assert X.dtype == F and A3.dtype == F
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        per_tri = A3 / ((A2 * F(w)) * F(h))
    cov = prim != MISS
    out = np.zeros((h, w), F)
    out[cov] = per_tri[prim[cov].astype(np.int64)]
    return out


def reach_squared(reach):
    with np.errstate(over="ignore"):
        r = F(reach or 2.0)
        return r * r


def _neighbours_within_reach(pos, area, reach2):
    """denoise_common._neighbours with the REACH test: d2 <= ((reach * reach) * area_p) * (float)(ox * ox + oy * oy)"""
    with np.errstate(invalid="ignore", over="ignore"):
        lim = reach2 * area

    def factory(valid, model):
        plain = _PLAIN(valid, model)

        def neighbour(ox, oy):
            ok = plain(ox, oy)
            if ox == 0 and oy == 0:
                return ok
            xq, _ = DC._shift(pos, ox, oy)
            d = xq[..., :3] - pos[..., :3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            with np.errstate(invalid="ignore", over="ignore"):
                return ok & (d2 <= lim * F(ox * ox + oy * oy))
        return neighbour
    return factory


@contextlib.contextmanager
def _neighbour_rule(factory):
    """denoise_common's spatial_variance and levels ask _neighbours who a tap's neighbour is: they run under this rule, otherwise untouched"""
    DC._neighbours = factory
    try:
        yield
    finally:
        DC._neighbours = _PLAIN


def frame_images(table, sums, n_samples):
    """the images of the defining property: accum = (sum, n) with w = 0 where uncovered, position = (P, 0), normal = n, model = 0"""
    prim, _, position, normal = table
    h, w = prim.shape
    cov = prim != MISS
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = np.asarray(sums, F).reshape(h, w, 3)
    acc[..., 3] = np.where(cov, F(n_samples), F(0))
    pos = np.concatenate([position, np.zeros((h, w, 1), F)], -1).astype(F)
    return acc, pos, np.asarray(normal, F), np.zeros((h, w), np.uint32)


def denoise(table, positions, uvs, sums, n_samples, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0, reach=0.0):
    """(means [h, w, 3], texel area [h, w]) of pt_lightmap_denoise"""
    prim = table[0]
    h, w = prim.shape
    it, sl, log2_sn, sx = DC.params(iterations, sigma_luminance, sigma_normal, sigma_plane)
    acc, pos, nrm, model = frame_images(table, sums, n_samples)
    area = texel_area(prim, positions, uvs, w, h)
    c, var, _, valid = DC.prepare(acc, model, None, None if sumsq is None else np.asarray(sumsq, F).reshape(h, w))
    hit = np.ones((h, w), bool)
    nv = np.concatenate([nrm, valid[..., None].astype(F)], axis=-1)
    with _neighbour_rule(_neighbours_within_reach(pos, area, reach_squared(reach))):
        if var is None:
            var = DC.spatial_variance(c, valid, hit, nv, pos, model, log2_sn, sx)
        c = DC.levels(c, var, valid, hit, nv, pos, model, it, sl, log2_sn, sx)
    return np.where(valid[..., None], c, F(0)).astype(F), area


# ---- scenes
def two_chart_scene(w=16):
    """TWO-CHART: two coplanar unit quads 100 units apart; chart A's UVs fill columns 0 .. w/2 - 2 of a map w wide, chart B's columns w/2 .. w - 1,
    and column w/2 - 1 is the one texel of padding between them"""
    assert w % 2 == 0 and w >= 8
    pos = np.concatenate([LC.QUAD_POS, LC.QUAD_POS + np.array([100, 0, 0], F)])
    nrm = np.tile(np.array([0, 0, 1], F), (4, 3, 1))
    s_a = LC.QUAD_UV[..., 0] * F((w // 2 - 1) / w)
    s_b = F(0.5) + LC.QUAD_UV[..., 0] * F(0.5)
    uv = np.concatenate([np.stack([s_a, LC.QUAD_UV[..., 1]], -1), np.stack([s_b, LC.QUAD_UV[..., 1]], -1)]).astype(F)
    return LC.quad_scene(uv, pos, nrm)


def chart_masks(prim):
    """(texels of chart A, texels of chart B) of the TWO-CHART model's table"""
    return (prim == 0) | (prim == 1), (prim == 2) | (prim == 3)


_SCENES = {}


def scene(kind):
    """(scene, model index) of 'quad', 'box' (the Cornell short box under the box atlas) or 'two' (TWO-CHART at 16 texels across)"""
    if kind not in _SCENES:
        _SCENES[kind] = {"quad": lambda: (LC.quad_scene(), 0), "box": LC.cornell_atlas_scene, "two": lambda: (two_chart_scene(16), 0)}[kind]()
    return _SCENES[kind]


def table_of(kind, w, h):
    sc, model = scene(kind)
    m = sc.models[model]
    return LC.texels(m.positions, m.normals, m.uvs, m.matrices[0], w, h)


def synthetic(w, h, n_samples, seed):
    """seeded, positive sums [h, w, 3] and second moments [h, w] of n_samples samples: means in [0.2, 2], a luminance variance in [0.01, 0.5]"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.2, 2.0, (h, w, 3)).astype(F)
    sums = (mean * F(n_samples)).astype(F)
    l = DC.lum(mean)
    sumsq = ((l * l + rng.uniform(0.01, 0.5, (h, w)).astype(F)) * F(n_samples)).astype(F)
    return sums, sumsq


# ---- the case grid: 16 x 16 is one workgroup, 37 x 19 has ragged edges, 48 x 32 several workgroups, 1 x 1 the smallest map; at 8 iterations
# (step 128) every non-centre tap leaves every one of these maps
MAPS = [("box", 16, 16), ("box", 37, 19), ("box", 48, 32), ("quad", 1, 1), ("two", 16, 16)]
ITERATIONS = [1, 3, 5, 8]
N_SAMPLES = 16
_EXPECT = {}


def case_ids():
    return [(kind, w, h, it, moments) for kind, w, h in MAPS for it in ITERATIONS for moments in (True, False)]


def expected(kind, w, h, it, moments, reach=0.0):
    """(table, sums, sumsq or None, (means, area) by the restatement), computed once per case"""
    key = (kind, w, h, it, moments, reach)
    if key not in _EXPECT:
        sc, model = scene(kind)
        m = sc.models[model]
        table = table_of(kind, w, h)
        sums, sumsq = synthetic(w, h, N_SAMPLES, seed=w * 1000 + h)
        sq = sumsq if moments else None
        _EXPECT[key] = (table, sums, sq, denoise(table, m.positions, m.uvs, sums, N_SAMPLES, sq, iterations=it, reach=reach))
    return _EXPECT[key]
