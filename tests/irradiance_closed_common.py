"""Shared by tests/test_irradiance_closed_host.py and tests/test_gpu_irradiance_closed.py: a sky whose radiance is a polynomial of degree <= 2
in the direction, the closed form of the irradiance it gives a surface that sees all of it, the nine real spherical harmonics from their
normalisation formulas, the exact projection of the sky onto them, the sky as an equirect map, the single-sample deviations of the two
estimators, the pass rule and the tilted quad.  Everything is binary64 and NOTHING here calls the library or the oracle (the scene is
written in path_tracer_amd.scene_desc's plain data, as every test's is): the module restates no line of either, it only knows the
conventions include/pt_api.h documents (the order y0..y8, the equirect map of pt_set_environment, the units of pt_set_probe_grid and
pt_set_lightmap).

THE CLOSED FORM.  Per channel L(w) = a + b.w + w^T C w with C symmetric.  For a unit normal n that sees the whole sky,
    I(n) = (1 / pi) * integral of L(w) max(0, n.w) dw = a + tr(C) / 3 + (2/3) b.n + (1/4) (n^T C n - tr(C) / 3)
one term per SH band: the cosine lobe over pi has the zonal factors 1, 2/3 and 1/4.  SH9 holds degree <= 2 exactly, so a probe that holds
the sky's projection owes I(n) to rounding alone; a convex Lambertian surface of colour R under the sky reflects exactly R * I(n).

THE PASS RULE.  A statistical comparison passes when |mean - closed form| <= 5 sigma / sqrt(independent samples) + delta_env + geometric
bias, sigma being the single-sample deviation of a KNOWN distribution (sigma_cos, sigma_sph below, by quadrature) and the seeds fixed.
Where the mean weighs its samples unequally (a view that blends texels or probes), the count is Kish's effective one, 1 / sum w^2 for
weights that sum to 1.  Figures: profiles/r26_closed_form.md."""
import numpy as np

D = np.float64
F = np.float32
U = 2.0 ** -24                    # half an ulp of 1 in binary32: one rounding, relative
ALBEDO = 0.8                      # lightmap_common.quad_scene's Lambertian colour
COSINE = (1.0, 2.0 / 3.0, 0.25)   # the cosine lobe over pi, per band
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)
SIGMAS = 5.0                      # the pass rule's margin, in standard errors


# ------------------------------------------------------------------------------------------------------------------------------- the sky
class Sky:
    """three channels of L_c(w) = a_c + b_c.w + w^T C_c w; a [3], b [3, 3] (channel, axis), C [3, 3, 3] (channel, symmetric matrix)"""

    def __init__(self, a, b, C):
        self.a = np.asarray(a, D); self.b = np.asarray(b, D); self.C = np.asarray(C, D)
        assert self.a.shape == (3,) and self.b.shape == (3, 3) and self.C.shape == (3, 3, 3)
        assert np.array_equal(self.C, np.transpose(self.C, (0, 2, 1)))

    def radiance(self, w):
        """L at directions w [..., 3] (used as given) -> [..., 3]"""
        w = np.asarray(w, D)
        return self.a + w @ self.b.T + np.einsum("...i,cij,...j->...c", w, self.C, w)

    def irradiance(self, n):
        """THE CLOSED FORM: I over pi at unit normals n [..., 3] -> [..., 3]"""
        n = np.asarray(n, D)
        tr = np.trace(self.C, axis1=1, axis2=2)
        return self.a + tr / 3.0 + (2.0 / 3.0) * (n @ self.b.T) + 0.25 * (np.einsum("...i,cij,...j->...c", n, self.C, n) - tr / 3.0)

    def bands(self, n):
        """the three terms of the closed form at n [3] -> [band, channel]"""
        n = np.asarray(n, D)
        tr = np.trace(self.C, axis1=1, axis2=2)
        return np.stack([self.a + tr / 3.0, (2.0 / 3.0) * (self.b @ n), 0.25 * (np.einsum("i,cij,j->c", n, self.C, n) - tr / 3.0)])

    def magnitude(self):
        """M_c = |a| + sum |b| + sum |C|: what every rounding of an evaluation is relative to"""
        return np.abs(self.a) + np.abs(self.b).sum(1) + np.abs(self.C).sum((1, 2))

    def least_and_largest(self):
        """bounds (below, above) of L over the unit sphere per channel: a -+ |b| + the least / largest eigenvalue of C; they are attained
        where a channel has b or C alone, as every channel of SKY has"""
        lo = np.array([self.a[c] - np.linalg.norm(self.b[c]) + np.linalg.eigvalsh(self.C[c])[0] for c in range(3)])
        hi = np.array([self.a[c] + np.linalg.norm(self.b[c]) + np.linalg.eigvalsh(self.C[c])[-1] for c in range(3)])
        return lo, hi


def _outer(v, lam):
    v = np.asarray(v, D)
    return lam * np.outer(v, v) / (v @ v)


# channel 0: constant; channel 1: constant + linear; channel 2: constant + quadratic with a trace
SKY = Sky(a=[0.75, 1.0, 0.25],
          b=[[0.0, 0.0, 0.0], [0.35, -0.55, 0.6], [0.0, 0.0, 0.0]],
          C=[np.zeros((3, 3)), np.zeros((3, 3)),
             _outer([0.3, -0.6, 0.74], 1.5) + np.array([[0.10, 0.05, -0.04], [0.05, -0.06, 0.03], [-0.04, 0.03, 0.02]])])
# a second sky, for a probe field that varies in space (positive too, every band in every channel)
SKY1 = Sky(a=[0.5, 0.625, 0.75],
           b=[[-0.2, 0.15, 0.1], [0.1, 0.2, -0.3], [-0.25, -0.1, 0.05]],
           C=[_outer([1.0, 0.5, -0.25], 0.4), np.array([[0.2, -0.1, 0.05], [-0.1, 0.1, 0.15], [0.05, 0.15, -0.05]]), _outer([-0.5, 1.0, 1.0], 0.3)])


# ----------------------------------------------------------------------------------------------------------------------------- the quad
QUAT = (2.0, 3.0, -5.0, 7.0)                      # a general rotation: the normal gets three non-zero components
TRANSLATION = (0.375, -0.25, 0.5)


def quad_matrix():
    """the rigid 3 x 4 (float32, the reference's own construction from a unit quaternion) that tilts lightmap_common's unit quad"""
    from path_tracer_amd.scene_desc import affine_from_rotation_translation, is_rigid, quat_unit
    m = affine_from_rotation_translation(quat_unit(*QUAT), TRANSLATION)
    assert is_rigid(m)
    return m


def _rotation64():
    x, y, z, w = np.asarray(QUAT, D) / np.sqrt(np.sum(np.square(QUAT)))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


ROTATION = _rotation64()                          # binary64, from the quaternion alone
NORMAL = ROTATION[:, 2].copy()                    # the tilted quad's front normal (the quad's own is +z)
NORMALS = np.stack([NORMAL, -NORMAL])             # THE TEST NORMALS: front and back
assert abs(np.linalg.norm(NORMAL) - 1.0) < 1e-15 and (np.abs(NORMAL) > 0.2).all()


def to_world(local):
    """quad-local points [..., 3] -> world, binary64"""
    return np.asarray(local, D) @ ROTATION.T + np.asarray(TRANSLATION, D)


def to_local(world):
    return (np.asarray(world, D) - np.asarray(TRANSLATION, D)) @ ROTATION


def placed_scene(instanced):
    """lightmap_common.quad_scene's quad, tilted.  instanced False: the VERTICES are turned (binary32 products of the matrix, normals
    alike) and the instance is the identity, which takes the one-ray walk; True: the axis-aligned quad under the matrix as its instance,
    which takes the general walk and the transform of the normal."""
    import lightmap_common as LC
    from path_tracer_amd.scene_desc import Lambertian, Model, SceneDesc
    m = quad_matrix()
    if instanced:
        model = Model.new(LC.QUAD_POS, LC.QUAD_NRM, Lambertian.new((ALBEDO,) * 3), m[None], "quad", uvs=LC.QUAD_UV)
    else:
        pos = (LC.QUAD_POS.astype(D) @ m[:, :3].astype(D).T + m[:, 3].astype(D)).astype(F)
        nrm = (LC.QUAD_NRM.astype(D) @ m[:, :3].astype(D).T).astype(F)
        model = Model.new(pos, nrm, Lambertian.new((ALBEDO,) * 3), None, "quad", uvs=LC.QUAD_UV)
    return SceneDesc.new([model], None, "tilted quad")


def inside_instance_box(local, margin=0.02):
    """which quad-local points [k, 3] lie, in the world, inside the box that the reference gives the INSTANCED quad in its TLAS: the box of
    the object box's two extreme corners (0, 0, 0) and (1, 1, 0) transformed, not of all its corners (boundingbox.rs:51-57, the corner-only
    AABB::transform the library and the oracle both keep).  Under a general rotation that box does not hold the whole quad, and a ray aimed
    at a point of the quad outside it may pass the box by and see the sky instead.  A ray through a point INSIDE the box meets the box, so
    the tests aim at such points only, `margin` inside every face; here that is the strip 2 s - 1 <= t <= 2 s, half the quad."""
    ends = to_world([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
    lo, hi = ends.min(0) + margin, ends.max(0) - margin
    w = to_world(local)
    return ((w >= lo) & (w <= hi)).all(-1)


CAMERA_DISTANCE, CAMERA_FOV = 0.5, 28.0


def close_camera(side):
    """a camera on the quad's axis, CAMERA_DISTANCE off its centre on the side of normal side * NORMAL.  The frame's half-diagonal on the
    quad is distance * tan(fov / 2) * sqrt(2) = 0.18, and the whole disc of that radius about the centre lies in the quad's interior and
    inside the instance's box (asserted below), so whatever the roll every ray meets the quad."""
    from path_tracer_amd.scene_desc import Camera
    centre = to_world([0.5, 0.5, 0.0])
    return Camera.new(centre + side * CAMERA_DISTANCE * NORMAL, centre, CAMERA_FOV, 1.0)


def _camera_footprint_is_inside():
    radius = CAMERA_DISTANCE * np.tan(np.radians(CAMERA_FOV) / 2.0) * np.sqrt(2.0) * 1.05      # 5 % for the jitter of the outermost pixels
    a = np.linspace(0.0, 2.0 * np.pi, 64)
    ring = np.stack([0.5 + radius * np.cos(a), 0.5 + radius * np.sin(a), np.zeros(64)], 1)
    return bool(inside_instance_box(ring).all() and (ring[:, :2] > 0.1).all() and (ring[:, :2] < 0.9).all())


assert _camera_footprint_is_inside()


def interior_rays(n, seed, side):
    """n rays (o, d float32) that meet seeded interior points of the quad (local s, t in [0.1, 0.9], inside the instance's box) from the
    side of side * NORMAL, each from its own origin one to two sides away and up to 45 degrees off the axis"""
    rng = np.random.default_rng(seed)
    st = np.zeros((0, 2))
    while len(st) < n:
        more = rng.uniform(0.1, 0.9, (2 * n, 2))
        st = np.concatenate([st, more[inside_instance_box(np.concatenate([more, np.zeros((2 * n, 1))], 1))]])
    st = st[:n]
    target = to_world(np.concatenate([st, np.zeros((n, 1))], 1))
    tilt = rng.uniform(-0.7, 0.7, (n, 2))
    local_dir = np.concatenate([tilt, np.full((n, 1), float(side))], 1)
    away = local_dir @ ROTATION.T
    o = target + rng.uniform(1.0, 2.0, (n, 1)) * away
    d = target - o
    return o.astype(F), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


# ----------------------------------------------------------------------------------------------------------------------------- the basis
K0, K1, K2, K3, K4 = np.sqrt(1.0 / (4.0 * np.pi)), np.sqrt(3.0 / (4.0 * np.pi)), np.sqrt(15.0 / (4.0 * np.pi)), np.sqrt(5.0 / (16.0 * np.pi)), \
    np.sqrt(15.0 / (16.0 * np.pi))


def sh9(d):
    """the nine real spherical harmonics of bands 0-2 at d [..., 3] (used as given) in the order include/pt_api.h documents for
    pt_bake_probes: 1 | y, z, x | xy, yz, 3 z^2 - 1, xz, x^2 - y^2 -> [..., 9]"""
    d = np.asarray(d, D)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, K0), K1 * y, K1 * z, K1 * x, K2 * x * y, K2 * y * z, K3 * (3.0 * z * z - 1.0), K2 * x * z, K4 * (x * x - y * y)], -1)


def sphere_rule(nz, nphi):
    """directions [nz * nphi, 3] and weights of Gauss-Legendre in z times the midpoint rule in phi: exact for polynomials of degree
    <= min(2 nz - 1, nphi - 1) in the direction"""
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], -1).reshape(-1, 3)
    return d, np.repeat(wz, nphi) * (2.0 * np.pi / nphi)


def project(sky):
    """the EXACT radiance coefficients L_m,c = integral of L_c y_m over the sphere [9, 3]: 8 x 16 nodes, exact for degree <= 4"""
    d, w = sphere_rule(8, 16)
    return np.einsum("k,km,kc->mc", w, sh9(d), sky.radiance(d))


def evaluate(coeff, n):
    """the irradiance over pi that radiance coefficients [9, 3] give normal n [..., 3]: sum over m of A_band(m) y_m(n) L_m"""
    return (sh9(n) * np.asarray(COSINE)[list(BAND)]) @ np.asarray(coeff, D)


def kernel(n, d):
    """4 pi * sum over m of A_m y_m(n) y_m(d) for one normal n [3] and directions d [k, 3]: the weight a uniform sample of the sphere has
    in the probe estimate of I(n).  Its largest value is 1 + 2 + 5/4 at d = n."""
    return 4.0 * np.pi * (sh9(d) @ (sh9(n) * np.asarray(COSINE)[list(BAND)]))


KERNEL_MAX = 4.25


# --------------------------------------------------------------------------------------------------------------------- the sky as a map
ENV_W, ENV_H = 512, 256


def env_directions(w, h):
    """the direction texel (i, j) of a w x h equirect map stands for under pt_set_environment's convention: a lookup of direction d reads
    u = atan2(d.x, d.z) / (2 pi) + 0.5 and v = 0.5 - asin(d.y) / pi and blends the texels around (w u, h v), so texel (i, j) sits AT u = i / w,
    v = j / h with no half-texel offset -> [h, w, 3]"""
    u = np.arange(w, dtype=D) / w
    v = np.arange(h, dtype=D) / h
    return _uv_directions(*np.meshgrid(u, v))


def _uv_directions(u, v):
    theta, lat = (u - 0.5) * (2.0 * np.pi), (0.5 - v) * np.pi
    return np.stack([np.cos(lat) * np.sin(theta), np.sin(lat), np.cos(lat) * np.cos(theta)], -1)


def env_map(sky=None, w=ENV_W, h=ENV_H):
    """the sky as the float32 map [h, w, 3] the tests set"""
    return (SKY if sky is None else sky).radiance(env_directions(w, h)).astype(F)


def _map_quadrature(texels, normals, sub, exact=None):
    """(1 / pi) * integral of L max(0, n.w) dw over the (u, v) square, sub x sub midpoints a texel, for every normal -> [normals, 3].
    L is the bilinear blend of `texels` as the reference takes it (texel x0 = floor(w u) and its neighbour x0 + 1 modulo w; rows alike
    modulo h, so the last row blends towards row 0), or with `exact` that sky itself: the rule's own error."""
    h, w = texels.shape[:2]
    t = texels.astype(D)
    out = np.zeros((len(normals), 3))
    x = (np.arange(w * sub) + 0.5) / sub
    x0 = np.floor(x).astype(np.int64); xf = x - x0; x1 = (x0 + 1) % w
    for j in range(h):                                            # a row of texels at a time keeps the arrays small
        y = j + (np.arange(sub) + 0.5) / sub
        yf = (y - j)[:, None, None]
        uu, vv = np.meshgrid(x / w, y / h)
        d = _uv_directions(uu, vv)                               # [sub, w * sub, 3]
        if exact is None:
            top = t[j][x0] * (1.0 - xf)[:, None] + t[j][x1] * xf[:, None]
            bot = t[(j + 1) % h][x0] * (1.0 - xf)[:, None] + t[(j + 1) % h][x1] * xf[:, None]
            L = top[None] * (1.0 - yf) + bot[None] * yf
        else:
            L = exact.radiance(d)
        area = np.cos((0.5 - vv) * np.pi) * (2.0 * np.pi * np.pi / (w * h * sub * sub))
        for k, n in enumerate(normals):
            out[k] += np.einsum("ab,abc->c", np.maximum(d @ n, 0.0) * area, L)
    return out / np.pi


_ENV = {}


def delta_env():
    """delta_env [normal, channel]: |I_bilinear(n) - I(n)| at the test normals plus the quadrature rule's own error (the same rule on the
    exact sky against the closed form); computed once"""
    if "delta" not in _ENV:
        want = SKY.irradiance(NORMALS)
        rule = np.abs(_map_quadrature(env_map(), NORMALS, 2, exact=SKY) - want)
        _ENV["rule"] = rule
        _ENV["delta"] = np.abs(_map_quadrature(env_map(), NORMALS, 2) - want) + rule
        assert (_ENV["delta"] <= 1e-3 * want).all(), _ENV["delta"] / want          # the map's size is chosen for this: at most 0.1 % of I
    return _ENV["delta"]


# -------------------------------------------------------------------------------------------------------- the single-sample deviations
def _frame(n):
    a = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    t = np.cross(n, a); t /= np.linalg.norm(t)
    return t, np.cross(n, t)


def sigma_cos(n, sky=None):
    """ALBEDO * the deviation of L(w) for w cosine-distributed about n [3] -> [3].  With t = cos(theta) the density is 2 t dt dphi / (2 pi):
    Gauss-Legendre on [0, 1] (32 nodes) times the midpoint rule in phi (32), far beyond the degree of L^2."""
    sky = SKY if sky is None else sky
    n = np.asarray(n, D)
    x, wx = np.polynomial.legendre.leggauss(32)
    t, wt = 0.5 * (x + 1.0), 0.5 * wx
    phi = (np.arange(32) + 0.5) * (2.0 * np.pi / 32)
    tt, pp = np.meshgrid(t, phi, indexing="ij")
    s = np.sqrt(1.0 - tt * tt)
    e1, e2 = _frame(n)
    w = (s * np.cos(pp))[..., None] * e1 + (s * np.sin(pp))[..., None] * e2 + tt[..., None] * n
    weight = (2.0 * tt * wt[:, None] / 32.0)[..., None]
    L = sky.radiance(w)
    mean, second = (weight * L).sum((0, 1)), (weight * L * L).sum((0, 1))
    assert np.abs(mean - sky.irradiance(n)).max() < 1e-12             # the cosine mean of L IS the closed form
    return ALBEDO * np.sqrt(np.maximum(second - mean * mean, 0.0))              # a constant channel: exactly 0


def sigma_sph(n, sky=None):
    """the deviation of 4 pi L(d) sum_m A_m y_m(n) y_m(d) for d uniform on the sphere -> [3] (its square has degree 8: 16 x 32 nodes)"""
    sky = SKY if sky is None else sky
    n = np.asarray(n, D)
    d, w = sphere_rule(16, 32)
    f = sky.radiance(d) * kernel(n, d)[:, None]
    p = (w / (4.0 * np.pi))[:, None]
    mean, second = (p * f).sum(0), (p * f * f).sum(0)
    assert np.abs(mean - sky.irradiance(n)).max() < 1e-12             # the estimator is unbiased for a sky of degree <= 2
    return np.sqrt(np.maximum(second - mean * mean, 0.0))


# ------------------------------------------------------------------------------------------------------------------------ the pass rule
def bound(sigma, samples, delta=0.0, bias=0.0, sigmas=SIGMAS):
    return sigmas * np.asarray(sigma, D) / np.sqrt(float(samples)) + delta + bias


def fold_rounding(n, value):
    """what a binary32 fold of n addends of one sign can lose of their mean: fewer than n roundings, each at most half an ulp of a partial
    sum that is at most the total.  It is there for the constant channel, whose sigma is 0; beside any other channel's noise it is nothing."""
    return n * U * np.abs(np.asarray(value, D))


def check(what, got, want, tolerance):
    """assert |got - want| <= tolerance per component; the message (and the line printed before the assertion) gives the worst deviation in
    units of its bound.  Returns that figure."""
    got, want, tolerance = np.broadcast_arrays(np.asarray(got, D), np.asarray(want, D), np.asarray(tolerance, D))
    units = np.abs(got - want) / tolerance
    worst = float(units.max())
    print(f"closed-form check | {what} | worst {worst:.3f} of its bound | per channel {np.round(units.reshape(-1, units.shape[-1]).max(0), 3).tolist()}")
    assert worst <= 1.0, f"{what}: {worst:.3f} times the bound (got {got.reshape(-1)[units.argmax()]:.7g}, want {want.reshape(-1)[units.argmax()]:.7g}, " \
                         f"bound {tolerance.reshape(-1)[units.argmax()]:.3g})"
    return worst


# ---------------------------------------------------------------------------------------------------- the probe grid around the quad
PROBE_CELL = 64.0                                  # 2 x 2 x 2 nodes, the quad near the middle of the one cell
PROBE_ORIGIN = (-32.0, -32.0, -32.0)
PROBE_COUNT = (2, 2, 2)


def probe_nodes():
    idx = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")[::-1], -1).reshape(-1, 3).astype(D)
    return np.asarray(PROBE_ORIGIN, D) + idx * PROBE_CELL      # node index (iz * 2 + iy) * 2 + ix, x fastest


def geometric_bias():
    """what the quad itself takes from a probe's view of the sky, per channel: its solid-angle fraction at the nearest node (at most
    area / (4 pi r^2), r to the nearest corner) times the largest radiance"""
    corners = to_world([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    r = min(np.linalg.norm(corners - p, axis=1).min() for p in probe_nodes())
    assert r >= 30.0                                           # every node at least 30 quad sides away
    return (1.0 / (4.0 * np.pi * r * r)) * SKY.least_and_largest()[1], r


def trilinear_weights(p):
    """the eight corner weights of the 2 x 2 x 2 grid at world points p [k, 3] -> [k, 8], corner bit 0: x1, bit 1: y1, bit 2: z1"""
    f = (np.asarray(p, D) - np.asarray(PROBE_ORIGIN, D)) / PROBE_CELL
    assert ((f > 0) & (f < 1)).all()
    return np.stack([np.where(c & 1, f[:, 0], 1 - f[:, 0]) * np.where(c & 2, f[:, 1], 1 - f[:, 1]) * np.where(c & 4, f[:, 2], 1 - f[:, 2])
                     for c in range(8)], 1)


# ------------------------------------------------------------------------------------------------------ the conditions, asserted here
def _conditions():
    lo, hi = SKY.least_and_largest()
    assert (lo > 0).all(), lo                                                      # positive on the whole sphere
    assert (SKY1.least_and_largest()[0] > 0).all()
    assert not SKY.b[0].any() and not SKY.C[0].any() and not SKY.C[1].any() and not SKY.b[2].any() and SKY.b[1].all()
    assert abs(np.trace(SKY.C[2])) > 0.5 and (np.abs(SKY.C[2]) > 0.01).all()       # a trace, and every basis function of band 2 takes part
    coeff = project(SKY)
    assert (np.abs(coeff[1:4, 1]) > 0.1).all() and (np.abs(coeff[4:9, 2]) > 0.02).all()
    for n in NORMALS:
        I, band = SKY.irradiance(n), SKY.bands(n)
        assert (I > 0.25).all(), I                                                 # the lookup clamps at 0
        assert abs(band[1, 1]) >= 0.25 * band[0, 1] and abs(band[2, 2]) >= 0.25 * band[0, 2], band
        assert np.abs(evaluate(coeff, n) - I).max() < 1e-14                        # SH9 holds the sky exactly
    # a dense check of the closed form itself against quadrature, at normals that are not the test's
    rng = np.random.default_rng(7)
    for n in rng.normal(size=(4, 3)):
        n /= np.linalg.norm(n)
        sigma_cos(n); sigma_sph(n); sigma_cos(n, SKY1)                             # each asserts mean == closed form
    bias, _ = geometric_bias()
    assert (bias <= 5e-4 * SKY.irradiance(NORMALS)).all()                          # below 0.05 %


_conditions()


# ------------------------------------------------------------------------------ the lookup's inputs (CPU and GPU tests share them)
FIELD_ORIGIN, FIELD_CELL, FIELD_COUNT = (-1.0, 0.5, 2.0), (1.0, 2.0, 0.5), (3, 2, 4)       # dyadic: node positions are exact
FIELD_GRADIENT = np.array([0.25, 0.125, 0.25])
FIELD_BIASES = (0.0, 0.375)
LOOKUP_ROUNDINGS = 64             # fewer than 64 roundings between the inputs and the result, each relative to a magnitude <= M


def field_nodes():
    nx, ny, nz = FIELD_COUNT
    idx = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")[::-1], -1).astype(D)
    return np.asarray(FIELD_ORIGIN, D) + idx * np.asarray(FIELD_CELL, D)                  # [nz, ny, nx, 3]


def field_coefficients(affine):
    """float32 coefficients [nz, ny, nx, 9, 3]: sh(p) = sh0 + (g.p) sh1 at the nodes, which the trilinear blend reproduces exactly between
    them; affine False: sh0 everywhere"""
    s = (field_nodes() @ FIELD_GRADIENT)[..., None, None] if affine else np.zeros(FIELD_COUNT[::-1] + (1, 1))
    return (project(SKY) + s * project(SKY1)).astype(F)


def field_queries(k, seed, bias):
    """k seeded points (float32) whose biased point P + bias * n stays inside the grid's box, the 24 nodes first where bias is 0, and a
    unit normal (float32) for each"""
    rng = np.random.default_rng(seed)
    lo = np.asarray(FIELD_ORIGIN, D) + bias
    hi = np.asarray(FIELD_ORIGIN, D) + np.asarray(FIELD_CELL, D) * (np.asarray(FIELD_COUNT, D) - 1.0) - bias
    assert (hi > lo).all()
    P = rng.uniform(lo, hi, (k, 3))
    if bias == 0.0:
        P[:24] = field_nodes().reshape(-1, 3)
    n = rng.normal(size=(k, 3))
    return P.astype(F), (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def field_expected(P, n, bias, affine):
    """(the closed form I0(n) + (g.p') I1(n) at p' = P + bias * n [k, 3], the bound LOOKUP_ROUNDINGS * 2^-24 * M [3]).  M is the sky's
    |a| + sum |b| + sum |C|, and for the affine field M0 + (sum_a |g_a| max |p'_a|) M1, the box's largest coordinates standing in for p'."""
    P, n = np.asarray(P, F).astype(D), np.asarray(n, F).astype(D)
    want, M = SKY.irradiance(n), SKY.magnitude()
    if affine:
        want = want + ((P + bias * n) @ FIELD_GRADIENT)[:, None] * SKY1.irradiance(n)
        far = np.maximum(np.abs(field_nodes().reshape(-1, 3)).max(0), 0.0)
        M = M + float(np.abs(FIELD_GRADIENT) @ far) * SKY1.magnitude()
    assert (want > 0.05).all()                                                            # the lookup clamps at 0
    return want, LOOKUP_ROUNDINGS * U * M


DEPTH_RES = 4


def depth_tables(seed=5):
    """depth moments [24 nodes, 16 texels, 2] float32 for the 3 x 2 x 4 grid: seeded random ones (mean distances around the cell size, so
    that some corners are nearer than their mean and some farther), fully occluding ones (every mean 0.03 with next to no variance: every
    corner farther away falls to the floor) and a mixture by node"""
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.1, 3.0, (24, 16)).astype(F)
    random = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.5, (24, 16)).astype(F)], -1).astype(F)
    near = np.full((24, 16), 0.03, F)
    occluding = np.stack([near, near * near + F(1e-6)], -1).astype(F)
    mixed = np.where((np.arange(24) % 2 == 0)[:, None, None], random, occluding).astype(F)
    return {"random": random, "occluding": occluding, "mixed": mixed}


def open_table():
    """every mean 1e6: nothing is farther than its mean, so every visibility is 1"""
    return np.stack([np.full((24, 16), 1e6, F), np.full((24, 16), 1e12, F)], -1).astype(F)
