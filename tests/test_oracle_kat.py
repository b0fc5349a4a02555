"""CPU: the oracle against every known answer that can be derived from the reference's source text
and against properties that need no reference binary.  The reference itself holds no tests, vectors or fixtures
(parity unpinned), so these are what anchors the restatement."""
import numpy as np
import pytest

from conftest import assert_bit_equal


def test_sobol_direction_numbers(oracle_mod):
    L = oracle_mod.lib()
    assert [L.pto_sobol_dim1(i) for i in range(8)] == [0x00000000, 0x80000000, 0xC0000000, 0x40000000, 0xA0000000, 0x20000000, 0x60000000, 0xE0000000]


def test_hashes(oracle_mod):
    L = oracle_mod.lib()
    assert [L.pto_low_bias_hash(x) for x in (0, 1, 2, 3, 0xDEADBEEF)] == [0x00000000, 0x06D3FA73, 0x0DA7F4E7, 0x0D6FDEFA, 0x8A2B8AF2]
    assert L.pto_lk_hash(1, 0) == 0x3EAEF8DD
    assert L.pto_lk_hash(0x12345678, 0x9ABCDEF0) == 0xFB1D0B68


@pytest.mark.parametrize("index,seed,shuffled,slot,x,y", [
    (0, 0, 0xDEBA4DF9, 505, 0xA30AE09A, 0x231C175E),
    (1, 0, 0xDEBA4DF8, 504, 0x19984A78, 0x9ECD1C95),
    (0, 1, 0x56F24A19, 25, 0x6B17BD49, 0x0EE62FF7),
    (5, 0xDEADBEEF, 0x2C575EDC, 220, 0x646F0B04, 0x9E5AF2A8),
    (255, 12345, 0x6A66A729, 297, 0xE2891023, 0x053CCA92),
])
def test_ss_sobol_integer_pipeline(oracle_mod, index, seed, shuffled, slot, x, y):
    raw = oracle_mod.ss_sobol_raw(512, index, seed)
    assert raw == (shuffled, x, y) and shuffled % 512 == slot
    f = oracle_mod.ss_sobol(512, index, seed)
    assert f[0] == np.float32(np.float32(x) / np.float32(4294967296.0)) and 0.0 <= f[1] <= 1.0


def test_wyrand_stream(oracle_mod):
    L = oracle_mod.lib()
    assert [L.pto_wyrand(0, k) for k in range(3)] == [0x111CB3A78F59A58E, 0xCEABD938FF4E856D, 0x61FB51318F47D2A4]
    assert [L.pto_wyrand(42, k) for k in range(3)] == [0xAE4A7CBFDDA9B434, 0xE9CC09D33D38D9D2, 0xCB5756512B93433A]


def test_deterministic_libm_accuracy(oracle_mod):
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 2 * np.pi, 100000).astype(np.float32)
    s, c = oracle_mod.math_batch(0, x)
    assert np.abs(s - np.sin(x.astype(np.float64))).max() < 2e-7
    assert np.abs(c - np.cos(x.astype(np.float64))).max() < 2e-7
    x = rng.uniform(-30, 30, 100000).astype(np.float32)
    e, _ = oracle_mod.math_batch(1, x)
    assert np.abs(e / np.exp(x.astype(np.float64)) - 1).max() < 3e-7
    x = np.exp(rng.uniform(-30, 30, 100000)).astype(np.float32)
    l, _ = oracle_mod.math_batch(2, x)
    assert np.abs(l - np.log(x.astype(np.float64))).max() < 4e-6
    a = rng.normal(size=10000).astype(np.float32); b = rng.normal(size=10000).astype(np.float32)
    h, _ = oracle_mod.math_batch(3, a, b)
    assert_bit_equal(h, np.sqrt(a.astype(np.float64) ** 2 + b.astype(np.float64) ** 2).astype(np.float32), "hypot")


def test_triangle_precompute_identities(oracle_mod, cornell64):
    """primitive.rs:31-54: n1.A + d1 = 0, n1.C + d1 = 1 (u = 1 at C), n2.B + d2 = 1 (v = 1 at B ... per Havel-Herout layout)."""
    o = oracle_mod.Oracle(cornell64)
    for blas in range(o.blas_count()):
        t = o.triangle(blas, 0).astype(np.float64)
        n0, n1, n2 = t[0:4], t[4:8], t[8:12]
        A, B, C = t[12:15], t[15:18], t[18:21]
        assert abs(n0[:3] @ A - n0[3]) < 1e-2 * max(1.0, abs(n0[3]))
        assert abs(n1[:3] @ A + n1[3]) < 1e-4
        assert abs(n2[:3] @ A + n2[3]) < 1e-4
        assert abs(n1[:3] @ B + n1[3] - 1) < 1e-4      # u = 1 at B
        assert abs(n2[:3] @ C + n2[3] - 1) < 1e-4      # v = 1 at C


def _camera_rays(o, w, h, n, seed):
    rng = np.random.default_rng(seed)
    px = rng.integers(0, w * h, n)
    O = np.zeros((n, 3), np.float32); D = np.zeros((n, 3), np.float32)
    for i, p in enumerate(px):
        O[i], D[i] = o.primary_ray(w, h, int(p), int(i % 7))
    return O, D


def _brute_force_closest(scene, O, D):
    """Moeller-Trumbore in float64 over every triangle (identity instances)."""
    best = np.full(len(O), np.inf)
    for m in scene.models:
        P = m.positions.astype(np.float64)
        for tri in P:
            e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
            pv = np.cross(D.astype(np.float64), e2)
            det = pv @ e1
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                tv = O.astype(np.float64) - tri[0]
                u = (tv * pv).sum(1) * inv
                qv = np.cross(tv, e1)
                v = (D.astype(np.float64) * qv).sum(1) * inv
                t = qv @ e2 * inv
            ok = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 5e-4)
            best = np.where(ok & (t < best), t, best)
    return best


def test_bvh_closest_hit_equals_brute_force(oracle_mod, cornell64):
    o = oracle_mod.Oracle(cornell64)
    O, D = _camera_rays(o, 64, 64, 600, 1)
    hit = o.trace_closest(O, D)
    ref = _brute_force_closest(cornell64, O, D)
    miss = hit["inst"] == 0xFFFFFFFF
    assert np.array_equal(miss, ~np.isfinite(ref))
    assert np.allclose(hit["t"][~miss], ref[~miss], rtol=2e-4)
    # second bounce: rays leaving the hit points in a fixed direction
    P = O[~miss] + D[~miss] * hit["t"][~miss, None]
    D2 = np.tile(np.array([[0.3, 0.8, 0.52]], np.float32), (len(P), 1))
    D2 /= np.linalg.norm(D2, axis=1, keepdims=True)
    hit2 = o.trace_closest(P, D2.astype(np.float32))
    ref2 = _brute_force_closest(cornell64, P, D2)
    m2 = hit2["inst"] == 0xFFFFFFFF
    # grazing / epsilon cases may differ between the two formulations; demand agreement on the clear ones
    clear = np.isfinite(ref2) & (ref2 > 1e-2)
    assert np.allclose(hit2["t"][clear & ~m2], ref2[clear & ~m2], rtol=1e-3)


def test_any_hit_consistent_with_closest_hit(oracle_mod, cornell64):
    o = oracle_mod.Oracle(cornell64)
    O, D = _camera_rays(o, 64, 64, 500, 2)
    hit = o.trace_closest(O, D)
    t = np.where(hit["inst"] == 0xFFFFFFFF, np.float32(1e30), hit["t"])
    assert np.array_equal(o.trace_any(O, D, t * np.float32(1.01)).astype(bool), hit["inst"] != 0xFFFFFFFF)
    assert not o.trace_any(O, D, t * np.float32(0.99)).any()
    assert not o.trace_any(O, D, np.full(len(O), np.nan, np.float32)).any()   # NaN t_max: every box test fails


def test_lambertian_throughput_is_albedo(oracle_mod, cornell64):
    """material.rs:109-115 + integrator.rs:249: weakening * bsdf / pdf == albedo up to rounding."""
    o = oracle_mod.Oracle(cornell64)
    mats = cornell64.materials()
    gray = next(i for i, m in enumerate(mats) if m.kind == 0)
    n = np.array([0, 1, 0], np.float32)
    for s in range(50):
        r = o.material_eval(gray, np.array([0.6, -0.8, 0.0], np.float32), n, 1, 17, s)
        wo, bsdf, pdf, weak, draws = r[0:3], r[3:6], r[6], r[7], r[8]
        assert draws == 2 and wo[1] >= 0 and abs(np.linalg.norm(wo) - 1) < 1e-5
        assert np.allclose(weak * bsdf / pdf, mats[gray].colour, rtol=1e-5)


def test_white_furnace(oracle_mod):
    """Closed albedo-1... here: a diffuse box lit only by the constant ambient term cannot exceed the ambient radiance
    (integrator.rs:263-266: every escaping path carries at most path_weight <= 1 times 0.006)."""
    from path_tracer_amd import scenes
    sc = scenes.cornell_box(32, 32)
    o = oracle_mod.Oracle(sc)
    acc, _, _, _ = o.render(32, 32, 8, max_bounces=6, enable_nee=0)
    img = acc[..., :3] / acc[..., 3:4]
    lit = img.max(axis=2) > 0.0061
    # without NEE the only radiance above ambient is light seen directly or through bounces: must be finite and non-negative
    assert np.isfinite(img).all() and (img >= 0).all() and lit.any()


def test_nee_on_off_agree_in_expectation(oracle_mod):
    from path_tracer_amd import scenes
    sc = scenes.cornell_box(24, 24)
    o = oracle_mod.Oracle(sc)
    a, _, _, _ = o.render(24, 24, 256, max_bounces=5, enable_nee=1)
    b, _, _, _ = o.render(24, 24, 1024, max_bounces=5, enable_nee=0)
    ma = (a[..., :3] / a[..., 3:4])[4:20, 4:20].mean()
    mb = (b[..., :3] / b[..., 3:4])[4:20, 4:20].mean()
    assert abs(ma - mb) / mb < 0.08


def test_accumulation_is_sequential_and_resumable(oracle_mod, cornell64):
    o = oracle_mod.Oracle(cornell64)
    full, pos_f, id_f, _ = o.render(64, 64, 4, max_bounces=4)
    part, _, idp, _ = o.render(64, 64, 2, max_bounces=4)
    part2, pos_p, idp2, _ = o.render(64, 64, 2, first_sample=2, accum=part, ident=idp, max_bounces=4)
    assert_bit_equal(full, part2, "resumed accumulation")
    assert_bit_equal(pos_f, pos_p, "position of last sample")
    assert np.array_equal(id_f, idp2)
    assert (full[..., 3] == 4).all()


def _narrow(sc):
    """the scene seen through a 1-degree lens along the room's view axis: every camera ray crosses the middle of the scene"""
    from path_tracer_amd.scene_desc import Camera
    sc.camera = Camera.new((0.0, 50.0, 1000.0), (0.0, 50.0, 0.0), 1.0, 1.0)
    return sc


@pytest.mark.parametrize("variant,depth", [("a", 2), ("b", 1), ("c", 1)])
def test_oracle_keys_volumes_per_model(oracle_mod, variant, depth):
    """volume.rs:146-162 keys a volume by the address of the material each BLAS owns (blas.rs:167,197): two models of one material
    are two volumes, two instances of one model or one model holding both spheres are one.  A ray through the overlap reaches a
    stack of 2, 1, 1 (counter 8, the deepest stack of the render)."""
    from path_tracer_amd import scenes
    o = oracle_mod.Oracle(_narrow(scenes.media_pair(variant)))
    ctr = o.render(4, 4, 8, max_bounces=3)[3]
    assert ctr.shape == (oracle_mod.N_COUNTERS,) and int(ctr[8]) == depth


def test_oracle_volume_stack_is_unbounded(oracle_mod):
    from path_tracer_amd import scenes
    for n in (1, 5, 9):
        assert int(oracle_mod.Oracle(scenes.media_shells(n)).render(48, 32, 2, max_bounces=12)[3][8]) == n


def _stream_f32(L, seed, px, sm, k):
    s0 = L.pto_stream_state0(seed, int(px), int(sm))
    return np.float32(np.float32(L.pto_wyrand(s0, k) & 0xFFFFFFFF) / np.float32(4294967296.0))


def volume_reference_f64(g, c, absorption_k, incoming, t_max, dist, u_t, u0, u1):
    """volume.rs:32-60 (HG direction on the ONB of -incoming, onb.rs generate_onb), :83-97 (free flight) and :113 (Beer-Lambert) in
    binary64, fed the binary32 material constants and uniforms the stream produced.  Returns scattered, t, z (along -incoming),
    direction, transmission."""
    g, c = np.float64(g), np.float64(c)
    n = -np.asarray(incoming, np.float64)
    t = -np.log(u_t) / c
    if g == 0.0:
        z = 1.0 - 2.0 * u1
    else:
        x = (1.0 - g * g) / (1.0 + g * (1.0 - 2.0 * u1))
        z = (1.0 + g * g - x * x) / (2.0 * g)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2.0 * np.pi * u0
    sign = np.where(np.signbit(n[:, 2]), -1.0, 1.0)
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    c0 = np.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], 1)
    c1 = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], 1)
    d = c0 * (r * np.cos(phi))[:, None] + c1 * (r * np.sin(phi))[:, None] + n * z[:, None]
    tr = np.exp(-np.asarray(absorption_k, np.float64)[None, :] * np.asarray(dist, np.float64)[:, None])
    return ~(t > t_max), t, z, d, tr


def check_volume_eval(out, vol, incoming, t_max, dist, u_t, u0, u1):
    """out (pt_volume_eval / pto_volume_eval rows) against volume_reference_f64.  Tolerances: t and the transmission a few ulp; z
    1e-6 plus the f32 formula's own conditioning (1 - g*g cancels near |g| = 1, and its rounding reaches z through x*x / 2g); the
    whole direction where it is well conditioned (r = sin(theta) > 0.5), z alone elsewhere; a NaN direction only where |z| rounds
    past 1."""
    f32 = np.float32
    g = float(np.clip(f32(vol.g), f32(-0.999), f32(0.999)))
    ak = np.array([f32(a) * f32(vol.k) for a in vol.absorption], np.float64)
    sc, t, z, d, tr = volume_reference_f64(g, f32(vol.c), ak, incoming, t_max.astype(np.float64), dist, u_t, u0, u1)
    # the scatter decision: equal wherever t is not within rounding of t_max
    clear = np.abs(t - t_max) > 1e-6 * np.abs(t) + 1e-30
    assert np.array_equal(out[clear, 0] == 1.0, sc[clear])
    s = out[:, 0] == 1.0
    assert np.all(np.abs(out[s, 1] - t[s]) <= 4e-7 * t[s]), "free-flight distance"
    assert np.all(out[:, 8] == np.where(vol.c != 0.0, np.where(s, 3.0, 1.0), 0.0)), "draws"
    if g == 0.0:
        tol_z = np.full(int(s.sum()), 1e-6)
    else:
        x = (1.0 - g * g) / (1.0 + g * (1.0 - 2.0 * u1[s]))
        tol_z = 1e-6 + 2.0 * 2.0 ** -24 * (x * x * (2.0 / (1.0 - g * g) + 3.0) + 4.0) / (2.0 * abs(g))
    dz = out[s, 2:5].astype(np.float64)
    zz = (dz * -incoming[s].astype(np.float64)).sum(1)
    finite = np.isfinite(dz).all(1)
    assert np.all(np.abs(1.0 - np.abs(z[s][~finite])) < 4 * tol_z[~finite]), "a NaN direction away from |z| = 1"
    assert np.all(np.abs(zz[finite] - z[s][finite]) <= tol_z[finite]), ("z along -incoming", np.max(np.abs(zz[finite] - z[s][finite])))
    good = finite & (np.sqrt(np.maximum(0.0, 1.0 - z[s] ** 2)) > 0.5)
    assert np.all(np.abs(dz[good] - d[s][good]) <= 2 * tol_z[good, None] + 1e-6), "direction"
    # exp(-a * d): the product's rounding is amplified by |a * d| (exp's condition number)
    e = ak[None, :] * dist.astype(np.float64)[:, None]
    with np.errstate(under="ignore"):
        ok = np.abs(out[:, 5:8] - tr) <= 6e-8 * (4.0 + 2.0 * e) * tr + 1e-44
    assert ok.all(), "transmission"


VOLUME_CASES = [(0.0, 1.0 / 50.0, 0.05), (0.3, 1.0 / 80.0, 0.0), (-0.6, 0.5, 1.0), (0.95, 1e-3, 0.01), (0.999, 1.0 / 50.0, 0.05),
                (-0.999, 1.0 / 50.0, 0.05), (-5.0, 2.0, 30.0), (1e-30, 1.0 / 50.0, 0.05), (-0.0, 1.0 / 50.0, 0.05)]


def volume_eval_inputs(n, seed):
    rng = np.random.default_rng(seed)
    inc = rng.normal(size=(n, 3))
    inc = (inc / np.linalg.norm(inc, axis=1, keepdims=True)).astype(np.float32)
    inc[:6] = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1]], np.float32)
    t_max = rng.uniform(0, 400, n).astype(np.float32)
    t_max[::5] = np.inf
    t_max[1::17] = 0.0
    t_max[2::17] = np.float32(1e-42)
    t_max[3::17] = np.float32(3e38)
    dist = rng.uniform(0, 300, n).astype(np.float32)
    dist[::13] = 0.0
    dist[1::13] = np.float32(1e-40)
    return inc, t_max, dist, rng.integers(0, 1 << 22, n).astype(np.uint32), rng.integers(0, 4096, n).astype(np.uint32)


def volume_probe_scene(vol):
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Dielectric, Model
    t, nr = scenes.sphere_mesh(0, (0.0, 0.0, 0.0), 10.0)
    return scenes.media_room(8, 8, [Model.new(t.astype(np.float32), nr.astype(np.float32), Dielectric.new((1.0, 1.0, 1.0), 1.5, vol))])


@pytest.mark.parametrize("g,c,k", VOLUME_CASES)
def test_oracle_volume_eval_matches_binary64(oracle_mod, g, c, k):
    from path_tracer_amd.scene_desc import Volume
    vol = Volume.new((0.4, 0.0, 0.9), k, c, g)
    sc = volume_probe_scene(vol)
    o = oracle_mod.Oracle(sc)
    mi = len(sc.materials()) - 1
    inc, t_max, dist, px, sm = volume_eval_inputs(2000, 7)
    out = np.stack([o.volume_eval(mi, inc[i], t_max[i], dist[i], int(px[i]), int(sm[i]), 2) for i in range(len(px))])
    L = oracle_mod.lib()
    u = np.array([[_stream_f32(L, oracle_mod.DEFAULT_SEED, px[i], sm[i], 2 + j) for j in range(3)] for i in range(len(px))], np.float64)
    check_volume_eval(out, vol, inc, t_max, dist, u[:, 0], u[:, 1], u[:, 2])
