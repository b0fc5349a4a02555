"""GPU: the surface materials and the explicit-light arithmetic at their edges.  The probes (pt_material_eval, pt_bsdf_eval) against the
oracle bit for bit and against the binary64 statement of tests/materials_common.py; statistics of 10^6 device draws that the
reference's own code implies; designed rays at a one-plate scene through every variant of the real shading kernels against
Oracle.integrate; and one composition that needs no oracle."""
import numpy as np
import pytest

import materials_common as MC
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = list(MC.materials())


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- a. the probes
@pytest.mark.parametrize("name", NAMES)
def test_material_eval_matches_oracle_and_binary64(api, oracle_mod, name):
    e = MC.oracle_edge_outputs(oracle_mod, name)
    inc, nrm, front, px, sm = e["inputs"]
    r = api.Renderer(e["scene"], 8, 8)
    for n in MC.PROBE_SIZES:                                           # one thread, one short of a block, a block, one over
        got = r.material_eval(e["index"], inc[:n], nrm[:n], front[:n], px[:n], sm[:n], MC.DRAWS_CONSUMED)
        assert_bit_equal(got, e["out"][:n], f"{name}: the first {n} rows")
    got = r.material_eval(e["index"], inc, nrm, front, px, sm, MC.DRAWS_CONSUMED)
    assert_bit_equal(got, e["out"], f"{name}: pt_material_eval")
    MC.check_material_eval(got, e["m"], inc, nrm, front, e["u"])


@pytest.mark.parametrize("name", NAMES)
def test_bsdf_eval_matches_oracle_and_binary64(api, oracle_mod, name):
    e = MC.oracle_edge_outputs(oracle_mod, name)
    bi = e["bsdf_inputs"]
    r = api.Renderer(e["scene"], 8, 8)
    for n in MC.PROBE_SIZES:
        assert_bit_equal(r.bsdf_eval(e["index"], *[a[:n] for a in bi]), e["out4"][:n], f"{name}: the first {n} rows")
    got = r.bsdf_eval(e["index"], *bi)
    assert_bit_equal(got, e["out4"], f"{name}: pt_bsdf_eval")
    MC.check_bsdf_eval(got, e["m"], *bi)


# ---- b. statistics over 10^6 draws on the device: only what the reference's own code implies
N_STAT = 1_000_000


def _stat_keys(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, N_STAT, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 16, N_STAT).astype(np.uint32)


def _probe(api, name):
    m = MC.materials()[name]
    sc, mi = MC.probe_scene(m)
    return m, api.Renderer(sc, 8, 8), mi


def test_lambertian_cosine_statistics(api):
    """utility.rs:7-19: z = sqrt(1 - u1) has mean 2/3 and variance 1/2 - 4/9; the tangential components r cos(phi), r sin(phi) have mean 0
    and variance 1/4.  Five standard deviations of the sample mean over n draws."""
    m, r, mi = _probe(api, "lambertian")
    nrm = np.broadcast_to(MC._normals()[10], (N_STAT, 3))
    inc = np.broadcast_to(-MC._normals()[10], (N_STAT, 3))
    px, sm = _stat_keys(41)
    out = r.material_eval(mi, inc, nrm, np.ones(N_STAT, np.uint8), px, sm, MC.DRAWS_CONSUMED).astype(np.float64)
    c0, c1 = MC._onb(nrm[:1].astype(np.float64))
    z, x, y = out[:, 0:3] @ nrm[0].astype(np.float64), out[:, 0:3] @ c0[0], out[:, 0:3] @ c1[0]
    print("mean cosine", z.mean(), "tangential", x.mean(), y.mean())
    assert abs(z.mean() - 2.0 / 3.0) < 5.0 * np.sqrt((0.5 - 4.0 / 9.0) / N_STAT)
    assert abs(x.mean()) < 5.0 * np.sqrt(0.25 / N_STAT) and abs(y.mean()) < 5.0 * np.sqrt(0.25 / N_STAT)
    assert (out[:, 8] == 2).all()


def test_smooth_dielectric_reflects_a_fresnel_fraction(api):
    """material.rs:496-509: a sample is reflected when u < f(cosine, eta); three incidences per side, the fraction against the binary64
    value of Dielectric::f within five standard deviations of the binomial"""
    m, r, mi = _probe(api, "dielectric")
    c = MC.Constants(m)
    cases = [(1, 0.0), (1, 1.0), (1, 1.45), (0, 0.0), (0, 0.5), (0, 0.72)]            # (front, incidence): 0.72 is just inside the critical angle
    n = N_STAT // len(cases)
    normal = MC._normals()[11]
    px, sm = _stat_keys(43)
    for k, (front, theta) in enumerate(cases):
        inc = np.broadcast_to(MC._directions(normal[None], np.array([theta]), np.array([0.4])), (n, 3))
        nrm = np.broadcast_to(normal, (n, 3))
        sl = slice(k * n, (k + 1) * n)
        out = r.material_eval(mi, inc, nrm, np.full(n, front, np.uint8), px[sl], sm[sl], MC.DRAWS_CONSUMED).astype(np.float64)
        cosine = -float(inc[0].astype(np.float64) @ normal.astype(np.float64))
        f, _ = MC._dielectric_f(np.array([cosine]), c.eta_scatter(np.array([bool(front)])), MC._Decide(), 0.0)
        got = np.mean(out[:, 0:3] @ normal.astype(np.float64) > 0)
        print(f"front {front} incidence {theta}: reflected {got}, binary64 Fresnel {f[0]}")
        assert 0.0 < f[0] < 1.0 and abs(got - f[0]) < 5.0 * np.sqrt(f[0] * (1.0 - f[0]) / n)


@pytest.mark.parametrize("name", ["glass_0.2", "glass_1.0"])
def test_rough_dielectric_draws_and_reflects_as_binary64_says(api, name):
    """material.rs:326-346: the third number is drawn only when refraction through the sampled half-vector exists, and then the sample
    is reflected with probability Schlick(-incoming . h).  The half-vectors come from the binary64 statement fed the same uniforms: the
    count of three-draw samples must equal binary64's but for the rows within rounding of k = 0; among the three-draw samples the
    number reflected is a sum of Bernoulli draws of mean f_i, within five standard deviations sqrt(sum f_i (1 - f_i))."""
    m, r, mi = _probe(api, name)
    c = MC.Constants(m)
    cases = [(1, 0.3), (1, 1.2), (0, 0.3), (0, 0.65), (0, 1.2)]
    n = N_STAT // len(cases)
    normal = MC._normals()[12]
    px, sm = _stat_keys(47)
    for k, (front, theta) in enumerate(cases):
        inc = np.broadcast_to(MC._directions(normal[None], np.array([theta]), np.array([1.9])), (n, 3))
        nrm = np.broadcast_to(normal, (n, 3))
        fr = np.full(n, front, np.uint8)
        sl = slice(k * n, (k + 1) * n)
        out = r.material_eval(mi, inc, nrm, fr, px[sl], sm[sl], MC.DRAWS_CONSUMED).astype(np.float64)
        u = MC.edge_uniforms(px[sl], sm[sl]).astype(np.float64)
        dec = MC._Decide()
        i64, n64 = inc.astype(np.float64), nrm.astype(np.float64)
        h, th = MC._half_vector(c, i64, n64, u[:, 0], u[:, 1], dec)
        eta = c.eta_scatter(fr.astype(bool))
        refr, _ = MC._refract(i64, h, eta, dec, 4 * MC.EPS + th)
        three = ~np.isnan(refr).any(1)
        near = np.broadcast_to(dec.near["k<=0"], (n,))
        got3 = out[:, 8] == 3
        print(f"{name} front {front} incidence {theta}: three draws {got3.sum()} of {n}, binary64 {three.sum()}, within rounding of k = 0: {near.sum()}")
        assert np.array_equal(got3[~near], three[~near]) and set(out[:, 8]) <= {2.0, 3.0}
        sel = got3 & three
        f0 = ((eta - 1.0) / (eta + 1.0)) ** 2
        f = ((1.0 + MC._dot(i64, h)) ** 5 * (1.0 - f0) + f0)[sel]
        reflected = MC._dot(out[sel, 0:3], h[sel]) > 0
        print(f"    reflected {reflected.sum()} of {sel.sum()}, sum of binary64 Schlick {f.sum()}")
        assert abs(reflected.sum() - f.sum()) < 5.0 * np.sqrt((f * (1.0 - f)).sum())


# ---- c. designed rays through the real shading kernels
def _same(got, want, what):
    assert_bit_equal(got[0], want[0], what + ": radiance")
    assert_bit_equal(got[1], want[1], what + ": position")
    assert np.array_equal(got[2], want[2]), what + ": id byte"


@pytest.mark.parametrize("variant", MC.VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_designed_rays_against_the_oracle(api, oracle_mod, name, variant):
    m = MC.materials()[name]
    o, d, key, sample = MC.designed_rays(m)
    delta = m.kind in (MC.SPECULAR, MC.DIELECTRIC)
    zeros = nonzeros = 0
    for light in MC.LIGHTS:
        lib_scene, _, flags = MC.plate_scene(m, light, variant)
        r = api.Renderer(lib_scene, 16, 16, max_bounces=6, flags=flags)
        for depth in (1, 6):
            for nee in (True, False):
                r.set_config(max_bounces=depth, enable_nee=int(nee))
                r.reset_stats()
                want = MC.oracle_rays(oracle_mod, name, light, variant, depth, nee)
                what = f"{name}, {light}, {variant}, depth {depth}, nee {nee}"
                _same(r.integrate_rays(o, d, key, sample, draws_consumed=1), want, what)
                st = r.stats()
                # the variant the case is meant for: where the BVH lives, which walk, whether shadow rays were cast, whether media passes run
                assert st.lds_scene == (0 if variant == "global" else 1), what
                assert (st.ident_tlas == 0) == (variant == "general"), what
                assert (st.rays_any > 0) == (nee and not delta), what
                assert st.paths == len(key)
                zeros += int((want[0][:, :3] == 0).all(1).sum()); nonzeros += int((want[0][:, :3] != 0).any(1).sum())
        if light == "overhead":
            r.set_config(max_bounces=6, enable_nee=1)
            want = MC.oracle_rays(oracle_mod, name, light, variant, 6, True)
            _same(r.integrate_rays(o, d, key, sample, draws_consumed=1, batch_rays=len(key) // 2 + 3), want, f"{name}, {variant}: batches cut inside the set")
            # the camera kernels: a 16 x 16 render from the grazing camera
            orc = oracle_mod.Oracle(MC.plate_scene(m, light, variant)[1])
            acc, pos, idb, _ = orc.render(16, 16, 4, max_bounces=6)
            got = r.render(0, 4)
            assert_bit_equal(got[0], acc, f"{name}, {variant}: render"); assert_bit_equal(got[1], pos, f"{name}, {variant}: render position")
            assert np.array_equal(got[2], idb)
            assert (idb & 0xff != 255).any() and (idb & 0xff == 255).any()
    # the expected set is not trivial.  A Lambertian, Specular or nearly smooth metal plate returns at least the ambient term along every
    # designed path, so exact zeros are demanded only of the materials that can lose a path (test_materials_host.py shows the rough
    # metal's come from the finisher)
    assert nonzeros > 0 and (zeros > 0 or name not in MC.YIELDS_ZEROS)
    if variant == "volumes":
        assert any(mm.volume is not None for mm in lib_scene.materials())
    if variant == "textured":
        assert lib_scene.materials()[1].texture is not None


@pytest.mark.parametrize("flags", [0, 2, 16], ids=["lds", "global", "general"])
def test_a_nan_pdf_after_gathered_light_is_walked_past(api, oracle_mod, flags):
    """materials_common.nan_pdf_scene: under the committed keys the path gathers light on the Lambertian plate, then the smooth dielectric
    sheet answers a NaN pdf (a draw of exactly 1.0 under total internal reflection).  integrator.rs:243 ends a path only on pdf < 0, which
    a NaN is not; the sum turns NaN and the finisher returns zero.  A shading pass that tested pdf >= 0 would return the gathered light."""
    sc = MC.nan_pdf_scene()
    orc = oracle_mod.Oracle(sc)
    o, d, key, sample = MC.nan_pdf_rays()
    want = [orc.integrate(o[i], d[i], int(key[i]), 0, MC.DRAWS_CONSUMED, max_bounces=6) for i in range(len(key))]
    want = (np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), np.array([w[2] for w in want], np.uint8))
    n = len(key) // 2
    assert (want[0][:n, :3] == 0).all() and (want[0][n:, :3] > 0).any()
    r = api.Renderer(sc, 16, 16, max_bounces=6, flags=flags)
    _same(r.integrate_rays(o, d, key, sample, draws_consumed=MC.DRAWS_CONSUMED), want, f"NaN pdf, flags {flags}")


# ---- d. one composition that needs no oracle
def test_specular_plate_returns_the_light_times_its_colour(api):
    """Specular, no next-event estimation, max_bounces 1: the path weight after the plate is 1 * colour / 1 (material.rs:155, integrator.rs:249);
    a mirror direction that hits the light returns emitted * colour (integrator.rs:211), one that misses the ambient 0.006 * colour (:265)"""
    m = MC.materials()["specular"]
    colour = np.array(m.colour, F)
    sc, _, _ = MC.plate_scene(m, "overhead")
    r = api.Renderer(sc, 16, 16, max_bounces=1, enable_nee=False)
    toward = np.array([[0.1, 1.0, 0.05], [-0.15, 1.0, 0.1], [0.9, 1.0, 0.0], [0.0, 1.0, -0.7]])           # mirror directions from the hit point: two reach the light
    toward /= np.linalg.norm(toward, axis=1, keepdims=True)
    d = (toward * [1.0, -1.0, 1.0]).astype(F)                                                            # the rays that mirror into them
    o = (np.array([0.2, 0.0, -0.6]) - 3.0 * d.astype(np.float64)).astype(F)          # the hit lies inside one triangle
    rad, pos, idb = r.integrate_rays(o, d, np.arange(4, dtype=np.uint32), np.zeros(4, np.uint32), draws_consumed=1)
    hit = np.array(MC.EMITTED, F) * colour
    miss = F(0.006) * colour
    want = np.array([np.append(v, F(1.0)) for v in (hit, hit, miss, miss)], F)
    assert_bit_equal(rad, want, "specular plate")
    assert (idb != 255).all()
