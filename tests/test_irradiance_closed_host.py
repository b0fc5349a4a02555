"""CPU: traced, lightmapped and probe-lit light against closed-form irradiance (tests/irradiance_closed_common.py), without a GPU.  The sky is
a polynomial of degree <= 2 in the direction, so the irradiance over pi at a normal that sees all of it is known exactly, one term per SH
band: the basis constants of pt_probe_ray, the cosine-lobe factors of the grid's lookup, the 4 pi / n of the wrapper, the orientation of the
equirect sky against the normal and the oracle's three transports are each held to that value and not to a restatement of themselves.
Figures and the mutations each test catches: profiles/r26_closed_form.md.  (The device: tests/test_gpu_irradiance_closed.py.)"""
import numpy as np
import pytest

import irradiance_closed_common as IC

F = np.float32
D = np.float64


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def plain(api):
    """a context for the host hooks that need no particular scene"""
    return api.Renderer(IC.placed_scene(False), 16, 16, enable_nee=False)


def _field_grid(r, affine, bias):
    r.set_probe_grid(IC.FIELD_ORIGIN, IC.FIELD_CELL, IC.field_coefficients(affine), None, bias)


# ---- 1. the basis
def test_probe_ray_basis_is_the_normalised_harmonics(plain):
    """pt_probe_ray's y0..y8 at its own d against the basis built from the normalisation formulas: 1e-6 absolute covers at most 4 roundings
    of values <= 1.1 (2.6e-7) and the 8-digit constants (5e-8 relative)"""
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 2 ** 32, 2000, dtype=np.uint64); samples = rng.integers(0, 2 ** 20, 2000, dtype=np.uint64)
    keys[:4] = (0, 1, 2 ** 32 - 1, 12345); samples[:4] = (0, 1, 511, 512)
    rays = [plain.probe_ray(int(k), int(s)) for k, s in zip(keys, samples)]
    d = np.array([q[0] for q in rays], D); y = np.array([q[1] for q in rays], D)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-6
    worst = np.abs(y - IC.sh9(d)).max(0)
    print("closed-form check | basis | worst |y - basis| per function, in units of 1e-6:", np.round(worst / 1e-6, 3).tolist())
    assert worst.max() <= 1e-6, f"basis function {int(worst.argmax())}: {worst.max() / 1e-6:.3f} times the bound"
    assert len(np.unique(np.round(d, 3), axis=0)) > 1900                                  # and the directions do cover the sphere
    assert np.abs(d.mean(0)).max() < 5.0 * np.sqrt(1.0 / 3.0 / 2000)                       # uniform: each component has variance 1/3


# ---- 2. the lookup from exact coefficients
@pytest.mark.parametrize("bias", IC.FIELD_BIASES)
def test_lookup_of_exact_coefficients_is_the_closed_form(plain, bias):
    """a 3 x 2 x 4 grid whose coefficients vary affinely in position holds, at every point of its box, the exact projection of the sky
    sky0 + (g.p) sky1: the lookup owes I0(n) + (g.p') I1(n) to rounding alone"""
    _field_grid(plain, True, bias)
    P, n = IC.field_queries(1000, 21, bias)
    want, tol = IC.field_expected(P, n, bias, True)
    got, lit = plain.probe_grid_lookup(P, n)
    assert lit.all()
    IC.check(f"host lookup, affine field, bias {bias}", got, want, tol)
    # the test normals on their own: the terms of bands 1 and 2 are at least a quarter of the constant there
    nn = np.repeat(IC.NORMALS, 4, 0).astype(F)
    want, tol = IC.field_expected(P[:8], nn, bias, True)
    got, lit = plain.probe_grid_lookup(P[:8], nn)
    assert lit.all()
    IC.check(f"host lookup, affine field, bias {bias}, the quad's normals", got, want, tol)


# ---- 3. visibility changes weights, not light
@pytest.mark.parametrize("facing", [False, True])
def test_visibility_reweighs_a_constant_field_without_changing_it(plain, facing):
    for bias in IC.FIELD_BIASES:
        P, n = IC.field_queries(1000, 31, bias)
        want, tol = IC.field_expected(P, n, bias, False)
        for name, table in IC.depth_tables().items():
            _field_grid(plain, False, bias)
            bare = plain.probe_grid_lookup(P, n)[0]
            plain.set_probe_grid_depth(table, vis_floor=0.05, facing=facing)
            got, lit = plain.probe_grid_lookup(P, n)
            assert lit.all()                                                              # the floor keeps every corner in
            IC.check(f"host lookup, constant field, {name} depth, facing {facing}, bias {bias}", got, want, tol)
            assert name != "mixed" or not np.array_equal(got, bare)                       # the weights did change: other roundings


def test_open_depth_is_the_plain_lookup_bit_for_bit(plain):
    from conftest import assert_bit_equal
    for bias in IC.FIELD_BIASES:
        P, n = IC.field_queries(1000, 41, bias)
        _field_grid(plain, True, bias)
        bare = plain.probe_grid_lookup(P, n)
        plain.set_probe_grid_depth(IC.open_table(), vis_floor=0.0, facing=False)
        assert plain.probe_grid_depth_info()[0] == IC.DEPTH_RES
        seen = plain.probe_grid_lookup(P, n)
        assert_bit_equal(seen[0], bare[0], f"every m1 1e6, facing off, bias {bias}")
        assert np.array_equal(seen[1], bare[1]) and bare[1].all()


# ---- 4. the wrapper's unit
def fold_probe_rays(r, radiance_of, keys, n_samples):
    """raw sums [len(keys), 9, 3] float32 of radiance_of(key, d [n, 3]) [n, 3] times pt_probe_ray's own y over its own directions, folded in
    binary64: what pt_bake_probes hands set_probe_grid_sums"""
    sums = np.zeros((len(keys), 9, 3))
    for j, key in enumerate(keys):
        rays = [r.probe_ray(int(key), s) for s in range(n_samples)]
        d = np.array([q[0] for q in rays], D); y = np.array([q[1] for q in rays], D)
        sums[j] = y.T @ radiance_of(int(key), d)
    return sums.astype(F)


def test_sums_through_the_wrapper_light_a_surface_with_the_closed_form(plain):
    """64 keys x 1 024 samples of the analytic sky through set_probe_grid_sums into a 4 x 4 x 4 grid, looked up at the nodes: the mean over the
    nodes is a mean of 65 536 independent samples of the sphere estimator"""
    n_samples = 1024
    sums = fold_probe_rays(plain, lambda key, d: IC.SKY.radiance(d), range(64), n_samples)
    plain.set_probe_grid_sums((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), sums.reshape(4, 4, 4, 9, 3), n_samples)
    nodes = plain.probe_grid_positions((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4)).reshape(-1, 3)
    for n in IC.NORMALS:
        got, lit = plain.probe_grid_lookup(nodes, np.repeat(n[None], 64, 0))
        assert lit.all()
        IC.check("set_probe_grid_sums, 64 x 1024 samples of the analytic sky", got.astype(D).mean(0), IC.SKY.irradiance(n),
                 IC.bound(IC.sigma_sph(n), 64 * n_samples))


# ---- 5. the oracle's three transports on the quad
PLACEMENTS = {"vertices": False, "instance": True}
SIDES = {"front": 1.0, "back": -1.0}


@pytest.fixture(scope="module")
def oracles(oracle_mod):
    out = {}
    for name, instanced in PLACEMENTS.items():
        orc = oracle_mod.Oracle(IC.placed_scene(instanced))
        orc.set_environment(IC.env_map())
        out[name] = orc
    return out


def _integrate(orc, o, d, keys, samples, want_id=None):
    out = [orc.integrate(o[i], d[i], int(keys[i]), int(samples[i]), 1, max_bounces=4, enable_nee=0) for i in range(len(o))]
    assert want_id is None or all(q[2] == want_id for q in out)
    return np.array([q[0][:3] for q in out], D)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_oracle_integrate_reflects_albedo_times_the_closed_form(oracles, placement, side):
    k = SIDES[side]
    o, d = IC.interior_rays(4096, 51, k)
    rad = _integrate(oracles[placement], o, d, np.arange(4096) + 7000, np.zeros(4096), want_id=0)        # every ray meets the quad
    n = k * IC.NORMAL
    IC.check(f"oracle integrate, {placement}, {side}", rad.mean(0), IC.ALBEDO * IC.SKY.irradiance(n),
             IC.bound(IC.sigma_cos(n), 4096, IC.ALBEDO * IC.delta_env()[0 if k > 0 else 1]))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("placement", PLACEMENTS)
def test_oracle_traced_lightmap_estimator_is_the_closed_form(api, oracles, placement, side):
    """pt_lightmap_ray's directions from the texel positions (pt_lightmap_texels, host evaluation; the back face: the normal negated),
    8 x 8 texels x 256 samples, each traced by the oracle: the mean of a texel is the lightmap's unit, irradiance over pi"""
    k = SIDES[side]
    r = api.Renderer(IC.placed_scene(PLACEMENTS[placement]), 16, 16, enable_nee=False)
    prim, _, position, normal = r.lightmap_texels(0, 0, 8, 8)
    assert (prim != 0xFFFFFFFF).all()
    position = position.reshape(-1, 3).astype(D); normal = (k * normal.reshape(-1, 3)).astype(F)
    assert np.abs(normal.astype(D) - k * IC.NORMAL).max() < 1e-6                           # the table's normal is the tilted quad's
    centres = np.stack(np.meshgrid((np.arange(8) + 0.5) / 8, (np.arange(8) + 0.5) / 8), -1).reshape(-1, 2)
    assert np.abs(position - IC.to_world(np.concatenate([centres, np.zeros((64, 1))], 1))).max() < 1e-6
    means = np.zeros((64, 3))
    for t in range(64):
        d = np.array([r.lightmap_ray(t, s, normal[t]) for s in range(256)], F)
        o = np.repeat((position[t] + 0.25 * normal[t].astype(D)).astype(F)[None], 256, 0)
        means[t] = _integrate(oracles[placement], o, d, np.full(256, t), np.arange(256), want_id=255).mean(0)      # and none of these does
    n = k * IC.NORMAL
    IC.check(f"oracle-traced lightmap estimator, {placement}, {side}", means.mean(0), IC.SKY.irradiance(n),
             IC.bound(IC.sigma_cos(n) / IC.ALBEDO, 64 * 256, IC.delta_env()[0 if k > 0 else 1]))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_oracle_traced_probe_fold_is_the_closed_form(plain, oracles, placement):
    """pt_probe_ray's directions from the 8 nodes around the quad (each more than 30 quad sides from it), traced by the oracle, folded,
    passed through the wrapper and looked up at the nodes.  The quad hides a sliver of the sky: the geometric bias."""
    n_samples = 1024
    nodes = IC.probe_nodes().astype(F)
    orc = oracles[placement]

    def traced(key, d):
        o = np.repeat(nodes[key][None], len(d), 0)
        return _integrate(orc, o, d.astype(F), np.full(len(d), key), np.arange(len(d)))
    sums = fold_probe_rays(plain, traced, range(8), n_samples)
    plain.set_probe_grid_sums(IC.PROBE_ORIGIN, (IC.PROBE_CELL,) * 3, sums.reshape(2, 2, 2, 9, 3), n_samples)
    bias, _ = IC.geometric_bias()
    for i, n in enumerate(IC.NORMALS):
        got, lit = plain.probe_grid_lookup(nodes, np.repeat(n[None], 8, 0))
        assert lit.all()
        IC.check(f"oracle-traced probe fold, {placement}, normal {'+-'[i]}n", got.astype(D).mean(0), IC.SKY.irradiance(n),
                 IC.bound(IC.sigma_sph(n), 8 * n_samples, IC.delta_env()[i], bias))
