"""GPU (-m gpu): the device's traced, lightmapped and probe-lit light against closed-form irradiance (tests/irradiance_closed_common.py): the
lookup kernels with and without visibility, pt_integrate_rays and pt_render on the tilted quad under the polynomial sky, pt_bake_lightmap and
the baked view of its map, pt_bake_probes through bake_probe_grid and the baked view of the grid.  Every expected value is the closed form,
never the host evaluation or the oracle, and every tolerance is the pass rule of the common module: five standard errors of a known
distribution, the sky map's own error and, where it applies, the geometric bias.  Shapes and reasons: tests/test_irradiance_closed_host.py,
which runs the same inputs through the host evaluation and the oracle.  Figures: profiles/r26_closed_form.md."""
import numpy as np
import pytest

import irradiance_closed_common as IC
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
W = H = 16
POINTS = 4097                     # sixteen blocks and one lane
PLACEMENTS = {"vertices": False, "instance": True}
SIDES = {"front": 1.0, "back": -1.0}
VIEW_SAMPLES = 4


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _renderer(api, instanced, **kw):
    r = api.Renderer(IC.placed_scene(instanced), W, H, max_bounces=4, enable_nee=False, **kw)
    r.set_environment(IC.env_map())
    return r


def _view_points(r, n_samples):
    """where the camera rays of samples [0, n_samples) of every pixel meet the quad's plane, quad-local [pixels * n_samples, 3], in binary64
    from pt_primary_ray's host evaluation: the weights a view's mean gives the texels or the probes come from these"""
    centre = IC.to_world([0.5, 0.5, 0.0])
    out = []
    for pixel in range(W * H):
        for s in range(n_samples):
            o, d, _ = r.primary_ray(pixel, s)
            o, d = o.astype(D), d.astype(D)
            out.append(IC.to_local(o + d * (((centre - o) @ IC.NORMAL) / (d @ IC.NORMAL))))
    out = np.array(out)
    assert np.abs(out[:, 2]).max() < 1e-9 and IC.inside_instance_box(out, margin=0.0).all() and (out[:, :2] > 0.1).all() and (out[:, :2] < 0.9).all()
    return out


def _mean(sums):
    assert (sums[..., 3] == sums[0, 0, 3]).all() and sums[0, 0, 3] > 0
    return (sums[..., :3].astype(D) / sums[..., 3:4].astype(D)).reshape(-1, 3).mean(0)


# ---- 6. the lookup kernels
@pytest.mark.parametrize("bias", IC.FIELD_BIASES)
def test_lookup_kernel_on_exact_coefficients_is_the_closed_form(api, bias):
    r = _renderer(api, False)
    r.set_probe_grid(IC.FIELD_ORIGIN, IC.FIELD_CELL, IC.field_coefficients(True), None, bias)
    P, n = IC.field_queries(POINTS, 21, bias)
    want, tol = IC.field_expected(P, n, bias, True)
    got, lit = r.probe_grid_lookup(P, n, on_device=True)
    assert lit.all()
    IC.check(f"device lookup, affine field, bias {bias}", got, want, tol)
    # the same field under depth that hides nothing (every mean 1e6, facing off): the visibility kernel returns the plain kernel's bits
    r.set_probe_grid_depth(IC.open_table(), vis_floor=0.0, facing=False)
    seen, seen_lit = r.probe_grid_lookup(P, n, on_device=True)
    assert_bit_equal(seen, got, f"device, every m1 1e6, facing off, bias {bias}")
    assert np.array_equal(seen_lit, lit)


@pytest.mark.parametrize("facing", [False, True])
def test_visibility_kernel_reweighs_a_constant_field_without_changing_it(api, facing):
    r = _renderer(api, False)
    for bias in IC.FIELD_BIASES:
        P, n = IC.field_queries(POINTS, 31, bias)
        want, tol = IC.field_expected(P, n, bias, False)
        for name, table in IC.depth_tables().items():
            r.set_probe_grid(IC.FIELD_ORIGIN, IC.FIELD_CELL, IC.field_coefficients(False), None, bias)
            bare = r.probe_grid_lookup(P, n, on_device=True)[0]
            r.set_probe_grid_depth(table, vis_floor=0.05, facing=facing)
            got, lit = r.probe_grid_lookup(P, n, on_device=True)
            assert lit.all()
            IC.check(f"device lookup, constant field, {name} depth, facing {facing}, bias {bias}", got, want, tol)
            assert name != "mixed" or not np.array_equal(got, bare)


# ---- 7. path traced
def _rays(side):
    o, d = IC.interior_rays(4096, 51, side)
    return o, d, (np.arange(4096) + 7000).astype(np.uint32), np.zeros(4096, np.uint32)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("walk", ["vertices", "instance", "vertices, general walk"])
def test_integrate_rays_reflects_albedo_times_the_closed_form(api, walk, side):
    k = SIDES[side]
    r = _renderer(api, walk == "instance", flags=api.FLAG_GENERAL_WALK if "general" in walk else 0)
    rad, pos, ident = r.integrate_rays(*_rays(k))
    assert (ident == 0).all() and (pos[:, 3] < 4.0).all()                                 # every ray meets the quad
    local = IC.to_local(pos[:, :3])
    assert np.abs(local[:, 2]).max() < 1e-5 and (local[:, :2] > 0.05).all() and (local[:, :2] < 0.95).all()
    n = k * IC.NORMAL
    IC.check(f"pt_integrate_rays, {walk}, {side}", rad[:, :3].astype(D).mean(0), IC.ALBEDO * IC.SKY.irradiance(n),
             IC.bound(IC.sigma_cos(n), 4096, IC.ALBEDO * IC.delta_env()[0 if k > 0 else 1]))


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_render_of_the_quad_is_albedo_times_the_closed_form(api, placement):
    r = _renderer(api, PLACEMENTS[placement])
    r.set_camera(IC.close_camera(1.0))
    acc, pos, ident = r.render(0, 64)
    local = IC.to_local(pos[..., :3].reshape(-1, 3))
    assert (ident == 0).all() and (acc[..., 3] == 64).all()                               # every ray of every pixel met the quad ...
    assert np.abs(local[:, 2]).max() < 1e-5 and (local[:, :2] > 0.1).all() and (local[:, :2] < 0.9).all()      # ... in its interior
    want = IC.ALBEDO * IC.SKY.irradiance(IC.NORMAL)
    IC.check(f"pt_render, {placement}, 16 x 16 x 64", _mean(acc), want,
             IC.bound(IC.sigma_cos(IC.NORMAL), W * H * 64, IC.ALBEDO * IC.delta_env()[0]) + IC.fold_rounding(64, want))


# ---- 8. lightmap
def test_lightmap_of_the_instanced_quad_is_the_closed_form(api):
    r = _renderer(api, True)
    n_samples = 256
    sums, cov = r.bake_lightmap(0, 0, 8, 8, n_samples, bias=0.25)
    assert (cov == 1).all()
    texel = sums.astype(D).reshape(64, 3) / n_samples
    want, sigma, delta = IC.SKY.irradiance(IC.NORMAL), IC.sigma_cos(IC.NORMAL) / IC.ALBEDO, IC.delta_env()[0]
    rounding = IC.fold_rounding(n_samples, want)
    IC.check("pt_bake_lightmap, mean of 8 x 8 texels x 256", texel.mean(0), want, IC.bound(sigma, 64 * n_samples, delta) + rounding)
    IC.check("pt_bake_lightmap, every texel at 6 sigma", texel, want, IC.bound(sigma, n_samples, delta, sigmas=6.0) + rounding)
    # the baked view of that map: R times a blend of texel means, weighed as the pixels' rays fall on the texels (the lookup of
    # pt_set_lightmap: texel (i, j) has its centre at ((i + .5) / 8, (j + .5) / 8), clamp to edge); Kish's count of the samples behind it
    r.set_lightmap_sums(0, 0, sums, n_samples)
    r.set_camera(IC.close_camera(1.0))
    view = r.render_baked(0, VIEW_SAMPLES)
    st = _view_points(r, VIEW_SAMPLES)[:, :2]
    weight = np.zeros((8, 8))
    x = np.clip(8.0 * st - 0.5, 0.0, 7.0)
    x0 = np.floor(x).astype(np.int64); f = x - x0; x1 = np.minimum(x0 + 1, 7)
    for ix, wx in ((x0[:, 0], 1 - f[:, 0]), (x1[:, 0], f[:, 0])):
        for iy, wy in ((x0[:, 1], 1 - f[:, 1]), (x1[:, 1], f[:, 1])):
            np.add.at(weight, (iy, ix), wx * wy / len(st))
    assert abs(weight.sum() - 1.0) < 1e-12
    effective = n_samples / np.square(weight).sum()
    print(f"baked view of the map: {int((weight > 0).sum())} texels in view, {effective:.0f} effective samples")
    want = IC.ALBEDO * want
    IC.check("pt_render_baked of the baked map", _mean(view), want,
             IC.bound(IC.sigma_cos(IC.NORMAL), effective, IC.ALBEDO * delta) + IC.fold_rounding(n_samples + VIEW_SAMPLES, want))


# ---- 9. probes
@pytest.mark.parametrize("depth_res", [0, 4])
def test_probe_lit_view_of_the_quad_is_albedo_times_the_closed_form(api, depth_res):
    """2 x 2 x 2 nodes around the quad, 4 096 samples each, no lightmap: the baked view's probe ending lights the front face with the lookup
    at n and the back face with the lookup at -n (the normal on the side the ray came from).  With depth the answer is the same within the
    rule: nothing but the tiny quad occludes."""
    r = _renderer(api, True)
    n_samples = 4096
    _, valid = r.bake_probe_grid(IC.PROBE_ORIGIN, (IC.PROBE_CELL,) * 3, IC.PROBE_COUNT, n_samples, depth_res=depth_res)
    assert valid.all() and r.probe_grid_info()[2] == IC.PROBE_COUNT and r.probe_grid_depth_info()[0] == depth_res
    bias, _ = IC.geometric_bias()
    for i, (side, k) in enumerate(SIDES.items()):
        r.set_camera(IC.close_camera(k))
        view = r.render_baked(0, VIEW_SAMPLES)
        corner = IC.trilinear_weights(IC.to_world(_view_points(r, VIEW_SAMPLES))).mean(0)      # the nodes' weights in the mean over the pixels
        assert abs(corner.sum() - 1.0) < 1e-12
        n = k * IC.NORMAL
        want = IC.ALBEDO * IC.SKY.irradiance(n)
        IC.check(f"pt_render_baked of the probe grid, depth_res {depth_res}, {side}", _mean(view), want,
                 IC.bound(IC.ALBEDO * IC.sigma_sph(n), n_samples / np.square(corner).sum(), IC.ALBEDO * IC.delta_env()[i], IC.ALBEDO * bias)
                 + IC.fold_rounding(n_samples + VIEW_SAMPLES, want))
