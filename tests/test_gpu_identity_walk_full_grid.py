"""GPU (-m gpu): the identity-walk parity cases of test_gpu_identity_walk.py on launches that fill the resident grid.

The IDENT traversal kernels of LDS-resident scenes run six waves per SIMD (PT_TRACE_WAVES_LDS_IDENT in pt_kernels.hip: 6 x 256 lanes per CU,
393 216 lanes on 256 CUs), the general kernels five: the grids differ, the result must not.  test_gpu_identity_walk.py sends 6 000 rays, which
24 workgroups take; here every launch holds two to three rays per resident lane of the six-wave grid, so that every workgroup claims
chunks, refills, and runs dry beside the others.  Compared: one-ray walk vs general walk (another grid) vs the CPU oracle (no grid)."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_gpu_identity_walk import _edge_rays, _ident_tlas, _tmax

pytestmark = pytest.mark.gpu

N_RAYS = 1_000_000   # > 2 x 256 CUs x 6 workgroups x 256 lanes


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _many_rays():
    """the edge rays (signed zeros, infinities, NaNs) spread among ordinary rays from inside the room"""
    E_O, E_D = _edge_rays()
    rng = np.random.default_rng(21)
    O = rng.uniform(-270, 270, (N_RAYS, 3)).astype(np.float32)
    O[:, 1] += 50.0
    D = rng.normal(size=(N_RAYS, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    at = rng.choice(N_RAYS, 20 * len(E_O), replace=False)
    O[at] = np.tile(E_O, (20, 1))
    D[at] = np.tile(E_D, (20, 1))
    tm = np.resize(_tmax(len(E_O)), N_RAYS)
    return O, D, tm


@pytest.mark.parametrize("scene_name", ["cornell_box", "cornell_mixed"])
def test_full_grid_rays_bit_equal_on_both_walks_and_vs_oracle(api, oracle_mod, scene_name):
    from path_tracer_amd import scenes
    sc = getattr(scenes, scene_name)(32, 32)
    fast = api.Renderer(sc, 32, 32)
    gen = api.Renderer(sc, 32, 32, flags=api.FLAG_GENERAL_WALK)
    assert _ident_tlas(fast) == 3 and _ident_tlas(gen) == 0
    o = oracle_mod.Oracle(sc)
    O, D, tm = _many_rays()
    for which in (0, 1):
        a = fast.trace_closest(O, D, which=which)
        b = gen.trace_closest(O, D, which=which)
        c = o.trace_closest(O, D, which=which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(a[k], b[k], f"{scene_name} tlas{which} closest.{k} ident vs general")
            assert_bit_equal(a[k], c[k], f"{scene_name} tlas{which} closest.{k} vs oracle")
        a = fast.trace_closest(O, D, tm, which=which)
        c = o.trace_closest(O, D, tm, which=which)
        for k in ("inst", "prim", "t"):
            assert_bit_equal(a[k], c[k], f"{scene_name} tlas{which} closest with t_max .{k} vs oracle")
        fa = fast.trace_any(O, D, tm, which=which)
        assert np.array_equal(fa, gen.trace_any(O, D, tm, which=which))
        assert np.array_equal(fa, o.trace_any(O, D, tm, which=which))


@pytest.mark.parametrize("scene_name", ["cornell_box", "cornell_mixed"])
def test_full_grid_frame_bit_equal_on_both_walks_and_vs_oracle(api, oracle_mod, scene_name):
    """a batch of 640 x 640 paths (more than the six-wave grid's lanes) through k_closest<PRIMARY>, k_trace_fused and the shading passes"""
    from path_tracer_amd import scenes
    W = H = 640
    sc = getattr(scenes, scene_name)(W, H)
    a = api.Renderer(sc, W, H, max_bounces=8).render_samples(0, 2)
    b = api.Renderer(sc, W, H, max_bounces=8, flags=api.FLAG_GENERAL_WALK).render_samples(0, 2)
    assert_bit_equal(a, b, f"{scene_name} per-sample radiance, one-ray vs general walk")
    acc, pos, idb = api.Renderer(sc, W, H, max_bounces=8).render(0, 2)
    oacc, opos, oid, _ = oracle_mod.Oracle(sc).render(W, H, 2, max_bounces=8)
    assert_bit_equal(acc, oacc, f"{scene_name} accumulated radiance vs oracle")
    assert_bit_equal(pos, opos, "first-hit position")
    assert np.array_equal(idb, oid)
