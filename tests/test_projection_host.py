"""CPU: panoramic and orthographic cameras (pt_set_projection, pt_get_projection, pt_primary_ray, pt_active_pixels).  No GPU is touched.
The definition is restated in tests/projection_common.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from projection_common import ORTHOGRAPHIC, PANORAMA, PERSPECTIVE, projection_rays

F = np.float32
ARG, STATE = -1, -3
TILTED = ((300.0, 220.0, 700.0), (-40.0, 10.0, -90.0), 50.0, 1.5)   # test_host.py's arbitrary camera
SIZES = [(32, 24), (7, 5)]
SAMPLES = (0, 5, 300)
SPANS = [(0.0, 0.0), (90.0, 60.0), (360.0, 180.0)]
NEW_SYMBOLS = ["pt_set_projection", "pt_get_projection"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _pair(api, O, pose, W, H):
    """a library context and an oracle on the Cornell box under the same camera.  pose "reference": the reference's camera; "input": the tilted camera
    of test_host.py moved on by Camera::input events (a key and a mouse drag), in both"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    sc = scenes.cornell_box(W, H)
    aspect = W / H
    if pose == "input":
        aspect = TILTED[3]
        sc = SceneDesc.new(sc.models, Camera.new(*TILTED), sc.name)
    r, orc = api.Renderer(sc, W, H), O.Oracle(sc)
    if pose == "input":
        for ev in [(api.EV_KEY_W, 0.0, 0.0, 3e-5), (api.EV_MOUSE_MOTION, 40.0, -15.0, 2e-4), (api.EV_KEY_D, 0.0, 0.0, 1e-5)]:
            assert r.camera_input(*ev) and orc.camera_input(*ev)
    return r, orc, aspect


def _library_rays(r, pixels, sample):
    o = np.zeros((len(pixels), 3), F); d = np.zeros((len(pixels), 3), F)
    draws = set()
    for i, p in enumerate(pixels):
        o[i], d[i], k = r.primary_ray(int(p), sample)
        draws.add(k)
    return o, d, draws


def test_new_symbols_are_exported(api):
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(L, name), name
    assert (api.PROJ_PERSPECTIVE, api.PROJ_PANORAMA, api.PROJ_ORTHOGRAPHIC) == (PERSPECTIVE, PANORAMA, ORTHOGRAPHIC)
    assert C.sizeof(api.Projection) == 32


@pytest.mark.parametrize("pose", ["reference", "input"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("spans", SPANS, ids=lambda s: f"{s[0]:g}-{s[1]:g}")
def test_panorama_ray_is_the_definition(api, oracle_mod, pose, size, spans):
    W, H = size
    r, orc, _ = _pair(api, oracle_mod, pose, W, H)
    r.set_projection(api.PROJ_PANORAMA, *spans)
    pixels = np.arange(W * H)
    for s in SAMPLES:
        o, d, draws = projection_rays(oracle_mod, orc, W, H, pixels, s, PANORAMA, *spans)
        go, gd, gdraws = _library_rays(r, pixels, s)
        assert gdraws == {1} and draws == 1
        assert_bit_equal(go, o, f"origin, sample {s}")
        assert_bit_equal(gd, d, f"direction, sample {s}")


@pytest.mark.parametrize("pose", ["reference", "input"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("height", [600.0, 37.5])
def test_orthographic_ray_is_the_definition(api, oracle_mod, pose, size, height):
    W, H = size
    r, orc, aspect = _pair(api, oracle_mod, pose, W, H)
    # spans are not looked at by ORTHOGRAPHIC beyond their validation
    r.set_projection(api.PROJ_ORTHOGRAPHIC, 90.0, 60.0, ortho_height=height)
    pixels = np.arange(W * H)
    for s in SAMPLES:
        o, d, draws = projection_rays(oracle_mod, orc, W, H, pixels, s, ORTHOGRAPHIC, ortho_height=height, aspect=aspect)
        go, gd, gdraws = _library_rays(r, pixels, s)
        assert gdraws == {1} and draws == 1
        assert_bit_equal(go, o, f"origin, sample {s}")
        assert_bit_equal(gd, d, f"direction, sample {s}")
    assert len(np.unique(gd, axis=0)) == 1 and len(np.unique(go, axis=0)) == W * H, "parallel rays from distinct origins"


def test_geometry_of_the_two_cameras(api, oracle_mod):
    """binary64 sanity of the binary32 rays, so that the restatement and the library cannot agree on nonsense: a full panorama's centre pixel looks
    along -c2, its columns sweep the azimuth monotonically through +-180 degrees, its top row looks up; an orthographic frame spans
    ortho_height x ortho_height * aspect in the camera's plane"""
    W, H = 32, 24
    r, _, aspect = _pair(api, oracle_mod, "reference", W, H)
    m34 = r.camera_matrices()[0].astype(np.float64)
    eye, c0, c1, c2 = m34[:, 3], m34[:, 0], m34[:, 1], m34[:, 2]
    r.set_projection(api.PROJ_PANORAMA)
    o, d, _ = _library_rays(r, np.arange(W * H), 0)
    d = d.astype(np.float64).reshape(H, W, 3)
    assert np.array_equal(o, np.tile(eye.astype(F), (W * H, 1)))
    assert np.abs(np.linalg.norm(d, axis=2) - 1).max() < 1e-6
    az = np.degrees(np.arctan2(d @ c0, -(d @ c2)))[H // 2]
    el = np.degrees(np.arcsin(np.clip(d @ c1, -1, 1)))[:, W // 2]
    assert np.all(np.diff(az) > 0) and az[0] < -165 and az[-1] > 165 and abs(az[W // 2]) < 360 / W
    assert np.all(np.diff(el) > 0) and el[0] < -80 and el[-1] > 80, "row 0 is the bottom row"
    r.set_projection(api.PROJ_ORTHOGRAPHIC, ortho_height=600.0)
    o, d, _ = _library_rays(r, np.arange(W * H), 0)
    off = o.astype(np.float64) - eye
    assert np.abs(d.astype(np.float64) - (-c2 / np.linalg.norm(c2))).max() < 1e-6
    assert np.abs(off @ c2).max() < 1e-3
    assert 600.0 * aspect * (1 - 2 / W) < np.ptp(off @ c0) < 600.0 * aspect and 600.0 * (1 - 2 / H) < np.ptp(off @ c1) < 600.0


def test_refusals_change_nothing(api, oracle_mod):
    W, H = 32, 24
    r, _, _ = _pair(api, oracle_mod, "reference", W, H)
    assert r.get_projection() == (PERSPECTIVE, 0.0, 0.0, 0.0)
    r.set_projection(api.PROJ_PANORAMA, 90.0, 60.0)
    prior = r.get_projection()
    assert prior == (PANORAMA, 90.0, 60.0, 0.0)
    ray = r.primary_ray(100, 5)
    nan, inf = float("nan"), float("inf")
    bad = [(3, 0.0, 0.0, 0.0), (0xFFFFFFFF, 0.0, 0.0, 0.0),
           (PANORAMA, -1.0, 0.0, 0.0), (PANORAMA, 0.0, -1.0, 0.0), (PANORAMA, nan, 0.0, 0.0), (PANORAMA, 0.0, nan, 0.0), (PANORAMA, inf, 0.0, 0.0),
           (PANORAMA, 0.0, inf, 0.0), (PANORAMA, 360.5, 0.0, 0.0), (PANORAMA, 0.0, 180.5, 0.0), (PERSPECTIVE, -1.0, 0.0, 0.0), (ORTHOGRAPHIC, nan, 0.0, 10.0),
           (ORTHOGRAPHIC, 0.0, 0.0, 0.0), (ORTHOGRAPHIC, 0.0, 0.0, -5.0), (ORTHOGRAPHIC, 0.0, 0.0, nan), (ORTHOGRAPHIC, 0.0, 0.0, inf)]
    for b in bad:
        with pytest.raises(api.PtError) as e:
            r.set_projection(*b)
        assert e.value.code == ARG, b
        assert r.get_projection() == prior, b
    for word in range(4):
        p = api.Projection(PANORAMA, 10.0, 10.0, 0.0)
        p.reserved[word] = 1
        assert r.L.pt_set_projection(r.ctx, C.byref(p)) == ARG
        assert r.get_projection() == prior
    assert r.L.pt_get_projection(r.ctx, None) == ARG and r.L.pt_set_projection(None, None) == ARG
    after = r.primary_ray(100, 5)
    assert_bit_equal(after[0], ray[0], "origin after the refusals")
    assert_bit_equal(after[1], ray[1], "direction after the refusals")
    # the limits themselves are accepted; NULL restores PERSPECTIVE
    r.set_projection(api.PROJ_PANORAMA, 360.0, 180.0)
    assert r.L.pt_set_projection(r.ctx, None) == 0
    assert r.get_projection() == (PERSPECTIVE, 0.0, 0.0, 0.0)


def test_lens_and_projection_exclude_each_other(api, oracle_mod):
    W, H = 32, 24
    r, _, _ = _pair(api, oracle_mod, "reference", W, H)
    r.set_lens(40.0, 800.0)
    lens_ray = r.primary_ray(50, 2)
    for proj in [(PANORAMA, 0.0, 0.0, 0.0), (ORTHOGRAPHIC, 0.0, 0.0, 600.0)]:
        with pytest.raises(api.PtError) as e:
            r.set_projection(*proj)
        assert e.value.code == STATE
        assert r.get_projection()[0] == PERSPECTIVE
    r.set_projection(api.PROJ_PERSPECTIVE)                                    # perspective under a lens is what there was
    again = r.primary_ray(50, 2)
    assert again[2] == 2 and np.array_equal(again[0], lens_ray[0]) and np.array_equal(again[1], lens_ray[1])
    r.set_lens(0.0, 0.0)
    for proj in [(PANORAMA, 0.0, 0.0, 0.0), (ORTHOGRAPHIC, 0.0, 0.0, 600.0)]:
        r.set_projection(*proj)
        ray = r.primary_ray(50, 2)
        with pytest.raises(api.PtError) as e:
            r.set_lens(40.0, 800.0)
        assert e.value.code == STATE
        r.set_lens(0.0, 950.0)                                                # no lens: accepted, the reference's own arguments
        after = r.primary_ray(50, 2)
        assert after[2] == 1 and np.array_equal(after[0], ray[0]) and np.array_equal(after[1], ray[1]), "the refused lens changed nothing"


def test_projection_survives_the_camera_and_culls_nothing(api, oracle_mod):
    from path_tracer_amd import scenes
    W, H = 32, 24
    r, orc, _ = _pair(api, oracle_mod, "reference", W, H)
    pin_rect, box = r.active_pixels()
    assert pin_rect[1] * pin_rect[3] < W * H, "the pinhole frame has a primary cull to lose"
    for proj in [(PANORAMA, 90.0, 60.0, 0.0), (ORTHOGRAPHIC, 0.0, 0.0, 600.0)]:
        r.set_projection(*proj)
        rect, pbox = r.active_pixels()
        assert rect == (0, W, 0, H) and np.array_equal(pbox, box)
        eye, target = (C.c_float * 3)(10.0, 60.0, 900.0), (C.c_float * 3)(0.0, 50.0, 0.0)
        assert r.L.pt_set_camera(r.ctx, eye, target, 55.0, 1.25) == 0
        assert r.camera_input(api.EV_KEY_W, 0.0, 0.0, 1e-4)
        assert r.get_projection() == proj
        assert r.active_pixels()[0] == (0, W, 0, H)
        r.set_camera(scenes.reference_camera(W / H))
        assert r.get_projection() == proj
    # pt_create_ray stays the pinhole ray
    o, d = r.create_ray(0.3, 0.6)
    oo, od = orc.create_ray(0.3, 0.6)
    assert_bit_equal(o, oo, "create_ray origin"); assert_bit_equal(d, od, "create_ray direction")
    r.set_projection(api.PROJ_PERSPECTIVE)
    assert r.active_pixels()[0] == pin_rect


def test_perspective_after_a_round_trip_is_the_old_ray(api, oracle_mod):
    W, H = 32, 24
    r, orc, _ = _pair(api, oracle_mod, "input", W, H)
    pixels = np.arange(W * H)
    before = [_library_rays(r, pixels, s) for s in SAMPLES]
    r.set_projection(api.PROJ_PANORAMA, 90.0, 60.0)
    assert not np.array_equal(_library_rays(r, pixels, 0)[1], before[0][1])
    r.set_projection(api.PROJ_ORTHOGRAPHIC, ortho_height=10.0)
    r.set_projection(api.PROJ_PERSPECTIVE)
    for s, (o, d, draws) in zip(SAMPLES, before):
        go, gd, gdraws = _library_rays(r, pixels, s)
        assert gdraws == draws == {1}
        assert_bit_equal(go, o, f"origin, sample {s}"); assert_bit_equal(gd, d, f"direction, sample {s}")
        want = [orc.primary_ray(W, H, int(p), s) for p in pixels]
        assert_bit_equal(gd, np.array([w[1] for w in want]), f"direction vs the oracle, sample {s}")
