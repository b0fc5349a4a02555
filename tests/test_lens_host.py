"""CPU: the thin lens (pt_set_lens, pt_primary_ray, the lens-aware active rectangle).  No GPU is touched.

`lens_rays` restates the definition of include/pt_api.h in numpy binary32, one rounding per operation, with the oracle's own stream draws,
Sobol points, sin/cos and camera matrices; tests/test_gpu_lens.py feeds its rays to the oracle's integrator for the expected radiance."""
import numpy as np
import pytest

from conftest import assert_bit_equal

F = np.float32
SEED = 0x5EED5EED
TILTED = ((300.0, 220.0, 700.0), (-40.0, 10.0, -90.0), 50.0, 1.5)   # test_host.py's arbitrary camera
LENSES = [(40.0, 800.0), (120.0, 1100.0), (300.0, 600.0)]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _draw(O, state0, k):
    return int(O.lib().pto_wyrand(int(state0), int(k))) & 0xFFFFFFFF


def lens_rays(O, orc, W, H, pixels, sample, aperture, focus, n_sobol=512, seed=SEED, want_q=False):
    """The camera rays of `sample` of the global pixels `pixels` (y * W + x) under the camera of the oracle `orc` and the lens
    (aperture, focus): origins [n, 3], directions [n, 3] and the stream draws consumed.  include/pt_api.h, pt_set_lens, line for line.
    want_q: the definition's q (the pinhole ray before normalising) instead."""
    pixels = np.asarray(pixels, np.int64)
    n = len(pixels)
    m34, _, rm = orc.camera_matrices()          # rm[row][col] = M[col * 4 + row]
    eye, c0, c1 = m34[:, 3].astype(F), m34[:, 0].astype(F), m34[:, 1].astype(F)
    L = O.lib()
    state0 = [L.pto_stream_state0(seed, int(p), int(sample)) for p in pixels]
    jit = np.array([O.ss_sobol(n_sobol, int(sample), _draw(O, s0, 0)) for s0 in state0], F).reshape(n, 2)
    gx, gy = (pixels % W).astype(F), (pixels // W).astype(F)
    ox, oy = jit[:, 0] - F(0.5), jit[:, 1] - F(0.5)
    u, v = (gx + ox) / F(W), (gy + oy) / F(H)
    nx, ny, nz = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0), F(0.0)
    r = []
    for i in range(4):
        t = rm[i, 0] * nx
        t = rm[i, 1] * ny + t
        t = rm[i, 2] * nz + t
        t = rm[i, 3] + t
        r.append(t.astype(F))
    rw = F(1.0) / r[3]
    q = np.stack([r[0] * rw - eye[0], r[1] * rw - eye[1], r[2] * rw - eye[2]], 1).astype(F)

    if want_q:
        return q

    def unit(w):
        l = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        return (w / l[:, None]).astype(F)

    if aperture == 0:
        return np.tile(eye, (n, 1)), unit(q), 1
    lp = np.array([O.ss_sobol(n_sobol, int(sample), _draw(O, s0, 1)) for s0 in state0], F).reshape(n, 2)
    rad = (F(aperture) * F(0.5)) * np.sqrt(lp[:, 0])
    phi = F(6.2831855) * lp[:, 1]
    sn, cs = O.math_batch(0, phi)
    a, b = rad * cs, rad * sn
    o = np.stack([eye[k] + (c0[k] * a + c1[k] * b) for k in range(3)], 1).astype(F)
    f = np.stack([q[:, k] * F(focus) + eye[k] for k in range(3)], 1).astype(F)
    assert o.dtype == F and f.dtype == F and q.dtype == F
    return o, unit((f - o).astype(F)), 2


def _pair(api, O, cam, W, H, scene=None):
    """a library context and an oracle on the same scene and camera (`cam`: Camera.new's first four arguments, or None = the reference's)"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    sc = scene if scene is not None else scenes.cornell_box(W, H)
    if cam is not None:
        sc = SceneDesc.new(sc.models, Camera.new(*cam), sc.name)
    return api.Renderer(sc, W, H), O.Oracle(sc)


def _library_rays(r, pixels, sample):
    o = np.zeros((len(pixels), 3), F); d = np.zeros((len(pixels), 3), F)
    draws = set()
    for i, p in enumerate(pixels):
        o[i], d[i], k = r.primary_ray(int(p), sample)
        draws.add(k)
    return o, d, draws


@pytest.mark.parametrize("cam", [None, TILTED], ids=["reference", "tilted"])
def test_lens_ray_without_a_lens_is_the_oracle_primary_ray(api, oracle_mod, cam):
    W, H = 96, 54
    _, orc = _pair(api, oracle_mod, cam, W, H)
    pixels = np.arange(W * H)
    for s in (0, 1, 511):
        o, d, draws = lens_rays(oracle_mod, orc, W, H, pixels, s, 0.0, 0.0)
        assert draws == 1
        want = [orc.primary_ray(W, H, int(p), s) for p in pixels]
        assert_bit_equal(o, np.array([w[0] for w in want]), f"origin, sample {s}")
        assert_bit_equal(d, np.array([w[1] for w in want]), f"direction, sample {s}")


@pytest.mark.parametrize("cam", [None, TILTED], ids=["reference", "tilted"])
@pytest.mark.parametrize("lens", [(0.0, 0.0)] + LENSES, ids=lambda l: f"{l[0]:g}-{l[1]:g}")
def test_primary_ray_is_the_definition(api, oracle_mod, cam, lens):
    W, H = 96, 54
    r, orc = _pair(api, oracle_mod, cam, W, H)
    r.set_lens(*lens)
    pixels = np.arange(W * H)
    for s in (0, 1, 511):
        o, d, draws = lens_rays(oracle_mod, orc, W, H, pixels, s, *lens)
        go, gd, gdraws = _library_rays(r, pixels, s)
        assert gdraws == {draws} and draws == (2 if lens[0] > 0 else 1)
        assert_bit_equal(go, o, f"origin, sample {s}")
        assert_bit_equal(gd, d, f"direction, sample {s}")


@pytest.mark.parametrize("cam", [None, TILTED], ids=["reference", "tilted"])
@pytest.mark.parametrize("lens", LENSES, ids=lambda l: f"{l[0]:g}-{l[1]:g}")
def test_lens_rays_meet_on_the_plane_of_focus(api, oracle_mod, cam, lens):
    """binary64 geometry of the binary32 rays: every lens ray of a pixel passes within 1e-5 |f - eye| of f, the point where the pixel's pinhole
    ray meets the plane of focus (a few binary32 roundings: the numpy restatement measures 2.3e-7), and starts on the lens disk"""
    W, H = 96, 54
    r, orc = _pair(api, oracle_mod, cam, W, H)
    r.set_lens(*lens)
    m34 = r.camera_matrices()[0].astype(np.float64)
    eye, c0, c1, c2 = m34[:, 3], m34[:, 0], m34[:, 1], m34[:, 2]
    pixels = np.arange(W * H)
    worst = 0.0
    for s in (0, 1, 511):
        q = lens_rays(oracle_mod, orc, W, H, pixels, s, 0.0, 0.0, want_q=True).astype(np.float64)   # the pinhole ray of the same jittered position
        f = eye + q * lens[1]                                                # the definition's f ...
        axial = (f - eye) @ -c2
        # ... lies on the plane of focus: q's axial component is 1 up to the rounding of point and of point - eye, each half an ulp of a
        # coordinate of the eye's size per component
        assert np.abs(axial / lens[1] - 1).max() <= 4 * 2.0 ** -24 * np.abs(eye).max()
        o, d, _ = _library_rays(r, pixels, s)
        o, d = o.astype(np.float64), d.astype(np.float64)
        rel = f - o
        dist = np.linalg.norm(rel - d * np.sum(rel * d, 1)[:, None] / np.sum(d * d, 1)[:, None], axis=1)
        worst = max(worst, float((dist / np.linalg.norm(f - eye, axis=1)).max()))
        off = o - eye
        assert np.linalg.norm(off, axis=1).max() <= lens[0] / 2 * (1 + 1e-5)
        # in the plane spanned by c0, c1, up to the rounding of o's three components (half an ulp of a coordinate of the eye's size each)
        assert np.abs(off @ c2).max() <= 3 * 2.0 ** -24 * np.abs(eye).max() + 1e-6 * lens[0]
        assert np.linalg.norm(off, axis=1).max() > 0.8 * lens[0] / 2, "the samples should reach towards the rim of the disk"
    print(f"largest distance from f to a lens ray, relative to |f - eye|: {worst:.3g}")
    assert worst <= 1e-5


def _box_hit64(o, d, mn, mx):
    """binary64 slab test of the rays o + t d, t >= 0, against the box"""
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t0, t1 = (mn - o) * inv, (mx - o) * inv
        near = np.minimum(t0, t1).max(1)
        far = np.maximum(t0, t1).min(1)
    return np.maximum(near, 0.0) <= far


def _rect_share(rect, W, H):
    return rect[1] * rect[3] / (W * H)


@pytest.mark.parametrize("lens", LENSES, ids=lambda l: f"{l[0]:g}-{l[1]:g}")
def test_lens_rectangle_is_conservative_and_still_culls(api, oracle_mod, lens):
    """No lens ray of a pixel outside pt_active_pixels' rectangle meets the world's root box: every pixel within 6 pixels outside it plus 3000
    random outside pixels, 4 samples each.  And the rectangle is still a cull: under half of the frame (the construction gives about a third)."""
    W, H = 480, 270
    r, orc = _pair(api, oracle_mod, None, W, H)
    pin_rect, box = r.active_pixels()
    r.set_lens(*lens)
    (x0, w, y0, rows), _ = r.active_pixels()
    share = _rect_share((x0, w, y0, rows), W, H)
    print(f"lens {lens}: rectangle {(x0, w, y0, rows)}, {share:.3f} of the frame (pinhole {_rect_share(pin_rect, W, H):.3f})")
    assert share < 0.5
    assert x0 <= pin_rect[0] and y0 <= pin_rect[2] and x0 + w >= pin_rect[0] + pin_rect[1] and y0 + rows >= pin_rect[2] + pin_rect[3]
    ys, xs = np.mgrid[0:H, 0:W]
    outside = ~((xs >= x0) & (xs < x0 + w) & (ys >= y0) & (ys < y0 + rows))
    near = outside & (xs >= x0 - 6) & (xs < x0 + w + 6) & (ys >= y0 - 6) & (ys < y0 + rows + 6)
    far = np.flatnonzero(outside & ~near)
    rng = np.random.default_rng(11)
    pixels = np.concatenate([np.flatnonzero(near), rng.choice(far, 3000, replace=False)])
    assert len(pixels) > 3000
    mn, mx = box[:3].astype(np.float64), box[3:].astype(np.float64)
    for s in range(4):
        o, d, _ = lens_rays(oracle_mod, orc, W, H, pixels, s, *lens)
        hit = _box_hit64(o.astype(np.float64), d.astype(np.float64), mn, mx)
        assert not hit.any(), (s, pixels[hit][:8])
    # ... while rays from inside it do meet the box
    inner = (ys[~outside] * W + xs[~outside])[:: 37]
    o, d, _ = lens_rays(oracle_mod, orc, W, H, inner, 0, *lens)
    assert _box_hit64(o.astype(np.float64), d.astype(np.float64), mn, mx).any()


def test_lens_arguments_and_state(api, oracle_mod):
    import ctypes as C
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    W, H = 96, 54
    r = api.Renderer(scenes.cornell_box(W, H), W, H)
    pin_rect, _ = r.active_pixels()
    nan, inf = float("nan"), float("inf")
    for bad in [(-1.0, 100.0), (nan, 100.0), (inf, 100.0), (10.0, 0.0), (10.0, -5.0), (10.0, nan), (10.0, inf)]:
        with pytest.raises(api.PtError) as e:
            r.set_lens(*bad)
        assert e.value.code == -1, bad                                       # PT_ERR_ARG
    assert r.primary_ray(5, 0)[2] == 1, "a rejected lens leaves the pinhole"
    r.set_lens(0.0, 0.0); r.set_lens(0.0, -3.0)                              # no lens: the focus is not looked at
    with pytest.raises(api.PtError) as e:
        r.primary_ray(W * H, 0)
    assert e.value.code == -1
    r.set_lens(300.0, 600.0)
    lens_rect, _ = r.active_pixels()
    assert lens_rect != pin_rect and lens_rect[1] * lens_rect[3] > pin_rect[1] * pin_rect[3]
    r.set_lens(40.0, 800.0)
    before = r.primary_ray(1234, 3)
    assert before[2] == 2
    # the lens survives Camera::new and the camera's input
    eye, target = (C.c_float * 3)(10.0, 60.0, 900.0), (C.c_float * 3)(0.0, 50.0, 0.0)
    assert r.L.pt_set_camera(r.ctx, eye, target, 55.0, W / H) == 0
    moved = r.primary_ray(1234, 3)
    assert moved[2] == 2 and not np.array_equal(moved[0], before[0])
    assert r.camera_input(api.EV_KEY_W, 0.0, 0.0, 1e-4)
    assert r.primary_ray(1234, 3)[2] == 2
    # CameraDesc carries the lens: set_camera sets both
    r.set_camera(Camera.new((0.0, 50.0, 1000.0), (0.0, 50.0, 0.0), 60.0, W / H, 120.0, 1100.0))
    assert r.primary_ray(7, 0)[2] == 2
    r.set_camera(scenes.reference_camera(W / H))
    assert r.primary_ray(7, 0)[2] == 1
    assert r.active_pixels()[0] == pin_rect, "aperture 0 after a lens restores the pinhole rectangle"
    # no camera yet: a state error
    r2 = api.Renderer(SceneDesc.new(scenes.cornell_models(), None, "no camera"), W, H)
    r2.set_lens(40.0, 800.0)
    with pytest.raises(api.PtError) as e:
        r2.primary_ray(0, 0)
    assert e.value.code == -3                                                # PT_ERR_STATE
    r2.set_camera(scenes.reference_camera(W / H))                            # (a description without a lens: back to the pinhole)
    assert r2.primary_ray(0, 0)[2] == 1
