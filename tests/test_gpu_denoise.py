"""GPU (-m gpu): the denoiser.  The first-hit guides match the CPU oracle (primary_ray -> integrate for position, trace_closest for the
normal and hit leaf, tlas_dump for the leaf's model) and the render's own position / id bit for bit; the filter matches the numpy
restatement of include/pt_api.h (test_denoise_host.denoise) bit for bit, on caller images and on the context's own frames; and because the
output is exact, the quality bars below are deterministic."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from test_denoise_host import MISS, denoise, random_case

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 32, 24
DEPTH = 3


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _scene(name, w=W, h=H):
    from path_tracer_amd import scenes
    return {"cornell": scenes.cornell_box, "mixed": scenes.cornell_mixed, "instanced": scenes.cornell_instanced,
            "media": scenes.cornell_media}[name](w, h)


def _oracle_guides(o, rows, sample):
    """(position xyzt, normal xyz, model) of the camera ray of `sample` of every pixel of the given global rows, from the oracle"""
    leaf_blas = {}
    td = o.tlas_dump(0)
    for k, a, b in zip(td["kind"], td["a"], td["b"]):
        if k == 1:
            leaf_blas[int(a)] = int(b)
    os_, ds, pix = [], [], []
    for gy in rows:
        for x in range(W):
            p = int(gy) * W + x
            ro, rd = o.primary_ray(W, H, p, sample)
            os_.append(ro); ds.append(rd); pix.append(p)
    os_, ds = np.array(os_, F), np.array(ds, F)
    tc = o.trace_closest(os_, ds)
    pos = np.zeros((len(pix), 4), F)
    for i, p in enumerate(pix):
        _, pp, _ = o.integrate(os_[i], ds[i], p, sample, max_bounces=DEPTH)
        pos[i] = pp
    hit = tc["inst"] != MISS
    model = np.full(len(pix), MISS, np.uint32)
    model[hit] = [leaf_blas[int(i)] for i in tc["inst"][hit]]
    nrm = np.where(hit[:, None], tc["normal"], F(0)).astype(F)
    n = len(rows)
    return pos.reshape(n, W, 4), nrm.reshape(n, W, 3), model.reshape(n, W)


GUIDE_CASES = [("cornell", 0, {}, 7), ("cornell", 0, {}, 0), ("cornell", 0, {}, 300), ("cornell", 2, {}, 7),          # 2: PT_FLAG_NO_LDS_SCENE
               ("instanced", 0, {}, 7), ("instanced", 16, {}, 7), ("mixed", 0, {"env": True}, 7), ("media", 0, {}, 300),  # 16: GENERAL_WALK
               ("cornell", 0, {"rank": 1}, 7)]


@pytest.mark.parametrize("name,flags,extra,sample", GUIDE_CASES)
def test_guides_match_the_oracle(api, oracle_mod, name, flags, extra, sample):
    sc = _scene(name)
    kw = dict(rank=1, world_size=2) if extra.get("rank") else {}
    r = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=flags, **kw)
    o = oracle_mod.Oracle(sc)
    if extra.get("env"):
        env = (np.random.default_rng(3).uniform(0, 1, (9, 17, 3)) ** 2).astype(F)
        r.set_environment(env); o.set_environment(env)
    r.render_guides(sample)
    pos, nrm, model = r.read_guides()
    rows = r.local_rows()
    opos, onrm, omodel = _oracle_guides(o, rows, sample)
    assert_bit_equal(pos, opos, "position guide")
    assert_bit_equal(nrm, onrm, "normal guide")
    assert np.array_equal(model, omodel)
    assert (model != MISS).any()
    if extra.get("rank"):
        assert len(rows) == H // 2


@pytest.mark.parametrize("sample", [0, 5])
def test_guides_match_the_render_and_the_frame(api, sample):
    sc = _scene("mixed")
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    _, pos, idb = r.render(0, sample + 1)
    r.render_guides(sample)
    gpos, _, gmodel = r.read_guides()
    assert_bit_equal(gpos, pos, "guide vs render position")
    assert np.array_equal(gmodel & 0xFF, idb & 0xFFFF)
    r2 = api.Renderer(sc, W, H, max_bounces=DEPTH)
    for k in range(sample + 1):
        _, fpos, fid = r2.frame(k)
    r2.render_guides(sample)
    gpos2, _, gmodel2 = r2.read_guides()
    assert_bit_equal(gpos2, fpos, "guide vs frame position")
    assert np.array_equal(gmodel2 & 0xFF, fid & 0xFFFF)


def test_guides_and_denoise_leave_the_frame_alone(api):
    r = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 3)
    before = r.read_frame() + (r.read_moments(),)
    r.render_guides(11)
    r.denoise()
    after = r.read_frame() + (r.read_moments(),)
    for a, b in zip(before, after):
        assert_bit_equal(a, b, "frame state")


@pytest.mark.parametrize("wh", [(1, 1), (37, 19), (64, 64), (130, 70)])
def test_post_denoise_matches_the_restatement(api, wh):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    rng = np.random.default_rng(wh[0] * 1000 + wh[1])
    acc, pos, nrm, model, q = random_case(rng, wh[0], wh[1], n_models=9)
    for levels, sn, sl, sx in [(1, 0, 0.0, 0.0), (2, 16, 2.0, 0.5), (3, 1, 0.0, 3.0), (4, 256, 8.0, 0.0), (5, 0, 0.0, 0.0), (8, 64, 1.0, 2.0)]:
        for sumsq in (None, q):
            kw = dict(iterations=levels, sigma_luminance=sl, sigma_normal=sn, sigma_plane=sx)
            got = r.post_denoise(acc, pos, nrm, model, sumsq, **kw)
            assert_bit_equal(got, denoise(acc, pos, nrm, model, sumsq, **kw), f"{wh} levels {levels} moments {sumsq is not None}")


def test_post_denoise_keeps_models_apart(api):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    acc, pos, nrm, model, q = random_case(np.random.default_rng(9), 64, 48, n_models=5)
    base = r.post_denoise(acc, pos, nrm, model)
    sel = model == 3
    acc2 = acc.copy(); acc2[sel, :3] *= F(7)
    out = r.post_denoise(acc2, pos, nrm, model)
    assert np.array_equal(out[~sel].view(np.uint32), base[~sel].view(np.uint32)) and not np.array_equal(out[sel], base[sel])


def _restated(r, moments):
    acc, _, _ = r.read_frame()
    gpos, gnrm, gmodel = r.read_guides()
    return denoise(acc, gpos, gnrm, gmodel, r.read_moments() if moments else None)


def test_denoise_own_frame_spatial_variance(api):
    r = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH)
    r.render(0, 4)
    r.render_guides(3)
    assert_bit_equal(r.denoise(), _restated(r, False), "cornell 4 spp, spatial variance")


def test_denoise_own_frame_moments_after_adaptive_rounds(api):
    r = api.Renderer(_scene("mixed"), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 4)
    r.render_adaptive(4, 0.05)
    r.render_adaptive(4, 0.05)
    r.render_guides(0)
    assert_bit_equal(r.denoise(), _restated(r, True), "adaptive frame, moments")


def test_denoise_after_frames_with_a_moving_camera(api):
    r = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    last = r.inv_projection()
    ident = np.zeros((H, W), np.uint32)
    for k in range(6):
        if k >= 3:
            r.camera_input(api.EV_KEY_W, 0.0, 0.0, 2.0e-6)
            r.camera_input(api.EV_MOUSE_MOTION, 1.0, 0.25, 1.0e-6)
        _, fpos, ident = r.frame(k, last, ident)
        last = r.inv_projection()
    r.render_guides(5)
    gpos, _, _ = r.read_guides()
    assert_bit_equal(gpos, fpos, "guides of the last frame")
    # pt_frame invalidated the moments: the spatial variance is used although the context keeps moments
    assert_bit_equal(r.denoise(iterations=4), denoise(r.read_frame()[0], *r.read_guides(), None, iterations=4), "after pt_frame")


def _rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))


_REFS = {}


def _quality(api, name, spp, flags=0, n_ref=4096, size=256):
    """display-space RMSE (the library's GT tonemap, what pt_present shows) of the noisy and the denoised frame against an n_ref-spp
    render; the noisy frame's samples come after the reference's.  Linear RMSE is dominated by the light's partially covered edge pixels
    (radiance 15 against ~0.1), whose single-sample guide files them under the ceiling: profiles/r07_denoise.md has both."""
    sc = _scene(name, size, size)
    if name not in _REFS:
        ref = api.Renderer(sc, size, size, max_bounces=DEPTH)
        racc, _, _ = ref.render(0, n_ref, want_position=False)
        _REFS[name] = ref.post_tonemap(racc)
        ref.close()
    r = api.Renderer(sc, size, size, max_bounces=DEPTH, flags=flags)
    acc, _, _ = r.render(n_ref, spp, want_position=False)
    r.render_guides(n_ref + spp - 1)
    den = r.denoise()
    noisy, out = _rmse(r.post_tonemap(acc), _REFS[name]), _rmse(r.post_tonemap(den), _REFS[name])
    print(f"display quality {name} {spp} spp flags {flags}: noisy {noisy:.5f} denoised {out:.5f} ratio {out / noisy:.3f}")
    return noisy, out


def test_quality_cornell_4spp(api):
    noisy, den = _quality(api, "cornell", 4)
    assert den <= 0.7 * noisy                       # measured 0.648


def test_quality_mixed_4spp_improves(api):
    noisy, den = _quality(api, "mixed", 4)
    assert den < 0.9 * noisy                        # measured 0.852


def test_quality_cornell_16spp_with_moments_improves(api):
    noisy, den = _quality(api, "cornell", 16, flags=32)
    assert den < 0.9 * noisy                        # measured 0.861


def test_write_denoised_image_is_the_rgb8_of_the_result(api, tmp_path):
    from test_gpu_post import _read_png
    r = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH)
    r.render(0, 4)
    r.render_guides(3)
    den = r.denoise()
    path = tmp_path / "den.png"
    r.write_denoised_image(path)
    assert np.array_equal(_read_png(path), r.post_rgb8(den))


def test_headless_denoise_matches_the_python_route(api, tmp_path):
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, FRAMES, BOUNCES = 96, 64, 6, 4
    exe = B.build_host_driver()
    out_png, den_png = tmp_path / "headless.png", tmp_path / "headless_den.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", str(FRAMES), "--bounces", str(BOUNCES), "--move", "--out", str(out_png),
                          "--denoise", str(den_png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    last = r.inv_projection()
    for k in range(FRAMES):
        if k >= FRAMES // 2:
            r.camera_input(api.EV_KEY_W, 0.0, 0.0, 2.0e-6)
            r.camera_input(api.EV_MOUSE_MOTION, 1.0, 0.25, 1.0e-6)
        r.frame(k, last, download=False)
        last = r.inv_projection()
    r.render_guides(FRAMES - 1)
    den = r.denoise()
    assert np.array_equal(_read_png(den_png), r.post_rgb8(den))
    assert np.array_equal(_read_png(out_png), r.present_rgb8())


def test_device_path_state_errors(api):
    r = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH)
    r.render(0, 2)
    r.render_guides(1)
    r.denoise()
    r.camera_input(api.EV_KEY_W, 0.0, 0.0, 1e-6)
    with pytest.raises(api.PtError) as e:
        r.denoise()
    assert e.value.code == -3 and "stale" in str(e.value)
    r.render_guides(1)
    r.denoise()
    rk = api.Renderer(_scene("cornell"), W, H, max_bounces=DEPTH, rank=0, world_size=2)
    rk.render(0, 2)
    rk.render_guides(1)
    assert rk.read_guides()[0].shape[0] == H // 2
    with pytest.raises(api.PtError) as e:
        rk.denoise()
    assert e.value.code == -3
