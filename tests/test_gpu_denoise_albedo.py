"""GPU (-m gpu): the demodulated denoiser.  pt_post_denoise_albedo and pt_denoise_albedo match the numpy restatement of include/pt_api.h
(denoise_albedo_common.denoise_albedo) bit for bit; pt_accumulate_albedo matches the float32 sum, in sample order, of the albedo guides
pt_render_guides stores; none of the new calls changes what the existing ones return; and on a checker-textured scene the demodulated
result is closer to a many-sample render than pt_denoise's."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from denoise_albedo_common import checker_scene, denoise_albedo, mean_albedo, random_albedo, rmse
from test_denoise_host import MISS, denoise, random_case
from textures_common import varying_scene

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 32, 24
DEPTH = 3
LENS = (0.6, 9.0)
PARAMS = [(1, 0, 0.0, 0.0), (3, 1, 0.0, 3.0), (5, 0, 0.0, 0.0), (8, 64, 1.0, 2.0)]      # levels, sigma_normal, sigma_luminance, sigma_plane


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---------------------------------------------------------------- the post hook
@pytest.mark.parametrize("wh", [(1, 1), (37, 19), (130, 70)])
def test_post_denoise_albedo_matches_the_restatement(api, wh):
    from path_tracer_amd import scenes
    r = api.Renderer(scenes.cornell_box(8, 8), 8, 8, max_bounces=2)
    rng = np.random.default_rng(wh[0] * 1000 + wh[1])
    acc, pos, nrm, model, q = random_case(rng, wh[0], wh[1], n_models=9)
    albedo = random_albedo(rng, wh[1], wh[0])
    ones = np.ones_like(albedo)
    for levels, sn, sl, sx in PARAMS:
        for sumsq in (None, q):
            kw = dict(iterations=levels, sigma_luminance=sl, sigma_normal=sn, sigma_plane=sx)
            what = f"{wh} levels {levels} moments {sumsq is not None}"
            got = r.post_denoise_albedo(acc, pos, nrm, model, albedo, sumsq, **kw)
            assert_bit_equal(got, denoise_albedo(acc, pos, nrm, model, albedo, sumsq, **kw), what)
            assert_bit_equal(r.post_denoise_albedo(acc, pos, nrm, model, ones, sumsq, **kw), r.post_denoise(acc, pos, nrm, model, sumsq, **kw), what + ", albedo 1")
    r.close()


# ---------------------------------------------------------------- the mean albedo
def _guide_sum(r, samples):
    """float32 sum, in sample order, of the albedo guides of `samples`, (1, 1, 1) where that sample's guide is a miss; the per-sample images too"""
    s = None
    per = []
    for k in samples:
        r.render_guides(k)
        al = r.read_guide_albedo()
        miss = r.read_guides()[2] == MISS
        a = np.concatenate([np.where(miss[..., None], F(1), al), np.ones(al.shape[:2] + (1,), F)], -1).astype(F)
        per.append((a, miss, r.read_guides()[2]))
        s = a.copy() if s is None else (s + a).astype(F)
    return s, per


MEAN_CASES = [("plain", 0, {}, False), ("lens", 0, {}, True), ("rank 1 of 2", 0, dict(rank=1, world_size=2), False), ("no LDS scene", 2, {}, False)]


@pytest.mark.parametrize("name,flags,kw,lens", MEAN_CASES)
def test_mean_albedo_is_the_sum_of_the_albedo_guides(api, name, flags, kw, lens):
    desc = varying_scene(W, H)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH, flags=flags, **kw)
    ref = api.Renderer(desc, W, H, max_bounces=DEPTH, flags=flags, **kw)
    if lens:
        r.set_lens(*LENS); ref.set_lens(*LENS)
    want, per = _guide_sum(ref, range(5))
    r.accumulate_albedo(0, 5)
    one = r.read_albedo()
    assert_bit_equal(one, want, f"{name}: accumulate(0, 5)")
    r.reset_albedo()
    r.accumulate_albedo(0, 2)
    r.accumulate_albedo(2, 3)
    assert_bit_equal(r.read_albedo(), want, f"{name}: accumulate(0, 2) then (2, 3)")
    assert (want[..., 3] == 5).all()
    # the scene exercises what the definition distinguishes
    misses = np.stack([m for _, m, _ in per]); models = np.stack([g for _, _, g in per]); imgs = np.stack([a for a, _, _ in per])
    assert misses.any() and (models == 1).any() and (models == 2).any(), "misses and hits on both textured models"
    assert (np.abs(imgs - imgs[0]).max(axis=(0, 3)) > 0).any(), "pixels whose samples differ"
    if kw:
        assert len(r.local_rows()) == H // 2
    r.close(); ref.close()


def test_mean_albedo_goes_stale_with_the_guides_and_restarts_from_zero(api):
    desc = varying_scene(W, H)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH)
    r.accumulate_albedo(0, 3)
    r.render_guides(0)
    r.set_camera(desc.camera)
    for call in (r.read_albedo, lambda: r.denoise_albedo(api.ALBEDO_MEAN)):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == -3
    r.accumulate_albedo(3, 2)                   # onto a stale sum: from zero
    ref = api.Renderer(desc, W, H, max_bounces=DEPTH)
    want, _ = _guide_sum(ref, [3, 4])
    assert_bit_equal(r.read_albedo(), want, "after set_camera")
    r.reset_albedo()
    with pytest.raises(api.PtError):
        r.read_albedo()
    r.accumulate_albedo(4, 1)
    assert_bit_equal(r.read_albedo(), _guide_sum(ref, [4])[0], "after reset_albedo")
    r.close(); ref.close()


def test_new_calls_leave_the_frame_guides_moments_and_pt_denoise_alone(api):
    r = api.Renderer(varying_scene(W, H), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 3)
    r.render_guides(1)

    def state():
        return r.read_frame() + (r.read_moments(),) + r.read_guides() + (r.read_guide_instances(), r.read_guide_albedo())
    before, den = state(), r.denoise()
    r.accumulate_albedo(0, 3)
    r.denoise_albedo(api.ALBEDO_GUIDE)
    r.denoise_albedo(api.ALBEDO_MEAN)
    r.post_denoise_albedo(*[np.ones((4, 4, c), F) for c in (4, 4, 3)], np.zeros((4, 4), np.uint32), np.ones((4, 4, 3), F))
    r.read_albedo()
    for a, b in zip(before, state()):
        assert_bit_equal(a, b, "frame state")
    assert_bit_equal(r.denoise(), den, "pt_denoise after the new calls")
    r.close()


# ---------------------------------------------------------------- the context's own frame
@pytest.mark.parametrize("flags", [0, 32])                      # 32: PT_FLAG_ADAPTIVE (moments)
def test_denoise_albedo_own_frame(api, flags, tmp_path):
    from test_gpu_post import _read_png
    r = api.Renderer(varying_scene(W, H), W, H, max_bounces=DEPTH, flags=flags)
    r.render(0, 4)
    r.render_guides(3)
    r.accumulate_albedo(0, 4)
    plain = r.denoise()
    acc, _, _ = r.read_frame()
    gpos, gnrm, gmodel = r.read_guides()
    q = r.read_moments() if flags else None
    assert_bit_equal(plain, denoise(acc, gpos, gnrm, gmodel, q), "pt_denoise")
    guide = r.read_guide_albedo()
    mean = mean_albedo(r.read_albedo())
    assert (gmodel == MISS).any() and (gmodel == 1).any() and not np.array_equal(guide[gmodel != MISS], mean[gmodel != MISS])
    got = r.denoise_albedo(api.ALBEDO_GUIDE)
    assert_bit_equal(got, denoise_albedo(acc, gpos, gnrm, gmodel, guide, q), "GUIDE")
    got = r.denoise_albedo(api.ALBEDO_MEAN)
    assert_bit_equal(got, denoise_albedo(acc, gpos, gnrm, gmodel, mean, q), "MEAN")
    assert not np.array_equal(got, plain)
    path = tmp_path / "den.png"
    r.write_denoised_image(path)
    assert np.array_equal(_read_png(path), r.post_rgb8(got))
    assert_bit_equal(r.denoise(), plain, "pt_denoise after pt_denoise_albedo")
    r.close()


# ---------------------------------------------------------------- quality
def test_quality_checker_mean_albedo_beats_the_plain_filter(api):
    """A checker-textured floor and wall, 32 x 24, depth 3, 4 spp against a 1024-spp render of the same context; linear RMSE of the mean colour.
    Required: denoise_albedo(MEAN) strictly below pt_denoise (the bar is relative to the plain filter; the four figures are printed for
    profiles/r13_denoise_albedo.md, which does not hold a GPU measurement of them yet)"""
    SPP, REF = 4, 1024
    r = api.Renderer(checker_scene(W, H), W, H, max_bounces=DEPTH)
    racc, _, _ = r.render(0, REF, want_position=False)
    ref = racc[..., :3] / racc[..., 3:4]
    r.reset_accumulation()
    acc, _, _ = r.render(REF, SPP, want_position=False)
    r.render_guides(REF + SPP - 1)
    r.accumulate_albedo(REF, SPP)
    gmodel = r.read_guides()[2]
    assert (gmodel == 1).any() and (gmodel == 2).any()
    raw = rmse(acc[..., :3] / acc[..., 3:4], ref)
    plain = rmse(r.denoise(), ref)
    guide = rmse(r.denoise_albedo(api.ALBEDO_GUIDE), ref)
    mean = rmse(r.denoise_albedo(api.ALBEDO_MEAN), ref)
    print(f"checker scene {SPP} spp vs {REF}: raw {raw:.5f} plain {plain:.5f} GUIDE {guide:.5f} MEAN {mean:.5f}")
    r.close()
    assert mean < plain
