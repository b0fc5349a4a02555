"""GPU (-m gpu): the followed guides (pt_render_guides_followed, pt_accumulate_albedo_followed), bit for bit.  The expected values are the
definition restated over oracle pieces (guides_follow_common.chains: primary_ray, trace_closest per hop, the leaf's material, the follow-on
direction tests/test_guides_follow_host.py holds to the oracle's material_eval), on the mixed Cornell box under the three traversal variants and
on a room built for the chains' cases (guides_follow_common.follow_room), under every camera and on a rank; the mean albedo is the float32
fold of the per-sample albedo guides; pt_denoise on followed guides is its numpy restatement fed those guides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
import guides_follow_common as G
from guides_follow_common import F, H, MISS, W
from test_denoise_host import denoise

pytestmark = pytest.mark.gpu
DEPTH = 3
ALL_HOPS = (0, 1, 2, 8)
SAMPLES = (0, 5)
LENS = (0.5, 14.0)
NO_LDS_SCENE, GENERAL_WALK = 2, 16


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_SCENES, _ORACLES, _RAYS, _EXPECT = {}, {}, {}, {}


def _scene(name):
    if name not in _SCENES:
        from path_tracer_amd import scenes
        _SCENES[name] = scenes.cornell_mixed(W, H) if name == "mixed" else G.follow_room()
    return _SCENES[name]


def _oracle(O, name):
    if name not in _ORACLES:
        _ORACLES[name] = O.Oracle(_scene(name))
    return _ORACLES[name]


def _expect(O, name, sample, max_hops):
    """the restated chains of every pixel of the scene under its own pinhole camera, computed once and left unchanged"""
    key = (name, sample, max_hops)
    if key not in _EXPECT:
        orc = _oracle(O, name)
        if (name, sample) not in _RAYS:
            _RAYS[name, sample] = G.pinhole_rays(orc, W, H, sample)
        _EXPECT[key] = G.chains(orc, _scene(name), *_RAYS[name, sample], max_hops)
    return _EXPECT[key]


def _followed(api, r, sample, max_hops):
    """pt_render_guides_followed itself, also for max_hops = 0 (Renderer.render_guides(follow=0) is the plain call)"""
    prm = api.GuideParams(max_hops)
    r._chk(r.L.pt_render_guides_followed(r.ctx, sample, C.byref(prm)))


def _accumulate(api, r, first, n, max_hops):
    prm = api.GuideParams(max_hops)
    r._chk(r.L.pt_accumulate_albedo_followed(r.ctx, first, n, C.byref(prm)))


def _read(r):
    pos, nrm, model = r.read_guides()
    return dict(position=pos, normal=nrm, model=model, instance=r.read_guide_instances(), albedo=r.read_guide_albedo(), hops=r.read_guide_hops())


def _same_guides(got, want, what):
    for k in ("position", "normal", "albedo"):
        assert_bit_equal(got[k], want[k].reshape(got[k].shape), f"{what}: {k} guide")
    for k in ("model", "instance", "hops"):
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), f"{what}: {k} guide"


# ---- 1. the mixed Cornell box: a glass box and a GGX box (never followed), every traversal variant
@pytest.mark.parametrize("flags", [0, NO_LDS_SCENE, GENERAL_WALK], ids=["lds", "no_lds_scene", "general_walk"])
def test_cornell_mixed_matches_the_restated_chains(api, oracle_mod, flags):
    r = api.Renderer(_scene("mixed"), W, H, max_bounces=DEPTH, flags=flags)
    for sample in SAMPLES:
        for hops in ALL_HOPS:
            _followed(api, r, sample, hops)
            got = _read(r)
            _same_guides(got, _expect(oracle_mod, "mixed", sample, hops), f"flags {flags} sample {sample} max_hops {hops}")
            if hops:
                assert (got["hops"] > 0).any() and (got["model"][got["hops"] > 0] != MISS).any()
        # max_hops = 0 IS pt_render_guides, and its sums pt_accumulate_albedo's
        _followed(api, r, sample, 0)
        zero = _read(r)
        assert not zero["hops"].any()
        r.reset_albedo()
        _accumulate(api, r, sample, 2, 0)
        zsum = r.read_albedo()
        r.render_guides(sample)
        _same_guides(_read(r), zero, f"flags {flags} sample {sample}: max_hops 0 vs pt_render_guides")
        r.reset_albedo()
        r.accumulate_albedo(sample, 2)
        assert_bit_equal(r.read_albedo(), zsum, "max_hops 0 vs pt_accumulate_albedo")
    assert r.stats().lds_scene == (0 if flags == NO_LDS_SCENE else 1)


# ---- 2. the room: every case the chains have
@pytest.mark.parametrize("flags", [0, GENERAL_WALK], ids=["lds", "general_walk"])
def test_room_matches_the_restated_chains_and_shows_every_case(api, oracle_mod, flags):
    r = api.Renderer(_scene("room"), W, H, max_bounces=DEPTH, flags=flags)
    for sample in SAMPLES:
        for hops in ALL_HOPS:
            want = _expect(oracle_mod, "room", sample, hops)
            _followed(api, r, sample, hops)
            got = _read(r)
            _same_guides(got, want, f"room, flags {flags} sample {sample} max_hops {hops}")
            if hops >= 2:
                # counted on what the LIBRARY returned (the guides) and on the restated chains' record of how they got there
                counts, _ = G.case_counts(dict(want, model=got["model"].ravel(), hops=got["hops"].ravel()), hops)
                print(sample, hops, counts)
                assert all(v > 0 for v in counts.values()), counts
                capped = (got["hops"] == hops) & (got["model"] != MISS)
                last = got["model"][capped] & 0x0FFFFFFF
                assert np.isin(last, [G.ROOM_MODELS.index("lower"), G.ROOM_MODELS.index("upper")]).any()   # ... on the last mirror of the wedge
                assert (got["model"][capped] >> 28 == hops).all()


CAMERAS = {"lens": dict(lens=LENS), "panorama": dict(proj=(1, 200.0, 120.0, 0.0)), "ortho": dict(proj=(2, 0.0, 0.0, 24.0)),
           "rank1of2": dict(kw=dict(rank=1, world_size=2))}


@pytest.mark.parametrize("camera", list(CAMERAS))
def test_room_under_every_camera_and_on_a_rank(api, oracle_mod, camera):
    c = CAMERAS[camera]
    sc = _scene("room")
    r = api.Renderer(sc, W, H, max_bounces=DEPTH, **c.get("kw", {}))
    if "lens" in c:
        r.set_lens(*c["lens"])
    if "proj" in c:
        r.set_projection(*c["proj"])
    rows = r.local_rows()
    idx = rows.astype(np.int64)
    orc = _oracle(oracle_mod, "room")
    sample = 5
    _expect(oracle_mod, "room", sample, 0)                               # (the pinhole rays of the sample)
    pin_o, pin_d = (a.reshape(H, W, 3)[idx].reshape(-1, 3) for a in _RAYS["room", sample])
    if camera == "rank1of2":
        assert len(rows) == H // 2
        o, d = pin_o, pin_d
    else:
        o, d = G.library_rays(r, W, rows, sample)
        assert not np.array_equal(d, pin_d) or not np.array_equal(o, pin_o)
    for hops in (0, 2, 8):
        want = G.chains(orc, sc, o, d, hops)
        _followed(api, r, sample, hops)
        got = _read(r)
        _same_guides(got, want, f"{camera}, max_hops {hops}")
        if hops:
            assert (got["hops"] > 1).any() and (got["model"] == MISS).any()
        if camera == "rank1of2":
            # ... which are the rank's rows of the single-rank result
            whole = _expect(oracle_mod, "room", sample, hops)
            _same_guides(got, {k: v.reshape((H, W) + v.shape[1:])[idx] for k, v in whole.items()}, f"rank 1 of 2 vs the whole frame, max_hops {hops}")


# ---- 3. the mean albedo of the chains
def _guide_sum(api, r, samples, hops):
    """float32 sum, in sample order, of the followed albedo guides of `samples`, (1, 1, 1) where that sample's chain ended as a miss"""
    total = np.zeros((H, W, 4), F)
    for k in samples:
        _followed(api, r, k, hops)
        al = r.read_guide_albedo()
        miss = r.read_guides()[2] == MISS
        a = np.where(miss[..., None], F(1.0), al).astype(F)
        total = total + np.concatenate([a, np.ones((H, W, 1), F)], axis=2)
    return total


def test_mean_albedo_is_the_fold_of_the_followed_albedo_guides(api):
    sc = _scene("room")
    ref = api.Renderer(sc, W, H, max_bounces=DEPTH)
    want2, want8 = _guide_sum(api, ref, range(5), 2), _guide_sum(api, ref, range(3), 8)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    _accumulate(api, r, 0, 5, 2)
    whole = r.read_albedo()
    assert_bit_equal(whole, want2, "(0, 5) at max_hops 2")
    r.reset_albedo()
    _accumulate(api, r, 0, 3, 2)
    _accumulate(api, r, 3, 2, 2)
    assert_bit_equal(r.read_albedo(), whole, "(0, 3) then (3, 2)")
    assert not np.array_equal(want2[..., :3], _guide_sum(api, ref, range(5), 0)[..., :3])
    # another max_hops starts from zero, like accumulating onto stale sums; so does the plain call after a followed one
    _accumulate(api, r, 0, 3, 8)
    assert_bit_equal(r.read_albedo(), want8, "a changed max_hops restarts the sums")
    r.accumulate_albedo(0, 5)
    assert_bit_equal(r.read_albedo(), _guide_sum(api, ref, range(5), 0), "pt_accumulate_albedo after followed sums restarts them")
    # the demodulated filter wants guides and sums of the same chains
    r.render(0, 2)
    r.render_guides(1, follow=2)
    with pytest.raises(api.PtError) as e:
        r.denoise_albedo(api.ALBEDO_MEAN)
    assert e.value.code == -3 and "max_hops" in str(e.value)
    r.denoise_albedo(api.ALBEDO_GUIDE)
    _accumulate(api, r, 0, 2, 2)
    from denoise_albedo_common import denoise_albedo, mean_albedo
    acc = r.read_frame()[0]
    gpos, gnrm, gmodel = r.read_guides()
    assert_bit_equal(r.denoise_albedo(api.ALBEDO_MEAN), denoise_albedo(acc, gpos, gnrm, gmodel, mean_albedo(r.read_albedo()), None), "MEAN on followed guides")
    r.render_guides(1)
    with pytest.raises(api.PtError) as e:
        r.denoise_albedo(api.ALBEDO_MEAN)
    assert e.value.code == -3


# ---- 4. the filter takes the followed guides as they are
def test_denoise_on_followed_guides_is_the_restatement(api):
    r = api.Renderer(_scene("room"), W, H, max_bounces=DEPTH)
    r.render(0, 4)
    r.render_guides(3, follow=2)
    gpos, gnrm, gmodel = r.read_guides()
    assert (gmodel[gmodel != MISS] >> 28).max() == 2
    acc = r.read_frame()[0]
    followed = r.denoise()
    assert_bit_equal(followed, denoise(acc, gpos, gnrm, gmodel, None), "pt_denoise on followed guides")
    r.render_guides(3)
    assert not np.array_equal(r.denoise(), followed)


def test_followed_guides_leave_the_frame_alone_and_frame_moving_writes_first_hits(api):
    r = api.Renderer(_scene("room"), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 3)
    before = r.read_frame() + (r.read_moments(),)
    r.render_guides(11, follow=8)
    r.accumulate_albedo(0, 2, follow=8)
    for a, b in zip(before, r.read_frame() + (r.read_moments(),)):
        assert_bit_equal(a, b, "frame state")
    # a refused call leaves the guides and the sums as they are
    kept, sums = _read(r), r.read_albedo()
    assert r.L.pt_render_guides_followed(r.ctx, 0, C.byref(api.GuideParams(9))) == -1
    assert r.L.pt_accumulate_albedo_followed(r.ctx, 0, 1, C.byref(api.GuideParams(2, (0, 0, 1)))) == -1
    assert r.L.pt_accumulate_albedo_followed(r.ctx, 0, 0, C.byref(api.GuideParams(8))) == -1
    _same_guides(_read(r), kept, "after refused calls")
    assert_bit_equal(r.read_albedo(), sums, "sums after refused calls")
    assert kept["hops"].max() == 8
    m = api.Renderer(_scene("room"), W, H, max_bounces=DEPTH)
    m.render_guides(0, follow=2)
    m.frame_moving(0)
    moved = _read(m)
    assert not moved["hops"].any()
    m.render_guides(0)
    _same_guides(moved, _read(m), "pt_frame_moving's guides are first-hit guides")
    m.render_guides(0, follow=2)
    assert _read(m)["hops"].any()


def test_unit_hook_on_the_device_is_the_host_evaluation(api):
    from test_guides_follow_host import _kinds_scene, _pairs
    sc, mats = _kinds_scene()
    r = api.Renderer(sc, 8, 8, max_bounces=2)
    inc, nrm = _pairs(np.random.default_rng(3), 333, grazing=40)         # more than one block, not a multiple of it
    front = (np.arange(333) % 2).astype(np.uint8)
    for mi in range(len(mats)):
        assert_bit_equal(r.guide_follow_dir(mi, inc, nrm, front, on_device=True), r.guide_follow_dir(mi, inc, nrm, front), f"material {mi}")


def test_headless_follow_matches_the_python_route(api, tmp_path):
    from test_gpu_post import _read_png
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Dielectric, Model, SceneDesc, Specular
    Wd, Hd, FRAMES, BOUNCES = 48, 32, 4, 4
    exe = B.build_host_driver()
    den_png, dal_png = tmp_path / "den.png", tmp_path / "dal.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", str(FRAMES), "--bounces", str(BOUNCES), "--mirror-glass", "--follow", "2",
                          "--denoise", str(den_png), "--denoise-albedo", str(dal_png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    mats = {"cb_box_tall": Specular.new((1.0, 1.0, 1.0)), "cb_box_short": Dielectric.new((0.95, 0.95, 0.95), 1.5, None)}
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), mats.get(m.name, m.material)) for m in scenes.cornell_models()],
                       scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    last = r.inv_projection()
    for k in range(FRAMES):
        r.frame(k, last, download=False)
        last = r.inv_projection()
    r.render_guides(FRAMES - 1, follow=2)
    assert (r.read_guide_hops() == 2).any() and (r.read_guide_hops() == 1).any()
    followed = r.post_rgb8(r.denoise())
    assert np.array_equal(_read_png(den_png), followed)
    r.accumulate_albedo(0, FRAMES, follow=2)
    assert np.array_equal(_read_png(dal_png), r.post_rgb8(r.denoise_albedo(api.ALBEDO_MEAN)))
    r.render_guides(FRAMES - 1)
    assert not np.array_equal(r.post_rgb8(r.denoise()), followed)


# ---- 5. what it is for
def test_quality_in_the_mirror_improves(api):
    """The room's mirror shows the boundary between the two differently coloured walls behind the camera.  4 spp through pt_denoise, RMSE
    against 4096 spp of the same context over the pixels with hops > 0: followed guides (max_hops = 2) against first-hit guides.  Both arms
    are deterministic.  Measured on an MI355X: see profiles/r16_followed_guides.md."""
    REF, SPP = 4096, 4
    r = api.Renderer(_scene("room"), W, H, max_bounces=DEPTH)
    racc = r.render(0, REF, want_position=False)[0]
    ref = racc[..., :3] / racc[..., 3:4]
    r.reset_accumulation()
    acc = r.render(REF, SPP, want_position=False)[0]
    r.render_guides(REF + SPP - 1, follow=2)
    sel = r.read_guide_hops() > 0
    followed = r.denoise()
    r.render_guides(REF + SPP - 1)
    first = r.denoise()

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3][sel].astype(np.float64) - ref[sel].astype(np.float64)) ** 2)))
    noisy = rmse(acc[..., :3] / acc[..., 3:4])
    e_first, e_followed = rmse(first), rmse(followed)
    print(f"followed-guide quality, {int(sel.sum())} pixels with hops > 0: noisy {noisy:.5f} first-hit guides {e_first:.5f} max_hops 2 guides {e_followed:.5f}")
    assert sel.sum() > 100
    assert e_followed < e_first
