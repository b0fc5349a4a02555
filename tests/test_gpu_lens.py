"""GPU: thin-lens depth of field (pt_set_lens), bit for bit.  The expected values are the definition's camera rays in numpy
(test_lens_host.lens_rays) walked by the oracle's integrator from that ray with two stream draws spent (pto_integrate)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from test_lens_host import lens_rays

pytestmark = pytest.mark.gpu

W, H, DEPTH = 48, 32, 6
LENS = (40.0, 800.0)
ENV_SEED = 21


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _scene(name, w=W, h=H):
    from path_tracer_amd import scenes
    return {"cornell": lambda: scenes.cornell_box(w, h), "cornell_mixed": lambda: scenes.cornell_mixed(w, h),
            "media": lambda: scenes.cornell_media(w, h, level=2), "cornell_instanced": lambda: scenes.cornell_instanced(w, h),
            "cornell_env": lambda: scenes.cornell_box(w, h)}[name]()


def _env():
    return (np.random.default_rng(ENV_SEED).uniform(0, 1, (17, 33, 3)) ** 3 * 4).astype(np.float32)


class Expect:
    """per-sample radiance, first-hit position and id byte of every pixel of a scene under a lens, from the oracle; cached by sample"""

    def __init__(self, O, name, lens=LENS, w=W, h=H, depth=DEPTH, scene=None):
        self.O, self.lens, self.w, self.h, self.depth = O, lens, w, h, depth
        self.orc = O.Oracle(scene if scene is not None else _scene(name, w, h))
        if name == "cornell_env":
            self.orc.set_environment(_env())
        self.cache = {}

    def sample(self, s):
        if s not in self.cache:
            w, h = self.w, self.h
            o, d, draws = lens_rays(self.O, self.orc, w, h, np.arange(w * h), s, *self.lens)
            col = np.zeros((h * w, 4), np.float32); pos = np.zeros((h * w, 4), np.float32); idb = np.zeros(h * w, np.uint32)
            for p in range(w * h):
                col[p], pos[p], idb[p] = self.orc.integrate(o[p], d[p], p, s, draws, max_bounces=self.depth)
            self.cache[s] = (col.reshape(h, w, 4), pos.reshape(h, w, 4), idb.reshape(h, w))
        return self.cache[s]

    def samples(self, first, n):
        return np.stack([self.sample(s)[0] for s in range(first, first + n)])

    def frame(self, n, first=0):
        """pt_render(first, n) from a cleared frame: the f32 fold in sample order, the last sample's position, the id history"""
        acc = np.zeros((self.h, self.w, 4), np.float32)
        idv = np.zeros((self.h, self.w), np.uint32)
        for s in range(first, first + n):
            col, pos, idb = self.sample(s)
            acc = acc + col
            idv = (idv << np.uint32(16)) | idb
        return acc, pos, idv


_EXPECT = {}


def _expect(O, name, **kw):
    key = (name, tuple(sorted((k, v) for k, v in kw.items() if k != "scene")))
    if key not in _EXPECT:
        _EXPECT[key] = Expect(O, name, **kw)
    return _EXPECT[key]


def _renderer(api, name, flags=0, lens=LENS, **kw):
    r = api.Renderer(_scene(name), W, H, max_bounces=DEPTH, flags=flags, **kw)
    if name == "cornell_env":
        r.set_environment(_env())
    r.set_lens(*lens)
    return r


def _same_frame(got, want, what):
    assert_bit_equal(got[0], want[0], what + ": accumulation")
    assert_bit_equal(got[1], want[1], what + ": position")
    assert np.array_equal(got[2], want[2]), what + ": id history"


@pytest.mark.parametrize("name,flags", [("cornell", 0), ("cornell", 2), ("cornell", 16), ("cornell_mixed", 0), ("cornell_mixed", 2), ("media", 0), ("media", 2),
                                        ("cornell_instanced", 0), ("cornell_instanced", 2), ("cornell_env", 0), ("cornell_env", 2)])
def test_per_sample_radiance(api, oracle_mod, name, flags):
    """every pixel, samples 0..3 and 508..511 (n_sobol 512): BVH in LDS, in global memory (FLAG_NO_LDS_SCENE = 2), the general walk (16)"""
    ex = _expect(oracle_mod, name)
    r = _renderer(api, name, flags)
    for first in (0, 508):
        got = r.render_samples(first, 4)
        want = ex.samples(first, 4)
        assert got.shape == want.shape
        assert_bit_equal(got, want, f"{name} flags {flags} samples {first}..{first + 3}")


@pytest.mark.parametrize("name", ["cornell", "cornell_mixed", "cornell_env"])
@pytest.mark.parametrize("n", [5, 33])
def test_frame_contract(api, oracle_mod, name, n):
    """pt_render(0, n): the accumulation is the f32 fold of the samples in order, the position the last sample's, the id history shifted in
    once per sample; batch_spp 16, so that n = 33 crosses batches, both pipelines and the path-id block"""
    ex = _expect(oracle_mod, name)
    r = _renderer(api, name, batch_spp=16)
    _same_frame(r.render(0, n), ex.frame(n), f"{name}, {n} samples")


def test_primary_cull_changes_nothing(api, oracle_mod):
    ex = _expect(oracle_mod, "cornell", w=96, h=54)
    sc = _scene("cornell", 96, 54)
    frames = []
    for flags in (0, api.FLAG_NO_PRIMARY_CULL):
        r = api.Renderer(sc, 96, 54, max_bounces=DEPTH, flags=flags)
        r.set_lens(*LENS)
        rect, _ = r.active_pixels()
        if flags:
            assert rect == (0, 96, 0, 54)
        else:
            assert rect[1] * rect[3] < 96 * 54 and (rect[1] < 96 or rect[3] < 54), rect
        frames.append(r.render(0, 3))
    _same_frame(frames[0], frames[1], "with and without the primary cull")
    _same_frame(frames[0], ex.frame(3), "culled frame vs oracle")


def test_frame_and_guides(api, oracle_mod):
    """pt_frame(k) is sample k: data, position, id.  pt_render_guides(k) afterwards gives the same position and id byte."""
    ex = _expect(oracle_mod, "cornell_mixed")
    r = _renderer(api, "cornell_mixed")
    ident = np.zeros((H, W), np.uint32)
    want_id = np.zeros((H, W), np.uint32)
    for k in (0, 1, 7):
        data, pos, ident = r.frame(k, None, ident)
        col, opos, oid = ex.sample(k)
        want_id = (want_id << np.uint32(16)) | oid
        assert_bit_equal(data, col, f"frame {k} data")
        assert_bit_equal(pos, opos, f"frame {k} position")
        assert np.array_equal(ident, want_id), f"frame {k} id"
        r.render_guides(k)
        gpos, _, gmodel = r.read_guides()
        assert_bit_equal(gpos, opos, f"guides of sample {k}: position")
        assert np.array_equal(gmodel & 0xff, oid), f"guides of sample {k}: id byte"
    # a lens change makes the guides stale, like a camera change
    r.set_lens(120.0, 1100.0)
    with pytest.raises(api.PtError) as e:
        r.denoise(iterations=1)
    assert e.value.code == -3


def test_adaptive_rounds(api, oracle_mod):
    ex = _expect(oracle_mod, "cornell")
    r = _renderer(api, "cornell", flags=api.FLAG_ADAPTIVE)
    M = 4
    # a threshold the active set crosses gradually: the median relative error of the noisy pixels after M samples
    first = ex.samples(0, M)
    lum = 0.2126 * first[..., 0] + 0.7152 * first[..., 1] + 0.0722 * first[..., 2]
    mean, var = lum.mean(0), lum.var(0)
    rel = np.sqrt(var / M) / np.maximum(mean, 1e-3)
    threshold = float(np.quantile(rel[rel > 0], 0.5))
    for _ in range(3):
        r.render_adaptive(M, threshold, 0.0, M, 0)
    acc, pos, idb = r.read_frame()
    counts = np.rint(acc[..., 3]).astype(np.int64)
    assert set(np.unique(counts)) <= {M, 2 * M, 3 * M} and len(np.unique(counts)) > 1, np.unique(counts)
    for n in np.unique(counts):
        sel = counts == n
        oacc, opos, oid = ex.frame(int(n))
        assert_bit_equal(acc[sel], oacc[sel], f"accumulation of the {int(sel.sum())} pixels with {n} samples")
        assert_bit_equal(pos[sel], opos[sel], f"position of the pixels with {n} samples")
        assert np.array_equal(idb[sel], oid[sel]), f"id history of the pixels with {n} samples"


def test_ranks_and_multi(api, oracle_mod):
    from path_tracer_amd.dist import rows_of_rank
    ex = _expect(oracle_mod, "cornell_mixed")
    want = ex.frame(5)
    full = [np.zeros_like(w) for w in want]
    for rank in range(2):
        rr = _renderer(api, "cornell_mixed", rank=rank, world_size=2, strip_rows=4)
        got = rr.render(0, 5)
        for f, g in zip(full, got):
            f[rows_of_rank(H, rank, 2, 4)] = g
    _same_frame(full, want, "two ranks")
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    sc = _scene("cornell_mixed")
    cam = sc.camera
    sc = SceneDesc.new(sc.models, Camera.new(cam.origin, cam.target, cam.fov, cam.aspect_ratio, *LENS), sc.name)
    m = api.MultiRenderer(sc, W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    got = m.render(0, 5)
    m.close()
    assert_bit_equal(got, want[0], "pt_multi over a duplicated device")


def test_pinhole_is_untouched_by_a_lens_that_came_and_went(api, oracle_mod):
    sc = _scene("cornell_mixed")
    fresh = api.Renderer(sc, W, H, max_bounces=DEPTH).render(0, 5)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    r.set_lens(*LENS)
    lensed = r.render(0, 5)
    assert not np.array_equal(lensed[0], fresh[0])
    r.set_lens(0.0, 0.0)
    r.reset_accumulation()
    again = r.render(0, 5, ident=np.zeros((H, W), np.uint32))
    _same_frame(again, fresh, "pinhole after a lens")
    _same_frame(fresh, oracle_mod.Oracle(sc).render(W, H, 5, max_bounces=DEPTH)[:3], "pinhole vs oracle")


def test_headless_with_a_lens(api, oracle_mod, tmp_path):
    """examples/headless --aperture 40 --focus 800: the C++ surface (ptmi::Camera::New's two arguments) down to the PNG"""
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    from test_gpu_post import _read_png
    Wd, Hd, FRAMES, BOUNCES = 96, 64, 4, 4
    exe = B.build_host_driver()
    out_png = tmp_path / "lens.png"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", str(FRAMES), "--bounces", str(BOUNCES), "--aperture", "40", "--focus", "800",
                          "--out", str(out_png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    ex = Expect(oracle_mod, "cornell", w=Wd, h=Hd, depth=BOUNCES, scene=sc)
    acc = np.zeros((Hd, Wd, 4), np.float32)
    for k in range(FRAMES):
        acc = oracle_mod.post_accumulate(ex.sample(k)[0], acc)       # a camera at rest: State::update accumulates
    assert np.array_equal(_read_png(out_png), oracle_mod.post_rgb8(acc))
