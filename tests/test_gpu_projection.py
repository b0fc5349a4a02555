"""GPU: panoramic and orthographic cameras (pt_set_projection), bit for bit.  The expected values are the definition's camera rays in numpy
(projection_common.projection_rays, which test_projection_host.py holds pt_primary_ray to) walked by the oracle's integrator from that ray with one
stream draw spent (pto_integrate), as test_gpu_lens.py checks the lens."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from projection_common import ORTHOGRAPHIC, PANORAMA, projection_rays
from test_denoise_host import MISS, denoise

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH = 32, 24, 4
ENV_SEED = 21
INSIDE = ((0.0, 50.0, 100.0), (0.0, 50.0, 0.0))        # a camera inside the room: a full panorama's rays leave in every direction
# name -> (pt_projection fields, eye and target or None = the reference's camera)
PROJECTIONS = {"panorama": ((PANORAMA, 360.0, 180.0, 0.0), INSIDE), "ortho": ((ORTHOGRAPHIC, 0.0, 0.0, 600.0), None)}


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _env():
    return (np.random.default_rng(ENV_SEED).uniform(0, 1, (17, 33, 3)) ** 3 * 4).astype(F)


def _scene(name, proj, w=W, h=H, models=None):
    """the scene under the projection's camera pose"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    sc = {"cornell": scenes.cornell_box, "mixed_env": scenes.cornell_mixed, "instanced": scenes.cornell_instanced}[name](w, h)
    pose = PROJECTIONS[proj][1]
    cam = sc.camera if pose is None else Camera.new(pose[0], pose[1], 60.0, w / h)
    return SceneDesc.new(models if models is not None else sc.models, cam, sc.name)


class Expect:
    """per-sample radiance, first-hit position and id byte of every pixel of a scene under a projection, from the oracle; cached by sample"""

    def __init__(self, O, name, proj, w=W, h=H, depth=DEPTH, models=None, scene=None, params=None):
        """scene: a description of the caller's own, under ITS camera pose, in place of the named scene under the projection's pose;
        params: pt_projection fields of the caller's own in place of PROJECTIONS[proj]'s"""
        self.params = params if params is not None else PROJECTIONS[proj][0]
        self.O, self.proj, self.w, self.h, self.depth = O, proj, w, h, depth
        self.scene = scene if scene is not None else _scene(name, proj, w, h, models)
        self.orc = O.Oracle(self.scene)
        if name == "mixed_env":
            self.orc.set_environment(_env())
        self.cache = {}

    def rays(self, s, pixels=None):
        kind, sx, sy, oh = self.params
        pixels = np.arange(self.w * self.h) if pixels is None else pixels
        return projection_rays(self.O, self.orc, self.w, self.h, pixels, s, kind, sx, sy, oh, aspect=self.w / self.h)

    def sample(self, s):
        if s not in self.cache:
            w, h = self.w, self.h
            o, d, draws = self.rays(s)
            col = np.zeros((h * w, 4), F); pos = np.zeros((h * w, 4), F); idb = np.zeros(h * w, np.uint32)
            for p in range(w * h):
                col[p], pos[p], idb[p] = self.orc.integrate(o[p], d[p], p, s, draws, max_bounces=self.depth)
            self.cache[s] = (col.reshape(h, w, 4), pos.reshape(h, w, 4), idb.reshape(h, w))
        return self.cache[s]

    def frame(self, n, first=0):
        """pt_render(first, n) from a cleared frame: the f32 fold in sample order, the last sample's position, the id history"""
        acc = np.zeros((self.h, self.w, 4), F)
        idv = np.zeros((self.h, self.w), np.uint32)
        for s in range(first, first + n):
            col, pos, idb = self.sample(s)
            acc = acc + col
            idv = (idv << np.uint32(16)) | idb
        return acc, pos, idv

    def guides(self, s, rows):
        """(position xyzt, normal xyz, model, world-TLAS leaf) of the camera rays of sample s of the given global rows: position through integrate,
        normal and leaf through trace_closest, the leaf's model through tlas_dump"""
        leaf_blas = {}
        td = self.orc.tlas_dump(0)
        for k, a, b in zip(td["kind"], td["a"], td["b"]):
            if k == 1:
                leaf_blas[int(a)] = int(b)
        pixels = np.concatenate([np.arange(self.w) + int(gy) * self.w for gy in rows])
        o, d, _ = self.rays(s, pixels)
        tc = self.orc.trace_closest(o, d)
        hit = tc["inst"] != MISS
        model = np.full(len(pixels), MISS, np.uint32)
        model[hit] = [leaf_blas[int(i)] for i in tc["inst"][hit]]
        nrm = np.where(hit[:, None], tc["normal"], F(0)).astype(F)
        pos = self.sample(s)[1][np.asarray(rows, np.int64)]
        n = len(rows)
        return pos, nrm.reshape(n, self.w, 3), model.reshape(n, self.w), np.where(hit, tc["inst"], MISS).astype(np.uint32).reshape(n, self.w)


_EXPECT = {}


def _expect(O, name, proj, **kw):
    key = (name, proj, tuple(sorted(kw.items())))
    if key not in _EXPECT:
        _EXPECT[key] = Expect(O, name, proj, **kw)
    return _EXPECT[key]


def _renderer(api, name, proj, flags=0, **kw):
    r = api.Renderer(_scene(name, proj), W, H, max_bounces=DEPTH, flags=flags, **kw)
    if name == "mixed_env":
        r.set_environment(_env())
    r.set_projection(*PROJECTIONS[proj][0])
    return r


def _same_frame(got, want, what):
    assert_bit_equal(got[0], want[0], what + ": accumulation")
    assert_bit_equal(got[1], want[1], what + ": position")
    assert np.array_equal(got[2], want[2]), what + ": id history"


def _assert_hits_and_misses(ex, proj, name, samples):
    """the frames exercise what they are meant to: a panorama inside the Cornell box sees every model and leaves through the open front; the
    orthographic frame is wider than the room"""
    ids = np.concatenate([ex.sample(s)[2].ravel() for s in samples])
    models = set(int(i) for i in np.unique(ids)) - {255}
    assert 255 in ids, "no camera ray leaves the scene"
    if proj == "panorama" and name != "instanced":
        assert len(models) >= 5, models
    else:
        assert len(models) >= 2, models


CASES = [("cornell", 0), ("cornell", 2), ("cornell", 16), ("mixed_env", 0), ("mixed_env", 2), ("instanced", 0), ("instanced", 16)]


@pytest.mark.parametrize("proj", list(PROJECTIONS))
@pytest.mark.parametrize("name,flags", CASES)
def test_per_sample_parity(api, oracle_mod, proj, name, flags):
    """every pixel, samples 0..2 and 300: radiance (pt_render_samples), and each sample's first-hit position and id byte (a one-sample pt_render);
    BVH in LDS, in global memory (FLAG_NO_LDS_SCENE = 2), the general walk (16)"""
    ex = _expect(oracle_mod, name, proj)
    _assert_hits_and_misses(ex, proj, name, (0, 1, 2, 300))
    r = _renderer(api, name, proj, flags)
    assert r.active_pixels()[0] == (0, W, 0, H)
    for first, n in ((0, 3), (300, 1)):
        got = r.render_samples(first, n)
        want = np.stack([ex.sample(s)[0] for s in range(first, first + n)])
        assert_bit_equal(got, want, f"{proj} {name} flags {flags} samples {first}..{first + n - 1}")
    for s in (0, 2, 300):
        r.reset_accumulation()
        got = r.render(s, 1, ident=np.zeros((H, W), np.uint32))
        col, pos, idb = ex.sample(s)
        _same_frame(got, (np.zeros_like(col) + col, pos, idb), f"{proj} {name} flags {flags} sample {s}")


@pytest.mark.parametrize("proj", list(PROJECTIONS))
def test_accumulation_ranks_and_batches(api, oracle_mod, proj):
    """pt_render(0, n): the f32 fold of the samples in order; both ranks of a two-way split; batch_spp 2 on two pipelines cuts 5 samples into 3 batches"""
    from path_tracer_amd.dist import rows_of_rank
    ex = _expect(oracle_mod, "mixed_env", proj)
    want = ex.frame(5)
    _same_frame(_renderer(api, "mixed_env", proj).render(0, 5), want, f"{proj}: 5 samples")
    _same_frame(_renderer(api, "mixed_env", proj, batch_spp=2, pipelines=2).render(0, 5), want, f"{proj}: 5 samples in batches of 2 on two pipelines")
    full = [np.zeros_like(w) for w in want]
    for rank in range(2):
        rr = _renderer(api, "mixed_env", proj, rank=rank, world_size=2, strip_rows=4)
        got = rr.render(0, 5)
        for f, g in zip(full, got):
            f[rows_of_rank(H, rank, 2, 4)] = g
        one = rr.render_samples(1, 1)
        assert_bit_equal(one[0], ex.sample(1)[0][rows_of_rank(H, rank, 2, 4)], f"{proj}: rank {rank} sample 1")
    _same_frame(full, want, f"{proj}: two ranks")


@pytest.mark.parametrize("proj", list(PROJECTIONS))
def test_multi_replicates_the_projection(api, oracle_mod, proj):
    ex = _expect(oracle_mod, "mixed_env", proj)
    m = api.MultiRenderer(_scene("mixed_env", proj), W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    m.rank0.set_environment(_env())
    m.rank0.set_projection(*PROJECTIONS[proj][0])
    got = m.render(0, 5)
    m.close()
    assert_bit_equal(got, ex.frame(5)[0], "pt_multi over a duplicated device")


def test_adaptive_rounds_under_a_panorama(api, oracle_mod):
    """two rounds of pt_render_adaptive: every pixel ends with exactly pt_render(0, n_p)'s bits, n_p its own count (test_gpu_adaptive.py's statement)"""
    ex = _expect(oracle_mod, "cornell", "panorama")
    r = _renderer(api, "cornell", "panorama", flags=api.FLAG_ADAPTIVE)
    M = 3
    first = np.stack([ex.sample(s)[0] for s in range(M)])
    lum = 0.2126 * first[..., 0] + 0.7152 * first[..., 1] + 0.0722 * first[..., 2]
    rel = np.sqrt(lum.var(0) / M) / np.maximum(lum.mean(0), 1e-3)
    threshold = float(np.quantile(rel[rel > 0], 0.5))     # the median relative error of the noisy pixels: the second round is a proper subset
    for _ in range(2):
        r.render_adaptive(M, threshold, 0.0, M, 0)
    acc, pos, idb = r.read_frame()
    counts = np.rint(acc[..., 3]).astype(np.int64)
    assert set(np.unique(counts)) == {M, 2 * M}, np.unique(counts)
    for n in (M, 2 * M):
        sel = counts == n
        oacc, opos, oid = ex.frame(n)
        assert_bit_equal(acc[sel], oacc[sel], f"accumulation of the {int(sel.sum())} pixels with {n} samples")
        assert_bit_equal(pos[sel], opos[sel], f"position of the pixels with {n} samples")
        assert np.array_equal(idb[sel], oid[sel]), f"id history of the pixels with {n} samples"


@pytest.mark.parametrize("proj", list(PROJECTIONS))
@pytest.mark.parametrize("name,flags,kw", [("cornell", 0, {}), ("instanced", 16, {}), ("mixed_env", 2, dict(rank=1, world_size=2))])
def test_guides_match_the_oracle_and_the_render(api, oracle_mod, proj, name, flags, kw):
    ex = _expect(oracle_mod, name, proj)
    r = _renderer(api, name, proj, flags, **kw)
    rows = r.local_rows()
    for k in (0, 2):
        _, pos, idb = r.render(0, k + 1) if k == 0 else r.render(1, k)
        r.render_guides(k)
        gpos, gnrm, gmodel = r.read_guides()
        opos, onrm, omodel, oleaf = ex.guides(k, rows)
        assert_bit_equal(gpos, opos, f"position guide, sample {k}")
        assert_bit_equal(gnrm, onrm, f"normal guide, sample {k}")
        assert np.array_equal(gmodel, omodel), f"model guide, sample {k}"
        assert np.array_equal(r.read_guide_instances(), oleaf), f"instance guide, sample {k}"
        assert_bit_equal(gpos, pos, f"guide vs render position, sample {k}")
        assert np.array_equal(gmodel & 0xFF, idb & 0xFFFF), f"guide vs render id byte, sample {k}"
        assert (gmodel == MISS).any() and (gmodel != MISS).any()


@pytest.mark.parametrize("proj", list(PROJECTIONS))
def test_denoise_and_mean_albedo(api, oracle_mod, proj):
    """pt_denoise on a projected frame's guides is the numpy restatement bit for bit; pt_accumulate_albedo is the fold of the albedo guides; a
    projection change makes both stale"""
    r = _renderer(api, "cornell", proj)
    r.render(0, 4)
    r.render_guides(3)
    acc = r.read_frame()[0]
    gpos, gnrm, gmodel = r.read_guides()
    assert_bit_equal(r.denoise(), denoise(acc, gpos, gnrm, gmodel, None), f"{proj}: pt_denoise")
    assert_bit_equal(r.denoise(iterations=2), denoise(acc, gpos, gnrm, gmodel, None, iterations=2), f"{proj}: pt_denoise, two levels")
    r.accumulate_albedo(0, 3)
    got = r.read_albedo()
    want = None
    for k in range(3):
        r.render_guides(k)
        al = r.read_guide_albedo()
        miss = r.read_guides()[2] == MISS
        a = np.concatenate([np.where(miss[..., None], F(1), al), np.ones(al.shape[:2] + (1,), F)], -1).astype(F)
        want = a if want is None else (want + a).astype(F)
    assert_bit_equal(got, want, f"{proj}: mean-albedo sums")
    assert_bit_equal(r.read_albedo(), want, "render_guides leaves the sums alone")
    kind, sx, sy, oh = PROJECTIONS[proj][0]
    r.set_projection(kind, 90.0 if kind == PANORAMA else 0.0, sy, oh * 2)
    for call in (r.read_albedo, lambda: r.denoise(iterations=1)):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == -3


def test_frames_under_a_panorama(api, oracle_mod):
    """three frames of a camera at rest are pt_render's accumulation; guides and the denoiser follow; once the camera moved the reprojection
    branch is refused and changes nothing"""
    ex = _expect(oracle_mod, "cornell", "panorama")
    r = _renderer(api, "cornell", "panorama")
    last = r.inv_projection()
    ident = np.zeros((H, W), np.uint32)
    for k in range(3):
        data, pos, ident = r.frame(k, last, ident)
        assert_bit_equal(data, ex.sample(k)[0], f"frame {k} data")
        assert_bit_equal(pos, ex.sample(k)[1], f"frame {k} position")
        last = r.inv_projection()
    want = ex.frame(3)
    assert_bit_equal(r.read_accumulation(), _renderer(api, "cornell", "panorama").render(0, 3)[0], "three frames vs pt_render(0, 3)")
    assert_bit_equal(r.read_accumulation(), want[0], "three frames vs the oracle's fold")
    assert np.array_equal(ident, want[2])
    r.render_guides(2)
    gpos, gnrm, gmodel = r.read_guides()
    assert_bit_equal(gpos, want[1], "guides of the last frame's sample")
    assert_bit_equal(r.denoise(), denoise(want[0], gpos, gnrm, gmodel, None), "pt_denoise after pt_frame")
    assert r.camera_input(api.EV_KEY_W, 0.0, 0.0, 1e-4)
    for frame in (r.frame, r.frame_moving):
        with pytest.raises(api.PtError) as e:
            frame(3, last)
        assert e.value.code == -3
    assert_bit_equal(r.read_accumulation(), want[0], "the refused frames changed nothing")


def test_perspective_is_untouched_by_a_projection_that_came_and_went(api, oracle_mod):
    from path_tracer_amd import scenes
    sc = scenes.cornell_mixed(W, H)
    fresh = api.Renderer(sc, W, H, max_bounces=DEPTH)
    want = fresh.render_samples(0, 4)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    r.set_projection(api.PROJ_PANORAMA)
    assert not np.array_equal(r.render_samples(0, 4), want)
    r.set_projection(api.PROJ_PERSPECTIVE)
    assert r.active_pixels()[0] == fresh.active_pixels()[0]
    assert_bit_equal(r.render_samples(0, 4), want, "perspective after a panorama")
    assert_bit_equal(want, oracle_mod.Oracle(sc).render_samples(W, H, 4, max_bounces=DEPTH), "perspective vs the oracle")
    r.reset_accumulation()
    _same_frame(r.render(0, 4, ident=np.zeros((H, W), np.uint32)), fresh.render(0, 4), "perspective frame after a panorama")


HEADLESS = {"panorama": (1, 0.0, 0.0, 0.0), "panorama:200:100": (1, 200.0, 100.0, 0.0), "ortho:600": (2, 0.0, 0.0, 600.0)}


@pytest.mark.parametrize("option", list(HEADLESS))
def test_headless_projection_with_the_denoiser(api, tmp_path, option):
    """examples/headless --projection ... --denoise: the C++ surface down to the two PNGs, against the Python route"""
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    from test_gpu_post import _read_png
    FRAMES, BOUNCES = 4, 3
    exe = B.build_host_driver()
    out_png, den_png = tmp_path / "out.png", tmp_path / "den.png"
    run = subprocess.run([exe, "--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--bounces", str(BOUNCES), "--projection", option,
                          "--out", str(out_png), "--denoise", str(den_png)], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(W / H))
    r = api.Renderer(sc, W, H, max_bounces=BOUNCES)
    r.set_projection(*HEADLESS[option])
    last = r.inv_projection()
    for k in range(FRAMES):
        r.frame(k, last, download=False)
    r.render_guides(FRAMES - 1)
    den = r.denoise()
    assert np.array_equal(_read_png(out_png), r.present_rgb8())
    assert np.array_equal(_read_png(den_png), r.post_rgb8(den))
    plain = api.Renderer(sc, W, H, max_bounces=BOUNCES)
    for k in range(FRAMES):
        plain.frame(k, last, download=False)
    assert not np.array_equal(plain.present_rgb8(), r.present_rgb8()), "the option changed the picture"


def test_headless_refuses_a_bad_projection(api):
    """the option's parse error, before anything is created, and the library's refusal through ptmi::Error"""
    from path_tracer_amd import build as B
    exe = B.build_host_driver()
    bad = subprocess.run([exe, "--projection", "fisheye"], capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode == 2 and "--projection" in bad.stderr
    bad = subprocess.run([exe, "--width", str(W), "--height", str(H), "--frames", "1", "--projection", "ortho:-3"], capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode == 1 and "ortho_height" in bad.stderr
