"""GPU: the texel-space denoiser (pt_lightmap_denoise on the device, pt_bake_lightmap_moments), bit for bit: the kernels against the numpy
restatement of tests/lightmap_denoise_common.py on the grid the host tests use, and, with the reach switched off, against the frame filter's
own kernels (pt_post_denoise) on the equivalent images; the moments bake against pt_bake_lightmap, pt_integrate_rays and a numpy fold; and the
filter's purpose: a denoised 16-sample bake is closer to a 4096-sample reference than the raw 16-sample mean."""
import numpy as np
import pytest

import denoise_common as DC
import lightmap_common as LC
import lightmap_denoise_common as LD
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH = 48, 32, 6
OFF = 1e30          # reach * reach overflows: the term is off


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


_RENDERERS = {}


def renderer(api, kind):
    if kind not in _RENDERERS:
        _RENDERERS[kind] = api.Renderer(LD.scene(kind)[0], W, H, max_bounces=DEPTH)
    return _RENDERERS[kind]


# ---- 1. the kernels are the definition
@pytest.mark.parametrize("kind, w, h, it, moments", LD.case_ids())
def test_device_filter_is_the_definition(api, kind, w, h, it, moments):
    table, sums, sumsq, (want, want_area) = LD.expected(kind, w, h, it, moments)
    got, area = renderer(api, kind).denoise_lightmap(LD.scene(kind)[1], 0, sums, LD.N_SAMPLES, sumsq=sumsq, iterations=it, on_device=True, want_area=True)
    assert_bit_equal(area, want_area, "texel area")
    assert_bit_equal(got, want, f"{kind} {w}x{h}, {it} levels, moments {moments}")
    assert (table[0] != LC.MISS).any() and (w * h == 1 or np.abs(got - sums / F(LD.N_SAMPLES))[table[0] != LC.MISS].max() > 0)


def test_device_equals_host_on_a_map_of_many_workgroups(api):
    """130 x 70: 9 x 5 workgroups with ragged edges on both sides, default parameters (5 levels)"""
    r = renderer(api, "box")
    sums, sumsq = LD.synthetic(130, 70, LD.N_SAMPLES, seed=2)
    for sq in (sumsq, None):
        host = r.denoise_lightmap(LD.scene("box")[1], 0, sums, LD.N_SAMPLES, sumsq=sq, on_device=False, want_area=True)
        dev = r.denoise_lightmap(LD.scene("box")[1], 0, sums, LD.N_SAMPLES, sumsq=sq, on_device=True, want_area=True)
        assert_bit_equal(dev[1], host[1], "texel area")
        assert_bit_equal(dev[0], host[0], "130 x 70")


# ---- 2. pinned to the frame filter's kernels
@pytest.mark.parametrize("kind, w, h", [("box", 37, 19), ("box", 48, 32), ("two", 16, 16), ("quad", 1, 1)])
@pytest.mark.parametrize("moments", [True, False])
def test_without_reach_it_is_the_frame_filter(api, kind, w, h, moments):
    r = renderer(api, kind)
    table = LD.table_of(kind, w, h)
    sums, sumsq = LD.synthetic(w, h, LD.N_SAMPLES, seed=5)
    sq = sumsq if moments else None
    acc, pos, nrm, model = LD.frame_images(table, sums, LD.N_SAMPLES)
    for it in (1, 4, 8):
        want = r.post_denoise(acc, pos, nrm, model, sumsq=sq, iterations=it)
        got = r.denoise_lightmap(LD.scene(kind)[1], 0, sums, LD.N_SAMPLES, sumsq=sq, iterations=it, reach=OFF, on_device=True)
        assert_bit_equal(got, want[..., :3], f"{kind} {w}x{h} moments {moments}, {it} levels: reach off")


# ---- 3. the moments bake
_BAKES = {}


def cornell(api):
    if "r" not in _BAKES:
        sc, model = LC.cornell_atlas_scene("cb_box_short", W, H)
        _BAKES["r"] = (api.Renderer(sc, W, H, max_bounces=DEPTH), sc, model)
    return _BAKES["r"]


def test_moments_bake_is_the_bake_and_the_fold(api, oracle_mod):
    r, sc, model = cornell(api)
    w, h, n = 48, 32, 8
    plain, plain_cov = r.bake_lightmap(model, 0, w, h, n, bias=0.25)
    sums, sumsq, cov = r.bake_lightmap_moments(model, 0, w, h, n, bias=0.25)
    assert np.array_equal(cov, plain_cov) and cov.sum() > 500 and not cov.all()
    assert_bit_equal(sums, plain, "rgb_sum of the moments bake")
    m = sc.models[model]
    table = LC.texels(m.positions, m.normals, m.uvs, m.matrices[0], w, h)
    k, o, d, keys, samples = LC.bake_rays(oracle_mod, table, n, bias=0.25)
    rad = r.integrate_rays(o, d, keys, samples)[0].reshape(len(k), n, 4)
    want = np.zeros(w * h, F)
    for s in range(n):
        l = DC.lum(rad[:, s, :3])
        want[k] = want[k] + l * l
    assert want.dtype == F and (want[k] > 0).any()
    assert_bit_equal(sumsq, want.reshape(h, w), "sumsq against a numpy fold of l(L)^2")
    assert not sumsq[cov == 0].any()
    a = r.bake_lightmap_moments(model, 0, w, h, 3, bias=0.25)
    b = r.bake_lightmap_moments(model, 0, w, h, 5, first_sample=3, bias=0.25, sums=a[0], sumsq=a[1])
    assert_bit_equal(b[0], sums, "sums of (0, 3) then (3, 5)")
    assert_bit_equal(b[1], sumsq, "sumsq of (0, 3) then (3, 5)")


# ---- 4. it denoises
def rmse(a, b, covered):
    d = (a.astype(np.float64) - b.astype(np.float64))[covered]
    return float(np.sqrt((d * d).mean()))


def test_denoised_16_samples_beat_the_raw_mean(api):
    """Cornell short box, 48 x 32, default parameters, RMSE over covered texels against a 4096-sample bake of disjoint samples (first_sample =
    16): the denoised 16-sample bake (moments) must have a lower RMSE than the raw 16-sample mean, with no margin."""
    r, _, model = cornell(api)
    w, h = 48, 32
    ref, cov = r.bake_lightmap(model, 0, w, h, 4096, first_sample=16, bias=0.25)
    ref = ref / F(4096)
    covered = cov == 1
    sums, sumsq, _ = r.bake_lightmap_moments(model, 0, w, h, 16, bias=0.25)
    raw = sums / F(16)
    den = r.denoise_lightmap(model, 0, sums, 16, sumsq=sumsq)
    e_raw, e_den = rmse(raw, ref, covered), rmse(den, ref, covered)
    print(f"RMSE against the 4096-sample reference over {int(covered.sum())} texels: raw 16-sample mean {e_raw:.6f}, denoised {e_den:.6f}")
    assert e_den < e_raw, (e_den, e_raw)


# ---- 5. the C++ surface
def test_headless_denoises_the_map_it_bakes(api, tmp_path):
    """examples/headless --bake-lightmap 16 16 8 2 out.txt --lightmap-denoise writes the dilated texel MEANS of the Python surface's moments
    bake and filter under the same UVs"""
    import os
    import subprocess
    from conftest import ROOT
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES = 48, 32, 4
    exe = B.build_host_driver()
    out_txt = tmp_path / "lightmap.txt"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--bake-lightmap", "16", "16", "8", "2",
                          str(out_txt), "--lightmap-denoise"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    rows = [line.split() for line in out_txt.read_text().splitlines()]
    assert len(rows) == 256 and all(len(v) == 4 for v in rows)
    got = np.array([[float.fromhex(x) for x in v[1:]] for v in rows], np.float64)
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    p = r.model_vertices(1)[0].reshape(-1, 3)[:, [0, 2]]
    lo, hi = p.min(0), p.max(0)
    r.set_model_uvs(1, ((p - lo) / (hi - lo)).astype(F).reshape(-1, 3, 2))
    r.rebuild()
    sums, sumsq, cov = r.bake_lightmap_moments(1, 0, 16, 16, 8, bias=0.25)
    mean = r.denoise_lightmap(1, 0, sums, 8, sumsq=sumsq)
    want, _ = r.dilate_lightmap(mean, cov, 2)
    assert_bit_equal(got.astype(F).reshape(16, 16, 3), want, "headless --lightmap-denoise")
    assert (want > 0).any() and np.abs(want - sums / F(8)).max() > 0
    refused = subprocess.run([exe, "--lightmap-denoise"], capture_output=True, text=True, cwd=ROOT)
    assert refused.returncode == 2 and "--bake-lightmap" in refused.stderr
