"""GPU (-m gpu): lightmap bakes with direct light sampled at the texel (pt_bake_lightmap_direct, pt_bake_lightmap_adaptive_direct,
pt_lightmap_light_sample on the device), bit for bit.  Expected values are the numpy restatement of tests/lightmap_direct_common.py: stream
draws, the oracle's light table and triangles, Oracle.trace_any for the shadow ray, Oracle.integrate with its first-hit id for the gather
ray, folded in numpy in sample order."""
import numpy as np
import pytest

import baked_common as BC
import guides_follow_common as G
import lightmap_adaptive_common as LA
import lightmap_common as LC
import lightmap_direct_common as LD
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
NO_LDS_SCENE = 2
KEY_BASE = 5000          # chosen on the RESTATEMENT: under these streams every bake case has a gather ray that meets a lamp first (asserted below)
BIAS = 0.25


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---- 1. the hook on the device
@pytest.mark.parametrize("name", ["quad", "short", "two_lamps", "emtex"])
def test_device_light_sample_equals_the_host(api, oracle_mod, name):
    keys, smp, o, n, want = LD.hook_inputs(oracle_mod, name)
    r = LD.renderer(api, name)
    host = r.lightmap_light_sample(keys, smp, o, n, on_device=False)
    dev = r.lightmap_light_sample(keys, smp, o, n, on_device=True)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[0], want["light"]), name
    for d, h, what in zip(dev[1:], host[1:], ("dir", "t_max", "ce")):
        assert_bit_equal(d, h, f"{name}: {what}")
    assert (dev[3] > 0).any() and len(keys) > 256          # more than one block


# ---- 2. the bakes against the restatement
BAKES = {"short": 4, "instanced": 3, "emtex": 4, "two_lamps": 4}


def _check_bake(api, O, name, batch_spp, moments, flags=0):
    sc, model, instance, w, h = LD.case(name)[:5]
    n = BAKES[name]
    s = LD.expected_bake(O, name, n, key_base=KEY_BASE, bias=BIAS)
    # the case means something: a gather ray that met a lamp first, a blocked light sample and one that arrives
    assert s["zeroed"].any() and (s["blocked"] & s["cast"]).any() and (s["D"] > 0).any(), name
    rng = np.random.default_rng(5)
    start = rng.uniform(-1, 1, (h, w, 3)).astype(F); start_sq = rng.uniform(0, 1, (h, w)).astype(F)
    want, want_sq = LD.fold(start, start_sq if moments else None, s["k"], s["X"], n)
    r = LD.renderer(api, name, flags=flags, batch_spp=batch_spp)
    before = r.stats().paths
    got = r.bake_lightmap_direct(model, instance, w, h, n, key_base=KEY_BASE, bias=BIAS, sums=start.copy(), sumsq=start_sq.copy() if moments else None)
    what = f"{name} batch_spp {batch_spp} moments {moments} flags {flags}"
    cov = got[-1]
    assert np.array_equal(cov, (LD.table_of(name)[0] != LC.MISS).astype(np.uint8)), what + ": coverage"
    assert_bit_equal(got[0], want, what + ": sums")
    assert_bit_equal(got[0][cov == 0], start[cov == 0], what + ": uncovered texels")
    if moments:
        assert_bit_equal(got[1], want_sq, what + ": sumsq")
    assert r.stats().paths - before == len(s["k"]) * n
    return r, got


@pytest.mark.parametrize("moments", [False, True], ids=["sums", "moments"])
@pytest.mark.parametrize("batch_spp", [0, 1, 3])
@pytest.mark.parametrize("name", list(BAKES))
def test_bake_against_the_restatement(api, oracle_mod, name, batch_spp, moments):
    """batch_spp 1 and 3 cut a texel's samples across wavefront batches and (three batches to a table) across ray tables"""
    _check_bake(api, oracle_mod, name, batch_spp, moments)


# ---- 3. continuation, and the BVH in global memory
def test_split_bakes_continue_and_the_bvh_may_live_in_global_memory(api, oracle_mod):
    sc, model, instance, w, h = LD.case("short")[:5]
    s = LD.expected_bake(oracle_mod, "short", 5, key_base=KEY_BASE, bias=BIAS)
    zero = np.zeros((h, w, 3), F); zero_sq = np.zeros((h, w), F)
    want, want_sq = LD.fold(zero, zero_sq, s["k"], s["X"], 5)
    r = LD.renderer(api, "short")
    a, a_sq, _ = r.bake_lightmap_direct(model, instance, w, h, 3, key_base=KEY_BASE, bias=BIAS, moments=True)
    b, b_sq, _ = r.bake_lightmap_direct(model, instance, w, h, 2, first_sample=3, key_base=KEY_BASE, bias=BIAS, sums=a, sumsq=a_sq)
    assert_bit_equal(b, want, "bake(0, 3) then bake(3, 2): sums")
    assert_bit_equal(b_sq, want_sq, "bake(0, 3) then bake(3, 2): sumsq")
    g = LD.renderer(api, "short", flags=NO_LDS_SCENE)
    whole, whole_sq, _ = g.bake_lightmap_direct(model, instance, w, h, 5, key_base=KEY_BASE, bias=BIAS, moments=True)
    assert g.stats().lds_scene == 0 and r.stats().lds_scene == 1
    assert_bit_equal(whole, want, "global BVH: sums")
    assert_bit_equal(whole_sq, want_sq, "global BVH: sumsq")


# ---- 4. the adaptive contract
def test_adaptive_rounds_hold_every_texel_to_the_direct_bake_at_its_count(api, oracle_mod):
    """three rounds of 2 samples on the 12 x 8 short box.  The selection is restated (lightmap_adaptive_common.active) on the restated sums,
    so the expected counts come from nothing of the library; rel_error 0.25 stops the texels that see the lamp unshadowed after their
    first round (their D hardly varies) and keeps the ones the gather term dominates"""
    sc, model, instance, w, h = LD.case("short")[:5]
    crit = dict(rel_error=0.25, abs_floor=0.0, min_samples=2, max_samples=0)
    s = LD.expected_bake(oracle_mod, "short", 6, key_base=KEY_BASE, bias=BIAS)
    cov = LD.table_of("short")[0] != LC.MISS
    k = s["k"]
    X = s["X"].reshape(len(k), 6, 3)
    rng = np.random.default_rng(9)
    sums = np.where(cov[..., None], F(0), rng.uniform(-1, 1, (h, w, 3))).astype(F)
    sq = np.where(cov, F(0), rng.uniform(0, 1, (h, w))).astype(F)
    counts = np.where(cov, 0, 0xFFFFFFFF).astype(np.uint32)
    want = (sums.copy(), sq.copy(), counts.copy())
    r = LD.renderer(api, "short")
    for rnd in range(3):
        act = LA.active(want[0], want[1], want[2], cov, **crit)
        ws, wq, wc = (a.copy() for a in want)
        for j, t in enumerate(k):
            y, x = divmod(int(t), w)
            if act[y, x]:
                c0 = int(wc[y, x])
                one, one_sq = LD.fold(ws[y, x].reshape(1, 1, 3), wq[y, x].reshape(1, 1), np.array([0]), X[j, c0:c0 + 2], 2)
                ws[y, x], wq[y, x], wc[y, x] = one.reshape(3), one_sq.reshape(()), c0 + 2
        want = (ws, wq, wc)
        sums, sq, counts, cv, n_active = r.bake_lightmap_adaptive_direct(model, instance, w, h, 2, key_base=KEY_BASE, bias=BIAS, sums=sums, sumsq=sq, counts=counts,
                                                                          **crit)
        assert n_active == int(act.sum()) and np.array_equal(cv, cov.astype(np.uint8)), rnd
        assert np.array_equal(counts, want[2]), rnd
        assert_bit_equal(sums, want[0], f"round {rnd}: sums (inactive and uncovered texels included)")
        assert_bit_equal(sq, want[1], f"round {rnd}: sumsq")
    assert len(np.unique(counts[cov])) > 1, np.unique(counts[cov])
    # THE CONTRACT: every covered texel holds pt_bake_lightmap_direct with sumsq at its own count
    for n in np.unique(counts[cov]):
        whole, whole_sq, _ = r.bake_lightmap_direct(model, instance, w, h, int(n), key_base=KEY_BASE, bias=BIAS, moments=True)
        at = cov & (counts == n)
        assert_bit_equal(sums[at], whole[at], f"texels with {n} samples: sums")
        assert_bit_equal(sq[at], whole_sq[at], f"texels with {n} samples: sumsq")


# ---- 5. neighbours keep their bits
def test_plain_bakes_and_renders_keep_their_bits_around_a_direct_bake(api):
    sc, model, instance, w, h = LD.case("short")[:5]
    r = LD.renderer(api, "short")

    def neighbours():
        plain = r.bake_lightmap(model, instance, w, h, 4, key_base=KEY_BASE, bias=BIAS)[0]
        mom = r.bake_lightmap_moments(model, instance, w, h, 4, key_base=KEY_BASE, bias=BIAS)
        r.reset_accumulation()
        return plain, mom[0], mom[1], r.render(0, 2)[0]

    before = neighbours()
    paths = r.stats().paths
    sums, cov = r.bake_lightmap_direct(model, instance, w, h, 4, key_base=KEY_BASE, bias=BIAS)
    assert r.stats().paths - paths == int(cov.sum()) * 4 and cov.sum() == 80
    after = neighbours()
    for a, b, what in zip(before, after, ("pt_bake_lightmap", "pt_bake_lightmap_moments: sums", "pt_bake_lightmap_moments: sumsq", "pt_render")):
        assert_bit_equal(a, b, what)
    assert (sums != before[0]).any()


# ---- 6. the baked view shows the map
def test_baked_view_shows_a_direct_map(api, oracle_mod):
    sc, model, instance, w, h = LD.case("short")[:5]
    r = LD.renderer(api, "short")
    sums, cov = r.bake_lightmap_direct(model, instance, w, h, 4, key_base=KEY_BASE, bias=BIAS)
    r.set_lightmap_sums(model, instance, sums, 4)
    orc = LD.oracle_of(oracle_mod, "short")
    o, d = G.pinhole_rays(orc, 48, 32, 0)
    unlit = (0.25, 0.5, 0.125)
    want, ending = BC.baked(orc, sc, {(model, instance): (sums / F(4)).astype(F)}, o, d, 0, unlit)
    assert (ending == BC.MAPPED_FRONT).sum() > 20
    r.reset_baked()
    got = r.render_baked(0, 1, follow=0, unlit=unlit)
    assert_bit_equal(got[..., :3], want.reshape(32, 48, 3), "render_baked over a direct map")


# ---- 7. the C++ surface
def test_headless_bakes_a_direct_lightmap(api, tmp_path):
    """examples/headless --bake-lightmap 16 16 8 2 out.txt --direct parses back to the Python surface's direct bake and dilation under the same
    UVs, with the light samples' streams behind the gather samples' (light_key_base = 16 * 16)"""
    import os
    import subprocess
    from conftest import ROOT
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    Wd, Hd, BOUNCES = 48, 32, 4
    exe = B.build_host_driver()
    out_txt = tmp_path / "lightmap.txt"
    run = subprocess.run([exe, "--width", str(Wd), "--height", str(Hd), "--frames", "1", "--bounces", str(BOUNCES), "--bake-lightmap", "16", "16", "8", "2",
                          str(out_txt), "--direct"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    rows = [line.split() for line in out_txt.read_text().splitlines()]
    assert len(rows) == 256 and all(len(v) == 4 for v in rows)
    got = np.array([[float.fromhex(x) for x in v[1:]] for v in rows], np.float64).astype(F).reshape(16, 16, 3)
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(Wd / Hd))
    r = api.Renderer(sc, Wd, Hd, max_bounces=BOUNCES)
    p = r.model_vertices(1)[0].reshape(-1, 3)[:, [0, 2]]
    lo, hi = p.min(0), p.max(0)
    r.set_model_uvs(1, ((p - lo) / (hi - lo)).astype(F).reshape(-1, 3, 2))
    r.rebuild()
    sums, cov = r.bake_lightmap_direct(1, 0, 16, 16, 8, bias=0.25, light_key_base=256)
    want, _ = r.dilate_lightmap(sums, cov, 2)
    assert_bit_equal(got, want, "headless --bake-lightmap --direct")
    assert (sums != r.bake_lightmap(1, 0, 16, 16, 8, bias=0.25)[0]).any()
