"""CPU: the oracle's surface materials against an independent binary64 statement of the reference (tests/materials_common.py), at the
edges: grazing and normal incidence, the critical angle, the onb_ggx flip, extreme uniforms, and for get_bsdf_pdf the directions
next-event estimation asks about.  Every GPU test compares with the oracle bit for bit, so this is what keeps a mistake made the same
way on both sides from passing."""
import numpy as np
import pytest

import materials_common as MC

F = np.float32
NAMES = list(MC.materials())


def _eval(O, name):
    return MC.oracle_edge_outputs(O, name)


def test_numpy_stream_is_the_oracles(oracle_mod):
    L = oracle_mod.lib()
    rng = np.random.default_rng(1)
    px = rng.integers(0, 1 << 32, 1000, dtype=np.uint64); sm = rng.integers(0, 1 << 32, 1000, dtype=np.uint64)
    s0 = MC.stream_state0(oracle_mod.DEFAULT_SEED, px, sm)
    assert [int(v) for v in s0] == [L.pto_stream_state0(oracle_mod.DEFAULT_SEED, int(p), int(s)) for p, s in zip(px, sm)]
    for k in (0, 1, 2, 3, 1000):
        assert [int(v) for v in MC.wyrand_u64(s0, k)] == [L.pto_wyrand(int(s), k) for s in s0]
    assert MC.SEED == oracle_mod.DEFAULT_SEED


def test_edge_key_fixture_is_current(oracle_mod):
    """every committed key draws, through the oracle's own stream, the extreme value it was kept for"""
    L = oracle_mod.lib()
    ek = MC.edge_keys()
    assert int(ek["seed"]) == oracle_mod.DEFAULT_SEED
    seen = set()
    for px, sm, index, kind, u32 in zip(ek["pixel"], ek["sample"], ek["index"], ek["kind"], ek["u32"]):
        got = L.pto_wyrand(L.pto_stream_state0(oracle_mod.DEFAULT_SEED, int(px), int(sm)), int(index)) & 0xFFFFFFFF
        assert got == int(u32), (px, sm, index)
        u = F(F(got) / F(4294967296.0))
        assert [0 < u < F(1e-6), F(0.9998) < u < 1, u == F(1.0), u == F(0.0) and got == 0][int(kind)], (px, sm, index, kind, u)
        seen.add((int(index) - MC.DRAWS_CONSUMED, int(kind)))
    assert seen == {(j, k) for j in range(3) for k in range(4)}       # every kind at every draw the materials consume


def test_edge_inputs_are_finite_unit_and_reach_the_edges():
    for name, m in MC.materials().items():
        inc, nrm, front, px, sm = MC.edge_inputs(m)
        bi = MC.bsdf_inputs(m)
        for v in (inc, nrm, bi[0], bi[1], bi[2]):
            assert v.dtype == F and np.isfinite(v).all()
            assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() < 4e-7
        cos = -(inc.astype(np.float64) * nrm).sum(1)
        assert cos.min() > 0 and cos.min() < 2e-6 and cos.max() >= 1.0 and set(front) == {0, 1}
        assert 10000 <= len(px) <= 70000 and 10000 <= len(bi[0]) <= 70000
        u = MC.edge_uniforms(px, sm)
        assert (u == 0.0).any(0).all() and (u == 1.0).any(0).all() and ((u > F(0.9998)) & (u < 1)).any(0).all()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_material_eval_matches_binary64(oracle_mod, name):
    e = _eval(oracle_mod, name)
    inc, nrm, front, px, sm = e["inputs"]
    MC.check_material_eval(e["out"], e["m"], inc, nrm, front, e["u"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_bsdf_eval_matches_binary64(oracle_mod, name):
    e = _eval(oracle_mod, name)
    rows, degenerate = MC.check_bsdf_eval(e["out4"], e["m"], *e["bsdf_inputs"])
    print(f"{name}: {rows} rows, {degenerate} with a denominator within rounding of zero")
    assert degenerate <= 0.13 * rows


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b)).astype(np.float64)


@pytest.mark.parametrize("name", ["lambertian", "specular", "dielectric"])
def test_throughput_identities(oracle_mod, name):
    """integrator.rs:249 multiplies the path weight by weakening * bsdf / pdf.  In exact arithmetic the reference's own formulas make that
    the colour for Lambertian (material.rs:109-115) and Specular (:155), 1 for a reflected smooth-dielectric sample and colour / eta^2
    for a refracted one (:511-527); in binary32, where the pdf is not zero, a few ulp (three roundings of a product and a quotient)."""
    e = _eval(oracle_mod, name)
    out = e["out"]
    inc, nrm, front = e["inputs"][:3]
    colour = np.array(e["m"].colour, F)
    ok = (out[:, 6] != 0) & np.isfinite(out[:, 0:7]).all(1)
    assert ok.sum() > 0.8 * len(out)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (out[:, 7:8] * out[:, 3:6] / out[:, 6:7]).astype(F)
    if name != "dielectric":
        # the Lambertian pdf is dot(outgoing, normal) / pi WITH its sign while the weakening is the absolute value: a draw of exactly 1.0 puts
        # the direction in the surface plane, where that dot product is rounding residue of either sign.  A negative one gives minus the
        # colour, which integrate never uses: it ends the path on pdf < 0 (integrator.rs:243).  Such rows must come from u1 == 1.0 alone.
        neg = ok & (out[:, 6] < 0)
        assert (e["u"][neg, 0] == 1.0).all() and (neg.sum() > 0) == (name == "lambertian")
        assert _ulps(w[neg], np.broadcast_to(-colour, w[neg].shape)).max(initial=0) <= 4
        ok &= ~neg
        assert _ulps(w[ok], np.broadcast_to(colour, w[ok].shape)).max() <= 4
        return
    up = (out[:, 0:3].astype(np.float64) * nrm).sum(1) > 0                       # the side get_bsdf_pdf decides by (material.rs:517)
    assert (ok & up).sum() > 1000 and (ok & ~up).sum() > 1000
    assert _ulps(w[ok & up], F(1.0)).max() <= 4
    eta = np.where(front != 0, F(1.0) / F(e["m"].ior), F(e["m"].ior)).astype(F)
    want = (colour[None, :] / (eta * eta)[:, None]).astype(F)
    assert _ulps(w[ok & ~up], want[ok & ~up]).max() <= 4


@pytest.mark.parametrize("name", NAMES)
def test_directions_are_unit_and_obey_the_laws(oracle_mod, name):
    """in binary64: every returned direction has length 1 to 1e-5; a Specular or reflected Dielectric direction is the mirror image of the
    incoming one; a refracted Dielectric direction obeys Snell's law and lies in the plane of incidence"""
    e = _eval(oracle_mod, name)
    out = e["out"].astype(np.float64)
    inc, nrm, front = [a.astype(np.float64) for a in e["inputs"][:3]]
    d = out[:, 0:3]
    fin = np.isfinite(d).all(1)
    assert np.abs(np.linalg.norm(d[fin], axis=1) - 1.0).max() < 1e-5
    if name not in ("specular", "dielectric"):
        assert fin.all()                                                         # a GGX sampler never returns NaN: r is clamped, material.rs:265
        return
    side = (d * nrm).sum(1)
    cos_i = -(inc * nrm).sum(1)
    refl = fin & (side > 0)
    assert np.abs(side[refl] - cos_i[refl]).max() < 1e-6                         # angle of reflection = angle of incidence
    tang_i = inc + cos_i[:, None] * nrm
    tang_o = d - side[:, None] * nrm
    assert np.abs(tang_o[refl] - tang_i[refl]).max() < 1e-6                      # and the tangential part goes straight on
    if name == "dielectric":
        refr = fin & (side <= 0)
        eta = np.where(front != 0, 1.0 / 1.5, 1.5)
        assert refr.sum() > 1000
        assert np.abs(tang_o[refr] - eta[refr, None] * tang_i[refr]).max() < 1e-6        # Snell, as a vector: sin_t = eta sin_i, same plane
        assert (~fin).sum() > 0                                                  # u == 1.0 under total internal reflection: NaN, as the reference


def test_rough_metal_reaches_the_finisher_with_non_finite_radiance(oracle_mod):
    """A roughness-1 GGX metal reflects below its own surface at grazing incidence; get_bsdf_pdf answers (0, 0), and weakening * bsdf / pdf
    is 0 / 0 (integrator.rs:249).  The next estimate poisons the sum and the finisher returns (0, 0, 0, 1) (integrator.rs:272-280).  Such
    a result shows as: the first hit alone (max_bounces 0, next-event estimation on) gathers light, the whole path returns exactly
    zero.  The designed set must hold some, so that test_designed_rays_against_the_oracle covers those NaN semantics on the device."""
    first = MC.oracle_rays(oracle_mod, "metal_1.0", "overhead", "lds", 0, True)[0]
    whole = MC.oracle_rays(oracle_mod, "metal_1.0", "overhead", "lds", 6, True)[0]
    zeroed = (first[:, :3] > 0).any(1) & (whole[:, :3] == 0).all(1)
    print("results the finisher zeroed:", int(zeroed.sum()), "of", len(whole))
    assert zeroed.sum() > 0


def test_nan_pdf_keys_are_current(oracle_mod):
    """the committed keys still draw exactly 1.0 where the path meets the dielectric sheet, and the oracle's path under them gathers light
    at the first hit and returns exactly zero as a whole: the NaN pdf was walked past (NaN < 0 is false, integrator.rs:243) and the
    finisher zeroed the sum.  test_gpu_materials.py runs the same rays through the shading kernels."""
    L = oracle_mod.lib()
    orc = oracle_mod.Oracle(MC.nan_pdf_scene())
    o, d, key, sample = MC.nan_pdf_rays()
    n = len(key) // 2
    assert n >= 4
    for i in range(n):
        draw = L.pto_wyrand(L.pto_stream_state0(oracle_mod.DEFAULT_SEED, int(key[i]), 0), MC.NAN_PDF_DRAW) & 0xFFFFFFFF
        assert F(F(draw) / F(4294967296.0)) == F(1.0)
        first = orc.integrate(o[i], d[i], int(key[i]), 0, MC.DRAWS_CONSUMED, max_bounces=0)[0]
        whole = orc.integrate(o[i], d[i], int(key[i]), 0, MC.DRAWS_CONSUMED, max_bounces=6)[0]
        assert (first[:3] > 0).all() and (whole == np.array([0, 0, 0, 1], F)).all()
    others = [orc.integrate(o[i], d[i], int(key[i]), 0, MC.DRAWS_CONSUMED, max_bounces=6)[0] for i in range(n, 2 * n)]
    assert any((w[:3] > 0).any() for w in others)
