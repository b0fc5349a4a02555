"""Shared by tests/test_denoise_albedo_host.py and tests/test_gpu_denoise_albedo.py: the demodulated filter (pt_denoise_albedo /
pt_post_denoise_albedo) as denoise_common's numpy float32 restatement of include/pt_api.h composes it; and the scenes and images the two
suites use.  Nothing here calls the library."""
import numpy as np

from denoise_common import F, filtered


def denoise_albedo(acc, pos, nrm, model, albedo, sumsq=None, iterations=0, sigma_luminance=0.0, sigma_normal=0, sigma_plane=0.0):
    """the demodulated filter of include/pt_api.h: test_denoise_host.denoise's images and an h x w x 3 albedo -> h x w x 4"""
    return filtered(acc, pos, nrm, model, albedo, sumsq, iterations, sigma_luminance, sigma_normal, sigma_plane)


def mean_albedo(sums):
    """A of PT_ALBEDO_MEAN from pt_read_albedo's (sum r, sum g, sum b, n)"""
    sums = np.asarray(sums, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (sums[..., :3] / sums[..., 3:4]).astype(F)


def random_albedo(rng, h, w):
    """albedo in (0, 2) with some channels forced to 0 and some pixels forced to 1"""
    al = (rng.random((h, w, 3)).astype(F) * F(2)).astype(F)
    al[rng.random((h, w, 3)) < 0.08] = 0
    al[rng.random((h, w)) < 0.1] = 1
    return al


def checker_image(W=48, H=32, square=4, spp=4, seed=1):
    """The issue's flat one-model image: a checker albedo (0.875 / 0.125, green halved) times a smooth irradiance ramp E = 0.5 + x / W, spp
    noisy samples d = E * |1 + 0.6 N|.  Returns acc, pos, nrm, model, albedo, truth."""
    rng = np.random.default_rng(seed)
    x = np.arange(W, dtype=F)[None, :, None]
    E = np.broadcast_to(F(0.5) + x / F(W), (H, W, 1)).astype(F)
    chk = ((np.arange(H)[:, None] // square + np.arange(W)[None, :] // square) % 2).astype(bool)
    a = np.where(chk, F(0.125), F(0.875)).astype(F)
    albedo = np.stack([a, a * F(0.5), a], -1).astype(F)
    acc = np.zeros((H, W, 4), F)
    for _ in range(spp):
        d = (E * np.abs(F(1) + F(0.6) * rng.normal(size=(H, W, 1)).astype(F))).astype(F)
        acc[..., :3] += albedo * d
        acc[..., 3] += F(1)
    pos = np.zeros((H, W, 4), F); pos[..., 0] = np.arange(W, dtype=F)[None]; pos[..., 1] = np.arange(H, dtype=F)[:, None]; pos[..., 3] = F(5)
    nrm = np.zeros((H, W, 3), F); nrm[..., 2] = 1
    return acc, pos, nrm, np.zeros((H, W), np.uint32), albedo, (albedo * E).astype(F)


def rmse(a, ref):
    return float(np.sqrt(np.mean((np.asarray(a)[..., :3].astype(np.float64) - np.asarray(ref)[..., :3].astype(np.float64)) ** 2)))


def checker_scene(width, height):
    """A checker-textured Lambertian floor and back wall (one 8 x 8 texture of texels 0.9 / 0.1: 8 squares across each), lit by a light above
    the view; open to the sides."""
    from path_tracer_amd.scene_desc import Camera, Emissive, Lambertian, Model, SceneDesc, Texture
    from textures_common import quad
    t = np.where((np.add.outer(np.arange(8), np.arange(8)) % 2).astype(bool), F(0.1), F(0.9)).astype(F)
    lam = Lambertian.new((1.0, 1.0, 1.0)).textured(Texture.new(np.repeat(t[..., None], 3, -1)))
    fp, fn = quad((-8.0, -4.0, -8.0), (-8.0, -4.0, 8.0), (8.0, -4.0, 8.0), (8.0, -4.0, -8.0))
    bp, bn = quad((-8.0, -4.0, -8.0), (8.0, -4.0, -8.0), (8.0, 6.0, -8.0), (-8.0, 6.0, -8.0))
    uv = np.array([[[0.0, 0.0], [0.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]], F)
    lp, ln = quad((-3.0, 5.9, -3.0), (3.0, 5.9, -3.0), (3.0, 5.9, 3.0), (-3.0, 5.9, 3.0))
    models = [Model.new(lp, ln, Emissive.new((6.0, 5.0, 4.0)), None, "light"), Model.new(fp, fn, lam, None, "floor", uvs=uv),
              Model.new(bp, bn, lam, None, "back", uvs=uv)]
    return SceneDesc.new(models, Camera.new((1.0, 1.5, 9.0), (0.0, -1.0, -2.0), 65.0, width / height), "checker floor and wall")
