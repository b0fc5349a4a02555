"""Texture record (profiles/r12_textures.md): what textured surface colour costs.  The 1080p Cornell frame untextured, with its floor, ceiling
and walls on a 1024 x 1024 checker, and the same on an 8 x 8 one — same build, same process, interleaved: wall clock of the blocking
pt_render_device per frame (median of --reps, after a warm-up frame of each).  The 8 x 8 texture lives in cache, so its ratio is the cost of the
TEX shading variants (and of queueing the shadow rays the untextured frame walks inline); the 1024 x 1024 ratio adds the texel traffic.

    python tools/texture_bench.py [--width 1920 --height 1080 --spp 256 --bounces 8 --reps 5 --repeat 8] [--out file.json]
    python tools/texture_bench.py --only tex1024 --reps 1      one variant alone, e.g. under rocprofv3 --kernel-trace --stats
    python tools/texture_bench.py --emission --reps 5          adds `emit8`: the untextured frame with its LIGHT on an 8 x 8 checker emission texture
                                                               (profiles/r17_emission_textures.md): emit8_over_plain beside tex8_over_plain
    python tools/texture_bench.py --normal --reps 5            adds `nmap8`: the frame with its floor, ceiling and walls under an 8 x 8 ripple NORMAL map instead
                                                               of the checker, same UVs (profiles/r18_normal_maps.md): nmap8_over_plain, nmap8_over_tex8
    python tools/texture_bench.py --roughness --reps 7         INSTEAD of the variants above (profiles/r33_roughness_maps.md): the texel-corner room of
                                                               tests/textures_common.py and the `mixed` Cornell box, each without textures (`*_plain`),
                                                               colour-textured (`*_tex`) and colour-textured with an 8 x 8 roughness checker of 0.1 / 0.6 on
                                                               its GGX materials (`*_rough`); every frame's time is kept (`ms_all`), so that two builds'
                                                               runs can be held against each other's spread.  A build without roughness maps measures
                                                               the first two states
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def checker(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    return np.repeat(np.where((i + j) & 1, np.float32(0.2), np.float32(1.0))[..., None], 3, axis=2)


def planar_uvs(positions, repeat):
    """UVs over the two longest axes of the model's extent, `repeat` periods across it"""
    p = np.asarray(positions, np.float32)
    lo, hi = p.min(axis=(0, 1)), p.max(axis=(0, 1))
    ax = np.sort(np.argsort(hi - lo)[1:])
    return (p[:, :, ax] - lo[ax]) / (hi - lo)[ax] * np.float32(repeat)


def textured_cornell(scenes, W, H, n, repeat):
    from path_tracer_amd.scene_desc import Model, SceneDesc, Texture
    tex = Texture.new(checker(n))
    models = []
    for m in scenes.cornell_models():
        if m.name in ("cb_main", "cb_left", "cb_right"):
            m = Model.new(m.positions, m.normals, m.material.textured(tex), m.matrices, m.name, uvs=planar_uvs(m.positions, repeat))
        models.append(m)
    return SceneDesc.new(models, scenes.reference_camera(W / H), f"cornell checker {n}")


def ripples(n):
    """the n x n ripple normal map of examples/headless --normal-ripples: tangent-space (0.3 tri(i), 0.3 tri(j), z) encoded 0.5 * v + 0.5"""
    f = np.float32
    a = (np.arange(n, dtype=f) + f(0.5)) / f(n)
    tri = f(0.3) * (f(4.0) * np.abs(a - f(0.5)) - f(1.0))
    x, y = np.meshgrid(tri, tri)
    z = np.sqrt((f(1.0) - x * x) - y * y)
    return f(0.5) * np.stack([x, y, z], axis=2).astype(f) + f(0.5)


def rippled_cornell(scenes, W, H, n, repeat):
    """textured_cornell's models and UVs under an n x n ripple normal map instead of the checker"""
    from path_tracer_amd.scene_desc import Model, SceneDesc, Texture
    tex = Texture.new(ripples(n))
    models = []
    for m in scenes.cornell_models():
        if m.name in ("cb_main", "cb_left", "cb_right"):
            m = Model.new(m.positions, m.normals, m.material.normal_mapped(tex), m.matrices, m.name, uvs=planar_uvs(m.positions, repeat))
        models.append(m)
    return SceneDesc.new(models, scenes.reference_camera(W / H), f"cornell ripples {n}")


def emission_cornell(scenes, W, H, n):
    """the Cornell frame with an n x n checker as the emission texture of its light, UVs planar over the light's extent"""
    from path_tracer_amd.scene_desc import Model, SceneDesc, Texture
    tex = Texture.new(checker(n))
    models = []
    for m in scenes.cornell_models():
        if m.name == "cb_light":
            m = Model.new(m.positions, m.normals, m.material.emission_textured(tex), m.matrices, m.name, uvs=planar_uvs(m.positions, 1.0))
        models.append(m)
    return SceneDesc.new(models, scenes.reference_camera(W / H), f"cornell emission checker {n}")


def roughness_checker(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    return np.repeat(np.where((i + j) & 1, np.float32(0.6), np.float32(0.1))[..., None], 3, axis=2)


def roughness_variants(scenes, W, H, repeat):
    """{name: make} of --roughness: the corner room and the mixed Cornell box in their two or three states"""
    import dataclasses
    from path_tracer_amd.scene_desc import GGX_DIELECTRIC, GGX_METAL, Material, SceneDesc, Texture
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from textures_common import corner_scene
    can = hasattr(Material, "roughness_mapped")
    rough = Texture.new(roughness_checker(8))

    def mapped(desc):
        """the roughness checker on every GGX material; a model that has no UVs yet gets planar ones (the corner room's keep their one
        corner, which the 8 x 8 map turns into one of its texels' corners: four different texels, blended)"""
        models = []
        for m in desc.models:
            if m.material.kind in (GGX_METAL, GGX_DIELECTRIC):
                m = dataclasses.replace(m, material=m.material.roughness_mapped(rough), uvs=m.uvs if m.uvs is not None else planar_uvs(m.positions, repeat))
            models.append(m)
        return SceneDesc.new(models, desc.camera, desc.name + " roughness")

    v = {"corner_plain": lambda: corner_scene(W, H)[1], "corner_tex": lambda: corner_scene(W, H)[0],
         "mixed_plain": lambda: scenes.cornell_mixed(W, H), "mixed_tex": lambda: scenes.checker_textured(scenes.cornell_mixed(W, H), repeat=repeat)}
    if can:
        v["corner_rough"] = lambda: mapped(corner_scene(W, H)[0])
        v["mixed_rough"] = lambda: mapped(scenes.checker_textured(scenes.cornell_mixed(W, H), repeat=repeat))
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeat", type=float, default=8.0)
    ap.add_argument("--only", choices=["plain", "tex8", "tex1024", "emit8", "nmap8"])
    ap.add_argument("--normal", action="store_true", help="also measure nmap8: the walls under an 8 x 8 ripple normal map")
    ap.add_argument("--emission", action="store_true", help="also measure emit8: the light on an 8 x 8 checker emission texture")
    ap.add_argument("--roughness", action="store_true", help="measure the corner room and the mixed box plain, textured and roughness-mapped instead")
    ap.add_argument("--out")
    a = ap.parse_args()
    from path_tracer_amd import api, scenes
    W, H = a.width, a.height
    variants = {"plain": lambda: scenes.cornell_box(W, H), "tex8": lambda: textured_cornell(scenes, W, H, 8, a.repeat),
                "tex1024": lambda: textured_cornell(scenes, W, H, 1024, a.repeat)}
    if a.emission or a.only == "emit8":
        variants["emit8"] = lambda: emission_cornell(scenes, W, H, 8)
    if a.normal or a.only == "nmap8":
        variants["nmap8"] = lambda: rippled_cornell(scenes, W, H, 8, a.repeat)
    if a.only:
        variants = {a.only: variants[a.only]}
    if a.roughness:
        variants = roughness_variants(scenes, W, H, a.repeat)
    rs = {}
    for name, make in variants.items():
        r = api.Renderer(make(), W, H, max_bounces=a.bounces)
        r.render_device(0, a.spp)          # warm-up: code objects, buffers, the scene upload
        r.synchronize()
        rs[name] = r
    times = {name: [] for name in rs}
    for rep in range(a.reps):              # interleaved: whatever else the machine does falls on all of them
        for name, r in rs.items():
            r.reset_accumulation()
            r.synchronize()
            t0 = time.perf_counter()
            r.render_device(0, a.spp)
            r.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    res = dict(width=W, height=H, spp=a.spp, bounces=a.bounces, reps=a.reps, variants={})
    for name, r in rs.items():
        t = times[name]
        st = r.stats()
        res["variants"][name] = dict(ms_per_frame=float(np.median(t)) if t else None, ms_min=min(t) if t else None, ms_max=max(t) if t else None, ms_all=t,
                                     scene_bytes=int(r.scene_info().scene_bytes), rays_any=int(st.rays_any))
    if "plain" in rs and a.reps:
        for name in rs:
            if name != "plain":
                res[name + "_over_plain"] = res["variants"][name]["ms_per_frame"] / res["variants"]["plain"]["ms_per_frame"]
    if "nmap8" in rs and "tex8" in rs and a.reps:
        res["nmap8_over_tex8"] = res["variants"]["nmap8"]["ms_per_frame"] / res["variants"]["tex8"]["ms_per_frame"]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
