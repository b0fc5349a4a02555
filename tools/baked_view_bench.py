#!/usr/bin/env python3
"""What a baked view costs (profiles/r22_baked_view.md): on the 1080p Cornell frame with a 256 x 256 map on every placement, milliseconds per
pt_render_baked(1 sample) at K = 0 and K = 2, beside pt_render_guides_followed at the same K (the same rays and traces, another ending) and
the 1-spp pt_frame.  Every figure is the median of --calls blocking calls, taken --reps times with the routes alternating, so that a drift
of the shared machine touches all of them; the report keeps every repeat, the spread is theirs.

    python tools/baked_view_bench.py [--calls 20] [--reps 3] [--what all|guides] [--probes [--depth R] [--radiance R [--views-only] [--roughness-checker N]]] [--directional] [--endings] [--out report.json]

--what guides times the guides call alone and runs on a tree that has no baked view: run it from the parent commit's tree and from this one,
turn about, for the comparison across the two (the guide kernels themselves must not have moved).

--probes (profiles/r24_probe_grid.md) times the probe ending instead: no map anywhere, so that a 16 x 16 x 16 probe grid over the scene's
bounds is the only light source of every final surface, ms per pt_render_baked(1 sample) at K = 0 and K = 2 with the grid beside the same
calls on a context without one; and pt_probe_backfaces for 4 096 probes x 256 samples beside pt_bake_probes of the same shape.

--probes --depth R (profiles/r25_probe_depth.md) adds probe visibility: a third context whose grid carries a seeded R x R depth table (FACING
on), its pt_render_baked beside the two others; pt_bake_probe_depth beside pt_probe_backfaces on 4 096 probes x 1 024 rays (the same trace
plus one fold each); and pt_probe_grid_lookup(on_device) with and without depth on 2^20 points (blocking calls: both include the same
staging copies of 28 MiB).

--probes --radiance R (profiles/r27_probe_radiance.md) adds reflection probes: both boxes of the scene become GGX metal (roughness 0.4) in
every context of the run, a further context's grid carries a seeded R x R radiance table of five levels, its pt_render_baked beside the
grid's alone; pt_bake_probe_radiance beside pt_bake_probes on 4 096 probes x 1 024 rays (the same integration, another fold);
pt_probe_radiance_prefilter(on_device) of 4 096 probes x 5 levels at R = 8 and R = 16 (blocking calls: staging copies included; the
profile quotes the kernel alone from a kernel trace beside them); and pt_probe_grid_specular(on_device) beside pt_probe_grid_lookup on 2^20 points.

--probes --radiance R --views-only [--roughness-checker N] (profiles/r33_roughness_maps.md) keeps the pt_render_baked routes of that run alone, and
with --roughness-checker adds a context whose two metal boxes carry an N x N roughness checker of 0.1 / 0.6 under planar UVs (a textured scene:
pt_set_material_roughness_texture), its pt_render_baked beside the unmapped metal's: what reading the alpha at the hit costs the SPEC ending.

--directional (profiles/r29_directional_lightmaps.md) times the DIR endings: every Lambertian material of the scene carries an 8 x 8 ripple
normal map, every placement a 256 x 256 map; one context stops there (the scalar kernels), a second also sets a seeded gradient on every
placement (the DIR kernels): ms per pt_render_baked(1 sample) at K = 0 and K = 2 on both, turn about; and pt_bake_lightmap_directional beside
pt_bake_lightmap on the shell's 256 x 256 map at 16 samples (the same integration, another fold, 36 more bytes per texel each way).

--endings (profiles/r30_baked_axes.md) times every ending of the baked view, one context after the other: the rippled scene of --directional
with both boxes GGX metal, a 256 x 256 map on the shell's placement only (the grid lights the other walls), and the axes switched on one by
one: the 16 x 16 x 16 grid, its R = 8 depth table, its R = 8 radiance table, the gradient: ms per pt_render_baked(1 sample) at K = 0 and K = 2
for the ten points of (grid, vis, spec, dir) that are kernels, and the SHA-1 of the sums the timed calls of each left (two builds that compute
the same bits report the same digests)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DEPTH, SIZE = 1920, 1080, 8, 256
HOPS = (0, 2)


def planar_uvs(positions):
    """UVs [n, 3, 2] over the two axes a model extends furthest along, each over the model's own extent: a layout for timing, not for baking"""
    p = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    ax = sorted(np.argsort(hi - lo)[1:])
    return ((p[:, :, ax] - lo[ax]) / np.maximum(hi[ax] - lo[ax], 1e-9)).astype(np.float32)


def timed(fn, calls):
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()                                  # blocking: the call has synchronised its stream when it returns
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--what", choices=["all", "guides"], default="all")
    ap.add_argument("--probes", action="store_true")
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--radiance", type=int, default=0)
    ap.add_argument("--views-only", action="store_true", help="with --probes: time the pt_render_baked routes alone")
    ap.add_argument("--roughness-checker", type=int, default=0, help="with --probes --radiance: also the metal boxes under an N x N roughness checker")
    ap.add_argument("--directional", action="store_true")
    ap.add_argument("--endings", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("baked_view_bench needs the GPU: there is nothing to time without one")
    from path_tracer_amd import api, scenes
    if args.probes:
        return probes(args, api, scenes)
    if args.directional:
        return directional(args, api, scenes)
    if args.endings:
        return endings(args, api, scenes)
    sc = scenes.cornell_box(W, H)
    baked = args.what == "all"
    if baked:
        for m in sc.models:
            m.uvs = planar_uvs(m.positions)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    report = {"width": W, "height": H, "map": SIZE, "calls": args.calls, "what": args.what, "guides_ms": {str(k): [] for k in HOPS}}
    if baked:
        rng = np.random.default_rng(22)
        for mi, m in enumerate(sc.models):
            for j in range(m.matrices.shape[0]):
                r.set_lightmap(mi, j, rng.uniform(0.0, 1.0, (SIZE, SIZE, 3)).astype(np.float32))
        report.update(baked_ms={str(k): [] for k in HOPS}, frame_ms=[])
    routes = []
    sample = [0]

    def guides(k):
        sample[0] += 1
        r.render_guides(sample[0], follow=k)

    def view(k):
        sample[0] += 1
        r.render_baked(sample[0], 1, follow=k, download=False)
    last = [r.inv_projection()]

    def frame():
        sample[0] += 1
        r.frame(sample[0], last[0], download=False)
        last[0] = r.inv_projection()
    for k in HOPS:
        routes.append((report["guides_ms"][str(k)], lambda k=k: guides(k)))
        if baked:
            routes.append((report["baked_ms"][str(k)], lambda k=k: view(k)))
    if baked:
        routes.append((report["frame_ms"], frame))
    for _, fn in routes:                      # warm-up: scene and map upload, code objects, the scratch at the size the timed calls use
        fn()
    for _ in range(args.reps):
        for into, fn in routes:
            into.append(round(timed(fn, args.calls), 4))
    emit(report, args.out)


def emit(report, out):
    line = json.dumps(report)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


GRID, CENSUS_PROBES, CENSUS_SAMPLES = 16, 4096, 256
DEPTH_SAMPLES, LOOKUPS = 1024, 1 << 20


def probes(args, api, scenes):
    sc = scenes.cornell_box(W, H)
    if args.radiance:
        from path_tracer_amd.scene_desc import GGX, SceneDesc
        metal = GGX.new_metal((0.9, 0.8, 0.6), 0.4)
        sc = SceneDesc.new(scenes.cornell_models(tall_material=metal, short_material=metal), sc.camera, "cornell, metal boxes")
    bare, lit = api.Renderer(sc, W, H, max_bounces=DEPTH), api.Renderer(sc, W, H, max_bounces=DEPTH)
    pts = np.concatenate([(m.positions.reshape(-1, 3) @ mat[:, :3].T + mat[:, 3]) for m in sc.models for mat in m.matrices.astype(np.float64)])
    lo, hi = pts.min(0), pts.max(0)
    cell = (hi - lo) / GRID
    rng = np.random.default_rng(24)
    sh = rng.uniform(-0.2, 0.2, (GRID, GRID, GRID, 9, 3)).astype(np.float32)
    sh[..., 0, :] = rng.uniform(1.0, 3.0, (GRID, GRID, GRID, 3)).astype(np.float32)
    lit.set_probe_grid(lo + 0.5 * cell, cell, sh, normal_bias=0.01 * float(cell.min()))
    pos = (lo + rng.uniform(0.0, 1.0, (CENSUS_PROBES, 3)) * (hi - lo)).astype(np.float32)
    report = {"width": W, "height": H, "grid": GRID, "calls": args.calls, "what": "probes", "baked_ms": {str(k): [] for k in HOPS},
              "baked_probes_ms": {str(k): [] for k in HOPS}, "census": [CENSUS_PROBES, CENSUS_SAMPLES], "backfaces_ms": [], "bake_probes_ms": []}
    sample = [0]

    def view(r, k):
        sample[0] += 1
        r.render_baked(sample[0], 1, follow=k, unlit=(0.5, 0.5, 0.5), download=False)
    routes = []
    for k in HOPS:
        routes.append((report["baked_ms"][str(k)], lambda k=k: view(bare, k), args.calls))
        routes.append((report["baked_probes_ms"][str(k)], lambda k=k: view(lit, k), args.calls))
    routes.append((report["backfaces_ms"], lambda: bare.probe_backfaces(pos, CENSUS_SAMPLES), 3))
    routes.append((report["bake_probes_ms"], lambda: bare.bake_probes(pos, CENSUS_SAMPLES), 3))
    if args.depth:
        R = args.depth
        vis = api.Renderer(sc, W, H, max_bounces=DEPTH)
        vis.set_probe_grid(lo + 0.5 * cell, cell, sh, normal_bias=0.01 * float(cell.min()))
        reach = float(np.linalg.norm(cell))
        m1 = rng.uniform(0.3, 1.5, (GRID ** 3, R * R)).astype(np.float32) * np.float32(reach)
        m2 = m1 * m1 + (rng.uniform(0.0, 0.3, m1.shape).astype(np.float32) * np.float32(reach)) ** 2
        vis.set_probe_grid_depth(np.stack([m1, m2], axis=-1), 0.0, True)
        far = 1.5 * reach
        q = (lo + rng.uniform(0.0, 1.0, (LOOKUPS, 3)) * (hi - lo)).astype(np.float32)
        qn = rng.normal(size=(LOOKUPS, 3))
        qn = (qn / np.linalg.norm(qn, axis=1, keepdims=True)).astype(np.float32)
        report.update(depth=R, baked_probes_depth_ms={str(k): [] for k in HOPS}, depth_census=[CENSUS_PROBES, DEPTH_SAMPLES], backfaces_1024_ms=[],
                      bake_probe_depth_ms=[], lookups=LOOKUPS, lookup_ms=[], lookup_depth_ms=[])
        for k in HOPS:
            routes.append((report["baked_probes_depth_ms"][str(k)], lambda k=k: view(vis, k), args.calls))
        routes.append((report["backfaces_1024_ms"], lambda: bare.probe_backfaces(pos, DEPTH_SAMPLES), 3))
        routes.append((report["bake_probe_depth_ms"], lambda: bare.bake_probe_depth(pos, DEPTH_SAMPLES, R, far), 3))
        routes.append((report["lookup_ms"], lambda: lit.probe_grid_lookup(q, qn, on_device=True), 5))
        routes.append((report["lookup_depth_ms"], lambda: vis.probe_grid_lookup(q, qn, on_device=True), 5))
    if args.radiance:
        R = args.radiance
        alphas = (0.1, 0.2, 0.4, 0.7, 1.0)
        spec = api.Renderer(sc, W, H, max_bounces=DEPTH)
        spec.set_probe_grid(lo + 0.5 * cell, cell, sh, normal_bias=0.01 * float(cell.min()))
        table = rng.uniform(0.0, 2.0, (GRID ** 3, len(alphas), R * R, 4)).astype(np.float32)
        table[..., 3] = 0.0
        spec.set_probe_grid_radiance(table, alphas)
        q = (lo + rng.uniform(0.0, 1.0, (LOOKUPS, 3)) * (hi - lo)).astype(np.float32)
        qn = rng.normal(size=(LOOKUPS, 3)); qd = rng.normal(size=(LOOKUPS, 3))
        qn = (qn / np.linalg.norm(qn, axis=1, keepdims=True)).astype(np.float32)
        qd = (qd / np.linalg.norm(qd, axis=1, keepdims=True)).astype(np.float32)
        qa = rng.uniform(0.0, 1.0, LOOKUPS).astype(np.float32)
        raw = {}
        for side in (8, 16):
            counts = rng.integers(0, 12, (CENSUS_PROBES, side * side)).astype(np.uint32)
            raw[side] = ((rng.uniform(0.0, 3.0, (CENSUS_PROBES, side * side, 3)) * counts[..., None]).astype(np.float32), counts)
        report.update(radiance=R, baked_probes_radiance_ms={str(k): [] for k in HOPS}, radiance_census=[CENSUS_PROBES, DEPTH_SAMPLES], bake_probes_1024_ms=[],
                      bake_probe_radiance_ms=[], prefilter_ms={"8": [], "16": []}, lookups=LOOKUPS, lookup_specular_ms=[])
        report.setdefault("lookup_ms", [])
        for k in HOPS:
            routes.append((report["baked_probes_radiance_ms"][str(k)], lambda k=k: view(spec, k), args.calls))
        if args.roughness_checker:
            import dataclasses
            from path_tracer_amd.scene_desc import GGX_METAL, Texture
            n = args.roughness_checker
            ci, cj = np.meshgrid(np.arange(n), np.arange(n))
            checker = Texture.new(np.repeat(np.where((ci + cj) & 1, np.float32(0.6), np.float32(0.1))[..., None], 3, axis=2))
            mapped = SceneDesc.new([dataclasses.replace(m, material=m.material.roughness_mapped(checker), uvs=planar_uvs(m.positions))
                                    if m.material.kind == GGX_METAL else m for m in sc.models], sc.camera, "cornell, roughness-mapped metal boxes")
            rough = api.Renderer(mapped, W, H, max_bounces=DEPTH)
            rough.set_probe_grid(lo + 0.5 * cell, cell, sh, normal_bias=0.01 * float(cell.min()))
            rough.set_probe_grid_radiance(table, alphas)
            report.update(roughness_checker=n, baked_probes_radiance_rough_ms={str(k): [] for k in HOPS})
            for k in HOPS:
                routes.append((report["baked_probes_radiance_rough_ms"][str(k)], lambda k=k: view(rough, k), args.calls))
        routes.append((report["bake_probes_1024_ms"], lambda: bare.bake_probes(pos, DEPTH_SAMPLES), 3))
        routes.append((report["bake_probe_radiance_ms"], lambda: bare.bake_probe_radiance(pos, DEPTH_SAMPLES, R), 3))
        for side in (8, 16):
            routes.append((report["prefilter_ms"][str(side)], lambda side=side: bare.probe_radiance_prefilter(*raw[side], alphas, on_device=True), 5))
        if not args.depth:
            routes.append((report["lookup_ms"], lambda: lit.probe_grid_lookup(q, qn, on_device=True), 5))
        routes.append((report["lookup_specular_ms"], lambda: spec.probe_grid_specular(q, qn, qd, qa, on_device=True), 5))
    if args.views_only:
        routes = [rt for rt in routes if rt[2] == args.calls]
    for _, fn, _ in routes:
        fn()
    for _ in range(args.reps):
        for into, fn, calls in routes:
            into.append(round(timed(fn, calls), 4))
    emit(report, args.out)


BAKE_SAMPLES = 16


def rippled(scenes, **materials):
    """the Cornell box with every Lambertian material under an 8 x 8 ripple normal map and planar UVs on every model"""
    import dataclasses
    from path_tracer_amd.scene_desc import LAMBERTIAN, SceneDesc, Texture
    n = 8
    a = (np.arange(n, dtype=np.float32) + 0.5) / n
    tri = 0.3 * (4.0 * np.abs(a - 0.5) - 1.0)
    x, y = np.meshgrid(tri, tri)
    ripples = Texture.new((0.5 * np.stack([x, y, np.sqrt(1.0 - x * x - y * y)], axis=2) + 0.5).astype(np.float32))
    models = [dataclasses.replace(m, material=m.material.normal_mapped(ripples) if m.material.kind == LAMBERTIAN else m.material, uvs=planar_uvs(m.positions))
              for m in scenes.cornell_models(**materials)]
    return SceneDesc.new(models, scenes.cornell_box(W, H).camera, "cornell, rippled")


def directional(args, api, scenes):
    sc = rippled(scenes)
    plain, dirn = api.Renderer(sc, W, H, max_bounces=DEPTH), api.Renderer(sc, W, H, max_bounces=DEPTH)
    rng = np.random.default_rng(29)
    for mi, m in enumerate(sc.models):
        for j in range(m.matrices.shape[0]):
            tex = rng.uniform(0.0, 1.0, (SIZE, SIZE, 3)).astype(np.float32)
            plain.set_lightmap(mi, j, tex)
            dirn.set_lightmap(mi, j, tex)
            dirn.set_lightmap_directional(mi, j, rng.uniform(-0.5, 0.5, (SIZE, SIZE, 3, 3)).astype(np.float32))
    shell = [m.name for m in sc.models].index("cb_main")
    report = {"width": W, "height": H, "map": SIZE, "calls": args.calls, "what": "directional", "baked_ms": {str(k): [] for k in HOPS},
              "baked_directional_ms": {str(k): [] for k in HOPS}, "bake": [SIZE, SIZE, BAKE_SAMPLES], "bake_lightmap_ms": [], "bake_lightmap_directional_ms": []}
    sample = [0]

    def view(r, k):
        sample[0] += 1
        r.render_baked(sample[0], 1, follow=k, download=False)
    routes = []
    for k in HOPS:
        routes.append((report["baked_ms"][str(k)], lambda k=k: view(plain, k), args.calls))
        routes.append((report["baked_directional_ms"][str(k)], lambda k=k: view(dirn, k), args.calls))
    routes.append((report["bake_lightmap_ms"], lambda: plain.bake_lightmap(shell, 0, SIZE, SIZE, BAKE_SAMPLES, bias=0.25), 3))
    routes.append((report["bake_lightmap_directional_ms"], lambda: plain.bake_lightmap_directional(shell, 0, SIZE, SIZE, BAKE_SAMPLES, bias=0.25), 3))
    for _, fn, _ in routes:
        fn()
    for _ in range(args.reps):
        for into, fn, calls in routes:
            into.append(round(timed(fn, calls), 4))
    emit(report, args.out)


def endings(args, api, scenes):
    from path_tracer_amd.scene_desc import GGX
    metal = GGX.new_metal((0.9, 0.8, 0.6), 0.4)
    sc = rippled(scenes, tall_material=metal, short_material=metal)
    pts = np.concatenate([(m.positions.reshape(-1, 3) @ mat[:, :3].T + mat[:, 3]) for m in sc.models for mat in m.matrices.astype(np.float64)])
    lo, hi = pts.min(0), pts.max(0)
    cell = (hi - lo) / GRID
    rng = np.random.default_rng(30)
    sh = rng.uniform(-0.2, 0.2, (GRID, GRID, GRID, 9, 3)).astype(np.float32)
    sh[..., 0, :] = rng.uniform(1.0, 3.0, (GRID, GRID, GRID, 3)).astype(np.float32)
    reach, R, alphas = float(np.linalg.norm(cell)), 8, (0.1, 0.2, 0.4, 0.7, 1.0)
    m1 = rng.uniform(0.3, 1.5, (GRID ** 3, R * R)).astype(np.float32) * np.float32(reach)
    m2 = m1 * m1 + (rng.uniform(0.0, 0.3, m1.shape).astype(np.float32) * np.float32(reach)) ** 2
    table = rng.uniform(0.0, 2.0, (GRID ** 3, len(alphas), R * R, 4)).astype(np.float32)
    table[..., 3] = 0.0
    shell = [m.name for m in sc.models].index("cb_main")
    tex, grad = rng.uniform(0.0, 1.0, (SIZE, SIZE, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (SIZE, SIZE, 3, 3)).astype(np.float32)
    report = {"width": W, "height": H, "map": SIZE, "grid": GRID, "calls": args.calls, "what": "endings", "baked_ms": {}, "baked_sha1": {}}
    for grid, vis, spec, dirn in [(g, v, s, d) for d in (0, 1) for g in (0, 1) for v in (0, 1) for s in (0, 1) if g or not (v or s)]:
        r = api.Renderer(sc, W, H, max_bounces=DEPTH)
        r.set_lightmap(shell, 0, tex)
        if dirn:
            r.set_lightmap_directional(shell, 0, grad)
        if grid:
            r.set_probe_grid(lo + 0.5 * cell, cell, sh, normal_bias=0.01 * float(cell.min()))
        if vis:
            r.set_probe_grid_depth(np.stack([m1, m2], axis=-1), 0.0, True)
        if spec:
            r.set_probe_grid_radiance(table, alphas)
        for k in HOPS:
            view = lambda n, k=k: r.render_baked(n, 1, follow=k, unlit=(0.5, 0.5, 0.5), download=False)
            view(0)
            ms = report["baked_ms"][f"grid {grid} vis {vis} spec {spec} dir {dirn}, K = {k}"] = []
            for rep in range(args.reps):
                ms.append(round(timed(lambda: view(1 + rep), args.calls), 4))
            report["baked_sha1"][f"grid {grid} vis {vis} spec {spec} dir {dirn}, K = {k}"] = hashlib.sha1(r.read_baked().tobytes()).hexdigest()
        del r
    emit(report, args.out)


if __name__ == "__main__":
    main()
