"""Projection record (profiles/r14_projections.md): what a panoramic or orthographic frame costs.  The Cornell frame under the perspective camera
(the reference's pose), a full panorama from inside the room (eye 0 50 100, spans 360 x 180) and an orthographic view (the reference's pose, view
volume 600 high), same build, same process: wall clock of the blocking pt_render_device per frame (median of --reps, interleaved, after a warm-up
frame of each), pt_stats' ray tallies of one frame, and from them the cost per traced ray (a projected frame has no primary cull, so frames
differ in how many rays they trace).  The generate kernels' own time comes from FLAG_TIMING's ms_generate of one more frame.

    python tools/projection_bench.py [--width 1920 --height 1080 --spp 256 --bounces 8 --reps 5] [--out file.json]
    python tools/projection_bench.py --only panorama --reps 1     one variant alone, e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["perspective", "panorama", "ortho"])
    ap.add_argument("--out")
    a = ap.parse_args()
    from path_tracer_amd import api, scenes
    from path_tracer_amd.scene_desc import Camera, SceneDesc
    W, H = a.width, a.height
    base = scenes.cornell_box(W, H)
    inside = SceneDesc.new(base.models, Camera.new((0.0, 50.0, 100.0), (0.0, 50.0, 0.0), 60.0, W / H), base.name)
    variants = {"perspective": (base, (api.PROJ_PERSPECTIVE, 0.0, 0.0, 0.0)), "panorama": (inside, (api.PROJ_PANORAMA, 360.0, 180.0, 0.0)),
                "ortho": (base, (api.PROJ_ORTHOGRAPHIC, 0.0, 0.0, 600.0))}
    if a.only:
        variants = {a.only: variants[a.only]}
    rs = {}
    for name, (sc, proj) in variants.items():
        r = api.Renderer(sc, W, H, max_bounces=a.bounces)
        r.set_projection(*proj)
        r.render_device(0, a.spp)          # warm-up: code objects, buffers, the scene upload
        r.synchronize()
        rs[name] = r
    times = {name: [] for name in rs}
    for rep in range(a.reps):              # interleaved: whatever else the machine does falls on all
        for name, r in rs.items():
            r.reset_accumulation()
            r.synchronize()
            t0 = time.perf_counter()
            r.render_device(0, a.spp)
            r.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    res = dict(width=W, height=H, spp=a.spp, bounces=a.bounces, reps=a.reps, variants={})
    for name, r in rs.items():
        # one frame's tallies, and the generate kernels' own time (per-kernel events serialise the pipelines: not a frame time)
        r.reset_stats(); r.reset_accumulation()
        r.render_device(0, a.spp); r.synchronize()
        st = r.stats()
        r.set_config(flags=api.FLAG_TIMING)
        r.reset_stats(); r.reset_accumulation()
        r.render_device(0, a.spp); r.synchronize()
        timed = r.stats()
        rect, _ = r.active_pixels()
        t = times[name]
        ms = float(np.median(t)) if t else None
        res["variants"][name] = dict(projection=list(variants[name][1]), rect=rect, share=rect[1] * rect[3] / (W * H), ms_per_frame=ms,
                                     ms_min=min(t) if t else None, ms_max=max(t) if t else None, paths=st.paths, rays_closest=st.rays_closest,
                                     rays_any=st.rays_any, rays_light_closest=st.rays_light_closest, rays_primary_culled=st.rays_primary_culled,
                                     rays=st.rays, ns_per_ray=1e6 * ms / st.rays if t and st.rays else None, ms_generate=timed.ms_generate,
                                     ms_accumulate=timed.ms_accumulate)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
