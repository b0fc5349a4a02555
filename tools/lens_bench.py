"""Thin-lens record (profiles/r09_lens.md): what depth of field costs.  The same Cornell frame with the pinhole camera and under a lens, same
build, same process: wall clock of the blocking pt_render_device per frame (median of --reps, after a warm-up frame of each) and the active
rectangle of each.

    python tools/lens_bench.py [--width 1920 --height 1080 --spp 256 --bounces 8 --aperture 40 --focus 950 --reps 5] [--out file.json]
    python tools/lens_bench.py --only lens --reps 1      one variant alone, e.g. under rocprofv3 --kernel-trace --stats for the per-kernel table
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
    ap.add_argument("--aperture", type=float, default=40.0)
    ap.add_argument("--focus", type=float, default=950.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["pinhole", "lens"])
    ap.add_argument("--out")
    a = ap.parse_args()
    from path_tracer_amd import api, scenes
    W, H = a.width, a.height
    variants = {"pinhole": (0.0, a.focus), "lens": (a.aperture, a.focus)}
    if a.only:
        variants = {a.only: variants[a.only]}
    rs = {}
    for name, lens in variants.items():
        r = api.Renderer(scenes.cornell_box(W, H), W, H, max_bounces=a.bounces)
        r.set_lens(*lens)
        r.render_device(0, a.spp)          # warm-up: code objects, buffers, the scene upload
        r.synchronize()
        rs[name] = r
    times = {name: [] for name in rs}
    for rep in range(a.reps):              # interleaved: whatever else the machine does falls on both
        for name, r in rs.items():
            r.reset_accumulation()
            r.synchronize()
            t0 = time.perf_counter()
            r.render_device(0, a.spp)
            r.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    res = dict(width=W, height=H, spp=a.spp, bounces=a.bounces, reps=a.reps, variants={})
    for name, r in rs.items():
        rect, _ = r.active_pixels()
        t = times[name]
        res["variants"][name] = dict(aperture=variants[name][0], focus=variants[name][1], rect=rect, share=rect[1] * rect[3] / (W * H),
                                     ms_per_frame=float(np.median(t)) if t else None, ms_min=min(t) if t else None, ms_max=max(t) if t else None)
    if len(rs) == 2 and a.reps:
        res["lens_over_pinhole"] = res["variants"]["lens"]["ms_per_frame"] / res["variants"]["pinhole"]["ms_per_frame"]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
