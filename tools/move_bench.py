#!/usr/bin/env python3
"""What moving an instance costs (profiles/r11_moving_instances.md): per scene, host ms of pt_set_instances + pt_build, and ms until the next
1-spp pt_frame_moving has returned — beside the only route a library without pt_set_instances offers: a new context, every model added again,
pt_build, first frame.  The fresh route goes through a minimal ctypes binding of its own, so that --fresh-lib can name a libptmi.so built from
an older commit and both routes are timed in one session on one device.

    python tools/move_bench.py [--scenes cornell,cornell_instanced,atrium,atrium_all,mesh328k] [--moves 20] [--fresh 3] [--fresh-lib PATH]
                               [--frames 200] [--out report.json]

Also times the 1080p 1-spp Cornell loop with pt_frame and with pt_frame_moving on a scene nobody moves (the guide trace plus, when something
moved, one elementwise pass).  PTMI_DEBUG_BUILD=1 is set around ONE atrium rebuild: the builder's stage times appear on stderr."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DEPTH = 1920, 1080, 8


def scene_and_moves(name):
    """(scene description, [model indices that move]); a move k shifts every instance of those models by (k + 1, 0, 0) from where it started"""
    from path_tracer_amd import scenes
    if name == "cornell":
        return scenes.cornell_box(W, H), [5]
    if name == "cornell_instanced":
        return scenes.cornell_instanced(W, H), [4]
    if name == "atrium":
        return scenes.atrium(W, H), [7]                  # one column is one matrix of model 7; the call replaces the model's list
    if name == "atrium_all":
        return scenes.atrium(W, H), [7, 8, 9, 10]        # all 72 columns (and the three toppled ones)
    if name == "mesh328k":
        sc = scenes.cornell_mesh(W, H, level=7)
        return sc, [max(range(len(sc.models)), key=lambda i: sc.models[i].positions.shape[0])]
    raise SystemExit(f"unknown scene {name}")


def moved(desc, models, k, one_only):
    out = []
    for mi in models:
        m = desc.models[mi].matrices.copy()
        if one_only:
            m[0, 0, 3] += np.float32(k + 1)
        else:
            m[:, 0, 3] += np.float32(k + 1)
        out.append((mi, m))
    return out


def move_route(api, desc, models, n_moves, one_only):
    r = api.Renderer(desc, W, H, max_bounces=DEPTH)
    last = r.inv_projection()
    r.frame_moving(0, last, download=False)
    r.frame_moving(1, last, download=False)
    build_ms, total_ms = [], []
    for k in range(n_moves):
        step = moved(desc, models, k, one_only)
        t0 = time.perf_counter()
        for mi, m in step:
            r.set_instances(mi, m)
        r.rebuild()
        t1 = time.perf_counter()
        r.frame_moving(2 + k, last, download=False)
        t2 = time.perf_counter()
        build_ms.append(1e3 * (t1 - t0)); total_ms.append(1e3 * (t2 - t0))
    info = r.scene_info().as_dict()
    r.close()
    return dict(set_and_build_ms=statistics.median(build_ms), until_frame_ms=statistics.median(total_ms), frame_ms=statistics.median(
        [b - a for a, b in zip(build_ms, total_ms)]), scene_info=info)


def fresh_route(api, L, desc, n):
    """pt_create, every material and model again, pt_build, pt_set_camera, pt_frame(0): only entry points every libptmi has"""
    vp = C.c_void_p
    L.pt_create.restype = vp
    mats = desc.materials()
    build_ms, total_ms = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        cfg = api.Config(W, H, DEPTH, 512, 1, api.DEFAULT_SEED, 0, 1, 4, 0, -1, 0, 0, 0, 0, 0)
        ctx = vp(L.pt_create(C.byref(cfg)))
        assert ctx
        for m in mats:
            d = api.MaterialDesc()
            d.kind = m.kind
            d.colour[:] = m.colour
            d.roughness, d.ior = m.roughness, m.ior
            if m.volume is not None:
                d.has_volume = 1
                d.vol_absorption[:] = m.volume.absorption
                d.vol_k, d.vol_c, d.vol_g = m.volume.k, m.volume.c, m.volume.g
            assert L.pt_add_material(ctx, C.byref(d)) >= 0
        p = lambda a: a.ctypes.data_as(vp)
        for mod in desc.models:
            assert L.pt_add_model(ctx, p(mod.positions), p(mod.normals), C.c_uint32(mod.positions.shape[0]), C.c_int(mats.index(mod.material)),
                                  p(mod.matrices), C.c_uint32(mod.matrices.shape[0])) >= 0
        assert L.pt_build(ctx) == 0
        t1 = time.perf_counter()
        cam = desc.camera
        eye = (C.c_float * 3)(*cam.origin); tgt = (C.c_float * 3)(*cam.target)
        assert L.pt_set_camera(ctx, eye, tgt, C.c_float(cam.fov), C.c_float(cam.aspect_ratio)) == 0
        assert L.pt_frame(ctx, C.c_uint32(0), None, None, None, None) == 0
        t2 = time.perf_counter()
        L.pt_destroy(ctx)
        build_ms.append(1e3 * (t1 - t0)); total_ms.append(1e3 * (t2 - t0))
    return dict(create_add_build_ms=statistics.median(build_ms), until_frame_ms=statistics.median(total_ms))


def frame_loop(api, frames):
    from path_tracer_amd import scenes
    out = {}
    for which in ("frame", "frame_moving"):
        r = api.Renderer(scenes.cornell_box(W, H), W, H, max_bounces=DEPTH)
        last = r.inv_projection()
        call = getattr(r, which)
        for k in range(8):
            call(k, last, download=False)
        t0 = time.perf_counter()
        for k in range(frames):
            call(8 + k, last, download=False)
        out[which + "_ms"] = 1e3 * (time.perf_counter() - t0) / frames
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,cornell_instanced,atrium,atrium_all,mesh328k")
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--fresh", type=int, default=3)
    ap.add_argument("--fresh-lib", default="")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from path_tracer_amd import api
    api.lib()
    fresh_lib = C.CDLL(a.fresh_lib) if a.fresh_lib else C.CDLL(api._build.LIB_PATH)
    report = {"width": W, "height": H, "max_bounces": DEPTH, "fresh_lib": a.fresh_lib or "in-tree", "scenes": {}}
    for name in [s for s in a.scenes.split(",") if s]:
        desc, models = scene_and_moves(name)
        if name == "atrium":
            os.environ["PTMI_DEBUG_BUILD"] = "1"
            probe = api.Renderer(desc, 64, 36)
            probe.set_instances(7, desc.models[7].matrices)
            probe.rebuild()                                   # stage times of an incremental atrium build on stderr
            probe.close()
            del os.environ["PTMI_DEBUG_BUILD"]
        row = {"instances": int(sum(len(m.matrices) for m in desc.models)), "triangles": int(sum(m.positions.shape[0] for m in desc.models)),
               "move": move_route(api, desc, models, a.moves, one_only=(name == "atrium")), "fresh": fresh_route(api, fresh_lib, desc, a.fresh)}
        report["scenes"][name] = row
        print(json.dumps({name: row}), flush=True)
    if a.frames:
        report["cornell_1spp_loop"] = frame_loop(api, a.frames)
        print(json.dumps({"cornell_1spp_loop": report["cornell_1spp_loop"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
