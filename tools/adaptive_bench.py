"""Adaptive sampling (PT_FLAG_ADAPTIVE) against uniform sampling at equal error, and the cost of the adaptive path itself.

For each configuration (bench.py's cornell and mixed geometry, size and depth):
  * a reference: the configuration's own spp with ANOTHER seed (independent of the renders it judges);
  * uniform N spp: wall time, paths traced, RMSE of the per-pixel mean rgb against the reference;
  * adaptive rounds for a sweep of rel_error values (min_samples, then rounds that add `--growth` times the selected pixels' count — a
    pixel once converged stays converged, so every selected pixel holds the same count — until no pixel is selected or the cap is
    reached): wall time of the pt_render_adaptive calls, paths traced, RMSE after each round.  The first round of a run that reaches the
    uniform RMSE is that run's equal-RMSE point; the cheapest over the sweep is reported.
Then the overhead of pt_render_adaptive with every pixel selected (rel_error 0, min_samples 2^24) against pt_render_device at 256 spp on
the Cornell 1080p frame, and of keeping the moments (the flag) on plain pt_render_device; once as is (the list traces the camera rays of
pixels the active rectangle answers without a ray) and once with PT_FLAG_NO_PRIMARY_CULL on both sides (the same rays).

Every timed call or schedule runs once untimed first, on a context with one pipeline (whose pool only ever grows), so that no timed
call reallocates a pool: a request that needs a larger pool than the context holds pays hipMalloc (seconds for tens of GiB),
and an adaptive schedule changes its request size from round to round.

usage: python tools/adaptive_bench.py [--configs cornell,mixed] [--uniform 256] [--out FILE.json]
Prints one JSON object per measurement line and a summary at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from path_tracer_amd import api, scenes  # noqa: E402

CONFIGS = {  # bench.py's geometry: scene, width, height, the configuration's own spp (reference), depth
    "cornell": ("cornell_box", 1920, 1080, 4096, 8),
    "mixed": ("cornell_mixed", 4096, 4096, 4096, 16),
}


def mean_rgb(acc):
    return acc[..., :3].astype(np.float64) / np.maximum(acc[..., 3:4].astype(np.float64), 1.0)


def rmse(acc, ref_mean):
    return float(np.sqrt(np.mean((mean_rgb(acc) - ref_mean) ** 2)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def emit(rec):
    print(json.dumps(rec), flush=True)
    return rec


def run_config(name, uniform_spp, rels, growth, min_samples, cap_factor, records):
    scene_fn, w, h, ref_spp, depth = CONFIGS[name]
    sc = getattr(scenes, scene_fn)(w, h)
    ref = api.Renderer(sc, w, h, max_bounces=depth, seed=api.DEFAULT_SEED + 1)
    _, ms = timed(lambda: ref.render_device(0, ref_spp))
    ref_mean = mean_rgb(ref.read_frame()[0])
    ref.close()
    emit({"config": name, "what": "reference", "spp": ref_spp, "ms": round(ms, 1)})
    # uniform: warm once (pools, code objects), then timed
    u = api.Renderer(sc, w, h, max_bounces=depth, pipelines=1)
    u.render_device(0, uniform_spp)
    u.reset_accumulation()
    _, ms = timed(lambda: u.render_device(0, uniform_spp))
    target = rmse(u.read_frame()[0], ref_mean)
    rect, _ = u.active_pixels()   # (pixels outside the active rectangle get the miss result without a path)
    uni = emit({"config": name, "what": "uniform", "spp": uniform_spp, "ms": round(ms, 1), "paths": w * h * uniform_spp,
                "paths_traced": rect[1] * rect[3] * uniform_spp, "rmse": target})
    u.close()
    records.append(uni)
    best = None
    r = api.Renderer(sc, w, h, max_bounces=depth, flags=api.FLAG_ADAPTIVE, pipelines=1)
    cap = uniform_spp * cap_factor

    def schedule(rel):
        r.reset_accumulation()
        t_ms, paths, hist, hit, count = 0.0, 0, [], None, 0
        for rnd in range(10_000):
            m = min_samples if rnd == 0 else min(max(4, int(count * growth)), cap - count)
            n, ms = timed(lambda: r.render_adaptive(m, rel, 0.01, min_samples, cap))
            if n == 0:
                break
            t_ms += ms
            paths += n * m
            count += m
            e = rmse(r.read_accumulation(), ref_mean)
            hist.append((n, round(e, 6)))
            if hit is None and e <= target:
                hit = {"rounds": rnd + 1, "ms": round(t_ms, 1), "paths": paths, "rmse": e}
        return t_ms, paths, hist, hit

    for rel in rels:
        schedule(rel)                                   # untimed: grows the pool to what this schedule asks for
        t_ms, paths, hist, hit = schedule(rel)
        rec = emit({"config": name, "what": "adaptive", "rel_error": rel, "abs_floor": 0.01, "min_samples": min_samples, "growth": growth,
                    "max_samples": cap, "ms_total": round(t_ms, 1), "paths_total": paths, "rmse_final": hist[-1][1] if hist else None,
                    "equal_rmse": hit, "active_per_round": [a for a, _ in hist]})
        records.append(rec)
        if hit and (best is None or hit["ms"] < best["equal_rmse"]["ms"]):
            best = rec
    r.close()
    return uni, best


def overhead(records, reps, scene="cornell_box", spp=256):
    """pt_render_adaptive with every pixel selected vs pt_render_device, Cornell 1080p x 256 spp; one context at a time (their pools
    would not fit the device together), each warmed with the call it is timed with.  --overhead-scene cornell_mesh:6 is a scene whose
    BVH stays in global memory: the adaptive path then runs k_shade_surface<LAMBERT, .., LIST> without the inline shadow walk."""
    name, _, level = scene.partition(":")
    sc = getattr(scenes, name)(1920, 1080, **({"level": int(level)} if level else {}))
    every = (spp, 0.0, 0.0, 1 << 24, 0)
    cases = [("render", 0, False), ("render_flag", api.FLAG_ADAPTIVE, False), ("adaptive_all", api.FLAG_ADAPTIVE, True),
             ("render_nocull", api.FLAG_NO_PRIMARY_CULL, False), ("adaptive_all_nocull", api.FLAG_ADAPTIVE | api.FLAG_NO_PRIMARY_CULL, True)]
    t = {}
    for key, flags, adaptive in cases:
        r = api.Renderer(sc, 1920, 1080, max_bounces=8, flags=flags)
        call = (lambda: r.render_adaptive(*every)) if adaptive else (lambda: r.render_device(0, spp))
        call()
        t[key] = []
        for _ in range(reps):
            r.reset_accumulation()
            t[key].append(timed(call)[1])
        if key == "adaptive_all":
            # the selection alone on the finished frame: k_adaptive_count + k_adaptive_write + the small read-back
            sel = [timed(lambda: r.adaptive_mask(0.05, 0.01, 2, 0))[1] for _ in range(5)]
        r.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    pct = lambda a, b: round(100.0 * (med[a] / med[b] - 1.0), 2)
    rec = {"what": "overhead", "config": f"{scene} 1920x1080 x {spp} spp", "reps": reps, "ms": {k: [round(x, 2) for x in v] for k, v in t.items()},
           "median_ms": {k: round(v, 2) for k, v in med.items()}, "adaptive_all_vs_render_pct": pct("adaptive_all", "render"),
           "flag_vs_render_pct": pct("render_flag", "render"), "adaptive_all_vs_render_nocull_pct": pct("adaptive_all_nocull", "render_nocull")}
    records.append(emit(rec))
    records.append(emit({"what": "selection", "config": "cornell 1920x1080", "adaptive_mask_ms": [round(x, 2) for x in sel]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cornell,mixed")
    ap.add_argument("--uniform", type=int, default=256, help="spp of the uniform render whose RMSE the adaptive runs must reach")
    ap.add_argument("--rel", default="0.05,0.035,0.025,0.018,0.012,0.008", help="rel_error values of the sweep")
    ap.add_argument("--growth", type=float, default=0.5, help="a round after the first adds this fraction of the selected pixels' count")
    ap.add_argument("--min-samples", type=int, default=16)
    ap.add_argument("--cap-factor", type=int, default=8, help="max_samples = cap-factor x the uniform spp")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-overhead", action="store_true")
    ap.add_argument("--overhead-scene", default="cornell_box", help="scene of the overhead measurement (scenes.NAME or NAME:level)")
    ap.add_argument("--overhead-spp", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    records = []
    summary = {}
    for name in [c for c in a.configs.split(",") if c]:
        uni, best = run_config(name, a.uniform, [float(x) for x in a.rel.split(",")], a.growth, a.min_samples, a.cap_factor, records)
        summary[name] = {"uniform_ms": uni["ms"], "uniform_paths": uni["paths"], "uniform_rmse": uni["rmse"],
                         "adaptive_equal_rmse": None if best is None else dict(best["equal_rmse"], rel_error=best["rel_error"])}
    if not a.skip_overhead:
        overhead(records, a.reps, a.overhead_scene, a.overhead_spp)
    records.append(emit({"what": "summary", **summary}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
