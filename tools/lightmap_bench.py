#!/usr/bin/env python3
"""What a lightmap bake costs over the bare integrator (profiles/r15_lightmap.md): a SIZE x SIZE x SPP map of a Cornell box model under the
tests' box atlas (no overlap), beside pt_integrate_rays_device given a ray table of the same shape rebuilt in torch from lightmap_texels -
the same origins P + bias * n, stream keys and samples, texel-major with a texel's samples consecutive, and cosine-distributed directions over
the same normals from torch's generator (the bake's own Sobol points have no device-side hook; the distribution and the order are the bake's).
The difference is coverage, resolve, ray generation, fold and the map's copies; the texel table alone is timed too.

    python tools/lightmap_bench.py [--size 1024] [--spp 64] [--reps 3] [--model cb_box_short] [--only bake|rays] [--out report.json]

--only bake with --reps 1 is the run to put under rocprofv3 --kernel-trace --stats for the per-kernel table (tools/kernel_times.py).

    python tools/lightmap_bench.py --denoise [--size 1024] [--reps 3] [--out report.json]

times the texel filter (pt_lightmap_denoise, profiles/r23_lightmap_denoise.md) beside the bake it follows: the moments bake against the plain
bake at 16 samples, the blocking filter call at 1 and at 5 levels (their difference / 4 is a level; what is left of the 1-level call is the
texel table, the prep and the staging of the map's copies), and the filter's purpose on the tests' 48 x 32 map: RMSE over covered texels of
the raw and of the denoised mean at 4, 16 and 64 samples against a 4096-sample bake of disjoint samples.

    python tools/lightmap_bench.py --adaptive [--size 1024] [--spp 16] [--reps 5] [--rel 0.05] [--cap 64] [--out report.json]

measures adaptive baking (pt_bake_lightmap_adaptive, profiles/r32_adaptive_lightmap.md).  OVERHEAD: one all-active adaptive call from zero
arrays (min_samples = max_samples = SPP) beside pt_bake_lightmap_moments of the same SPP at SIZE x SIZE, alternating; the rays and the fold
are the same, so the difference is the selection and the three arrays' transfers less the coverage round trip saved.  GAIN: on the tests'
48 x 32 map and on a 256 x 256 one, rounds of 4 samples under (REL, floor 0.01, at least 4, at most CAP) until no texel is selected, beside
uniform bakes of the same ray budget (the mean count rounded down and up): RMSE over covered texels, raw and through the texel filter,
against a 4096-sample bake of OTHER samples (key_base shifted by 2^24), and the distribution of the counts.

    python tools/lightmap_bench.py --direct [--size 1024] [--spp 64] [--reps 5] [--only-cost] [--out report.json]

measures direct light sampled at the texel (pt_bake_lightmap_direct, profiles/r34_lightmap_direct.md).  QUALITY, on the tests' 48 x 32 map: RMSE
over covered texels against a 4096-sample PLAIN bake of other samples (key_base shifted by 2^24) of the plain and the direct bake at 4, 16 and
64 samples, raw and through the texel filter; of both adaptive bakes (rounds of 4 under REL, floor 0.01, at least 4, at most 64) at REL 0.05,
0.1 and 0.2 with the rays each spent, beside a uniform direct bake of the plain adaptive bake's budget; and the residual of a 4096-sample
direct bake of yet other samples, which is clamp and estimator differences.  COST: the direct and the plain bake at SIZE x SIZE x SPP,
alternating, every time kept (--only-cost with --reps 1 is the run for rocprofv3 --kernel-trace --stats: the light-sample kernel, the any-hit
launch and the fold are kernels of their own).

    python tools/lightmap_bench.py --gather [--size 1024] [--spp 64] [--reps 5] [--passes 8] [--only-cost] [--out report.json]

measures the final-gather bake (pt_bake_lightmap_gather, profiles/r35_lightmap_gather.md).  COST: one gather pass with direct = 1 beside the
direct bake at SIZE x SIZE x SPP, alternating, every time kept; the box's own map (a direct bake's dilated means) is set, so the gather
chains that reach it end in a lookup (--only-cost with --reps 1 is the run for rocprofv3 --kernel-trace --stats).  NOISE, in the tests' lit
room, where every surface but the lamp is mapped, on 48 x 32 maps: RMSE over the room map's covered texels against a 4096-sample direct bake
of other samples, of every pass of the Jacobi loop (bake_lightmaps_gather from no maps, PASSES passes) at 4, 16 and 64 samples, beside the
direct bake's at the same counts: early passes lack their later bounces, late ones show the estimator's noise and the maps' own bias."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, DEPTH, BIAS = 1920, 1080, 8, 0.25


def torch_rays(torch, table, spp):
    """the bake's ray table on the device: (o, d, key, sample), texel-major"""
    prim, _, position, normal = table
    dev = torch.device("cuda")
    k = torch.from_numpy(np.flatnonzero(prim.reshape(-1) != 0xFFFFFFFF).astype(np.int64)).to(dev)
    P = torch.from_numpy(position.reshape(-1, 3)).to(dev)[k]
    n = torch.from_numpy(normal.reshape(-1, 3)).to(dev)[k]
    o = (P + BIAS * n).repeat_interleave(spp, 0).contiguous()
    n = n.repeat_interleave(spp, 0)
    gen = torch.Generator(device=dev).manual_seed(15)
    u = torch.rand((n.shape[0], 2), generator=gen, device=dev)
    r, phi = u[:, 0].sqrt(), 6.2831855 * u[:, 1]
    local = torch.stack([phi.cos() * r, phi.sin() * r, (1 - r * r).clamp_min(0).sqrt()], 1)
    # any orthonormal pair around n (material/onb.rs)
    sign = torch.copysign(torch.ones_like(n[:, 2]), n[:, 2])
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    c0 = torch.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], 1)
    c1 = torch.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], 1)
    d = (c0 * local[:, 0:1] + c1 * local[:, 1:2] + n * local[:, 2:3]).contiguous()
    key = k.to(torch.int32).repeat_interleave(spp).contiguous()
    sample = torch.arange(spp, dtype=torch.int32, device=dev).repeat(k.shape[0]).contiguous()
    return o, d, key, sample


def rmse(a, b, covered):
    d = (a.astype(np.float64) - b.astype(np.float64))[covered]
    return float(np.sqrt((d * d).mean()))


def denoise_report(r, model, size, reps):
    spp = 16
    report = {"size": size, "spp": spp, "bake_ms": [], "bake_moments_ms": [], "filter_1_level_ms": [], "filter_5_levels_ms": [], "filter_5_levels_spatial_ms": []}
    r.bake_lightmap(model, 0, size, size, 1, bias=BIAS)                          # warm-up, as below
    sums, sumsq, cov = r.bake_lightmap_moments(model, 0, size, size, 1, bias=BIAS)
    r.denoise_lightmap(model, 0, sums, 1, sumsq=sumsq, iterations=1)
    for _ in range(reps):
        t0 = time.perf_counter()
        r.bake_lightmap(model, 0, size, size, spp, bias=BIAS)
        report["bake_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        sums, sumsq, cov = r.bake_lightmap_moments(model, 0, size, size, spp, bias=BIAS)
        report["bake_moments_ms"].append(1e3 * (time.perf_counter() - t0))
        for name, kw in (("filter_1_level_ms", dict(sumsq=sumsq, iterations=1)), ("filter_5_levels_ms", dict(sumsq=sumsq, iterations=5)),
                         ("filter_5_levels_spatial_ms", dict(iterations=5))):
            t0 = time.perf_counter()
            r.denoise_lightmap(model, 0, sums, spp, **kw)                        # blocking
            report[name].append(1e3 * (time.perf_counter() - t0))
    report["covered"] = int(cov.sum())
    report["level_ms"] = (min(report["filter_5_levels_ms"]) - min(report["filter_1_level_ms"])) / 4.0
    report["table_prep_staging_ms"] = min(report["filter_1_level_ms"]) - report["level_ms"]
    # the error figures, on the map of tests/test_gpu_lightmap_denoise.py; the reference takes samples 16 .. 4111, the 64-sample bake the 64 after
    w, h = 48, 32
    ref, cov = r.bake_lightmap(model, 0, w, h, 4096, first_sample=16, bias=BIAS)
    ref = ref / np.float32(4096)
    report["rmse"] = {}
    for n, first in ((4, 0), (16, 0), (64, 16 + 4096)):
        sums, sumsq, _ = r.bake_lightmap_moments(model, 0, w, h, n, first_sample=first, bias=BIAS)
        den = r.denoise_lightmap(model, 0, sums, n, sumsq=sumsq)
        spatial = r.denoise_lightmap(model, 0, sums, n)
        report["rmse"][str(n)] = {"raw": rmse(sums / np.float32(n), ref, cov == 1), "denoised": rmse(den, ref, cov == 1), "denoised_spatial_variance": rmse(spatial, ref, cov == 1)}
    return report


def adaptive_report(r, model, size, spp, reps, rel, cap):
    report = {"size": size, "spp": spp, "rel_error": rel, "cap": cap, "bake_moments_ms": [], "adaptive_all_active_ms": []}
    for _ in range(2):                  # warm-up at the timed shape: scene upload, code objects, the wavefront pool, the staging sizes
        r.bake_lightmap_moments(model, 0, size, size, spp, bias=BIAS)
        r.bake_lightmap_adaptive(model, 0, size, size, spp, 0.0, min_samples=spp, max_samples=spp, bias=BIAS)
    for _ in range(reps):               # the two routes alternate, so that a drift of the shared machine touches both
        t0 = time.perf_counter()
        plain = r.bake_lightmap_moments(model, 0, size, size, spp, bias=BIAS)
        report["bake_moments_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ad = r.bake_lightmap_adaptive(model, 0, size, size, spp, 0.0, min_samples=spp, max_samples=spp, bias=BIAS)
        report["adaptive_all_active_ms"].append(1e3 * (time.perf_counter() - t0))
    report["covered"] = int(plain[2].sum())
    report["all_active_equals_plain"] = bool(np.array_equal(plain[0].view(np.uint32), ad[0].view(np.uint32)) and np.array_equal(plain[1].view(np.uint32), ad[1].view(np.uint32))
                                             and ad[4] == report["covered"])
    report["overhead_ms"] = float(np.median(report["adaptive_all_active_ms"]) - np.median(report["bake_moments_ms"]))
    report["gain"] = {}
    f32 = np.float32
    for w, h in ((48, 32), (256, 256)):
        ref, cov = r.bake_lightmap(model, 0, w, h, 4096, key_base=1 << 24, bias=BIAS)
        ref = ref / f32(4096)
        covered = cov == 1
        state, rays, rounds, spent = (None, None, None), 0, 0, 0.0
        while True:
            t0 = time.perf_counter()
            *state, _, n_active = r.bake_lightmap_adaptive(model, 0, w, h, 4, rel, abs_floor=0.01, min_samples=4, max_samples=cap, bias=BIAS, sums=state[0], sumsq=state[1], counts=state[2])
            spent += time.perf_counter() - t0
            if n_active == 0:
                break
            rays += n_active * 4
            rounds += 1
        sums, sumsq, counts = state
        mean = np.zeros_like(sums)
        mean[covered] = sums[covered] / counts[covered].astype(f32)[:, None]
        values, freq = np.unique(counts[covered], return_counts=True)
        g = {"covered": int(covered.sum()), "rays": int(rays), "rounds": rounds, "adaptive_ms": 1e3 * spent, "mean_count": float(counts[covered].mean()),
             "counts": {str(int(v)): int(f) for v, f in zip(values, freq)},
             "adaptive": {"raw": rmse(mean, ref, covered), "denoised": rmse(r.denoise_lightmap(model, 0, sums, 0, sumsq=sumsq, counts=counts), ref, covered)}}
        for name, n in (("uniform_floor", rays // g["covered"]), ("uniform_ceil", -(-rays // g["covered"]))):
            t0 = time.perf_counter()
            u = r.bake_lightmap_moments(model, 0, w, h, n, bias=BIAS)
            g[name] = {"samples": int(n), "rays": int(n) * g["covered"], "ms": 1e3 * (time.perf_counter() - t0), "raw": rmse(u[0] / f32(n), ref, covered),
                       "denoised": rmse(r.denoise_lightmap(model, 0, u[0], n, sumsq=u[1]), ref, covered)}
        report["gain"][f"{w}x{h}"] = g
    return report


def direct_report(r, model, size, spp, reps, only_cost):
    f32 = np.float32
    report = {"size": size, "spp": spp, "plain_ms": [], "direct_ms": []}
    for _ in range(2):                  # warm-up at the timed shape
        r.bake_lightmap(model, 0, size, size, spp, bias=BIAS)
        r.bake_lightmap_direct(model, 0, size, size, spp, bias=BIAS)
    for _ in range(reps):               # the two routes alternate, so that a drift of the shared machine touches both
        t0 = time.perf_counter()
        plain = r.bake_lightmap(model, 0, size, size, spp, bias=BIAS)
        report["plain_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        direct = r.bake_lightmap_direct(model, 0, size, size, spp, bias=BIAS)
        report["direct_ms"].append(1e3 * (time.perf_counter() - t0))
    covered = plain[1] == 1
    report["covered"] = int(covered.sum())
    report["rays"] = report["covered"] * spp
    for name in ("plain", "direct"):
        t = report[name + "_ms"]
        report[name + "_median_ms"], report[name + "_spread_ms"] = float(np.median(t)), [float(min(t)), float(max(t))]
    report["mean_irradiance"] = {"plain": float(np.pi * plain[0][covered].mean() / spp), "direct": float(np.pi * direct[0][covered].mean() / spp)}
    if only_cost:
        return report
    w, h = 48, 32
    ref, cov = r.bake_lightmap(model, 0, w, h, 4096, key_base=1 << 24, bias=BIAS)
    ref = ref / f32(4096)
    covered = cov == 1
    report["quality"] = {"covered": int(covered.sum()), "uniform": {}, "adaptive": {}}
    q = report["quality"]
    for n in (4, 16, 64):
        row = {}
        for name, bake in (("plain", lambda: r.bake_lightmap_moments(model, 0, w, h, n, bias=BIAS)), ("direct", lambda: r.bake_lightmap_direct(model, 0, w, h, n, bias=BIAS, moments=True))):
            sums, sumsq, _ = bake()
            row[name] = {"raw": rmse(sums / f32(n), ref, covered), "denoised": rmse(r.denoise_lightmap(model, 0, sums, n, sumsq=sumsq), ref, covered)}
        q["uniform"][str(n)] = row
    big, _ = r.bake_lightmap_direct(model, 0, w, h, 4096, key_base=1 << 25, bias=BIAS)
    again, _ = r.bake_lightmap(model, 0, w, h, 4096, key_base=1 << 25, bias=BIAS)
    q["residual_4096"] = {"direct": rmse(big / f32(4096), ref, covered), "plain_of_the_same_samples": rmse(again / f32(4096), ref, covered)}
    err = np.abs((big / f32(4096)).astype(np.float64) - ref.astype(np.float64)).mean(2)
    q["residual_4096"]["largest_texel"] = {"error": float(err[covered].max()), "texel": [int(v) for v in np.unravel_index(np.argmax(np.where(covered, err, -1)), err.shape)]}
    for rel in (0.05, 0.1, 0.2):
        row = {}
        for name, bake in (("plain", r.bake_lightmap_adaptive), ("direct", r.bake_lightmap_adaptive_direct)):
            state, rays = (None, None, None), 0
            while True:
                *state, _, n_active = bake(model, 0, w, h, 4, rel, abs_floor=0.01, min_samples=4, max_samples=64, bias=BIAS, sums=state[0], sumsq=state[1], counts=state[2])
                if n_active == 0:
                    break
                rays += n_active * 4
            sums, sumsq, counts = state
            mean = np.zeros_like(sums)
            mean[covered] = sums[covered] / counts[covered].astype(f32)[:, None]
            row[name] = {"rays": int(rays), "mean_count": float(counts[covered].mean()), "raw": rmse(mean, ref, covered),
                         "denoised": rmse(r.denoise_lightmap(model, 0, sums, 0, sumsq=sumsq, counts=counts), ref, covered)}
        n = -(-row["plain"]["rays"] // q["covered"])
        sums, sumsq, _ = r.bake_lightmap_direct(model, 0, w, h, n, bias=BIAS, moments=True)
        row["direct_uniform_at_the_plain_budget"] = {"samples": int(n), "rays": int(n) * q["covered"], "raw": rmse(sums / f32(n), ref, covered),
                                                      "denoised": rmse(r.denoise_lightmap(model, 0, sums, n, sumsq=sumsq), ref, covered)}
        q["adaptive"][str(rel)] = row
    return report


def gather_report(r, api, model, size, spp, reps, passes, only_cost):
    f32 = np.float32
    report = {"size": size, "spp": spp, "direct_ms": [], "gather_ms": []}
    sums, cov = r.bake_lightmap_direct(model, 0, size, size, 4, bias=BIAS)
    r.set_lightmap(model, 0, r.dilate_lightmap(sums / f32(4), cov, 1)[0])
    for _ in range(2):                  # warm-up at the timed shape
        r.bake_lightmap_direct(model, 0, size, size, spp, bias=BIAS)
        r.bake_lightmap_gather(model, 0, size, size, spp, bias=BIAS, follow=2)
    for _ in range(reps):               # the two routes alternate, so that a drift of the shared machine touches both
        t0 = time.perf_counter()
        direct = r.bake_lightmap_direct(model, 0, size, size, spp, bias=BIAS)
        report["direct_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        gather = r.bake_lightmap_gather(model, 0, size, size, spp, bias=BIAS, follow=2)
        report["gather_ms"].append(1e3 * (time.perf_counter() - t0))
    covered = direct[1] == 1
    report["covered"] = int(covered.sum())
    report["rays"] = report["covered"] * spp
    for name in ("direct", "gather"):
        t = report[name + "_ms"]
        report[name + "_median_ms"], report[name + "_spread_ms"] = float(np.median(t)), [float(min(t)), float(max(t))]
    report["mean_irradiance"] = {"direct": float(np.pi * direct[0][covered].mean() / spp), "gather_one_pass": float(np.pi * gather[0][covered].mean() / spp)}
    if only_cost:
        return report
    import baked_common as BC
    sc, placements = BC.lit_room()
    lit = api.Renderer(sc, 48, 32, max_bounces=DEPTH)
    w, h = 48, 32
    ref, cov = lit.bake_lightmap_direct(0, 0, w, h, 4096, key_base=1 << 24, bias=BIAS)
    ref = ref / f32(4096)
    covered = cov == 1
    report["noise"] = {"covered": int(covered.sum()), "passes": passes, "rmse": {}}
    for n in (4, 16, 64):
        d, _ = lit.bake_lightmap_direct(0, 0, w, h, n, bias=BIAS)
        for p in placements:
            lit.set_lightmap(*p, None)
        per_pass = lit.bake_lightmaps_gather(placements, [(w, h)] * len(placements), n, passes, bias=BIAS)
        report["noise"]["rmse"][str(n)] = {"direct": rmse(d / f32(n), ref, covered), "gather_per_pass": [rmse(q[0][0] / f32(n), ref, covered) for q in per_pass]}
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--only-cost", action="store_true")
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--rel", type=float, default=0.05)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", default="cb_box_short")
    ap.add_argument("--only", choices=["bake", "rays"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lightmap_bench needs the GPU: there is nothing to time without one")
    import lightmap_common as LC
    from path_tracer_amd import api
    sc, model = LC.cornell_atlas_scene(args.model, W, H)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    size, spp = args.size, args.spp
    if args.denoise or args.adaptive or args.direct or args.gather:
        line = json.dumps(gather_report(r, api, model, size, spp, args.reps, args.passes, args.only_cost) if args.gather
                          else direct_report(r, model, size, spp, args.reps, args.only_cost) if args.direct
                          else adaptive_report(r, model, size, spp, args.reps, args.rel, args.cap) if args.adaptive else denoise_report(r, model, size, args.reps))
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    # warm-up: scene upload, code objects, the wavefront pool at the size the timed calls use
    r.bake_lightmap(model, 0, size, size, 1, bias=BIAS)
    table = r.lightmap_texels(model, 0, size, size, on_device=True)
    covered = int((table[0] != 0xFFFFFFFF).sum())
    report = {"size": size, "spp": spp, "model": args.model, "covered": covered, "rays": covered * spp, "bake_ms": [], "rays_ms": [], "texels_ms": []}
    rays = None
    if args.only != "bake":
        rays = torch_rays(torch, table, spp)
        r.integrate_rays(rays[0][:covered], rays[1][:covered], rays[2][:covered], rays[3][:covered])
    for _ in range(args.reps):          # the two routes alternate, so that a drift of the shared machine touches both
        if args.only != "rays":
            t0 = time.perf_counter()
            r.lightmap_texels(model, 0, size, size, on_device=True)
            report["texels_ms"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            sums, _ = r.bake_lightmap(model, 0, size, size, spp, bias=BIAS)      # blocking
            report["bake_ms"].append(1e3 * (time.perf_counter() - t0))
        if args.only != "bake":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = r.integrate_rays(*rays)                                        # blocking: the results are complete when it returns
            torch.cuda.synchronize()
            report["rays_ms"].append(1e3 * (time.perf_counter() - t0))
            del out
    if report["bake_ms"]:
        report["mean_irradiance"] = float(np.pi * sums[table[0] != 0xFFFFFFFF].mean() / spp)
    if report["bake_ms"] and report["rays_ms"]:
        report["over_the_integrator_ms"] = min(report["bake_ms"]) - min(report["rays_ms"])
    line = json.dumps(report)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
