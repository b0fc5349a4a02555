"""Ray-list record (profiles/r10_rays.md): what pt_integrate_rays_device costs against the same rays rendered as a lens frame, what coherent
ordering is worth, and a probe bake.

The yardstick is pt_render_device of the 1080p Cornell frame under pt_set_lens(40, 950) with PT_FLAG_NO_PRIMARY_CULL, --spp samples; the ray
list is exactly that frame's camera rays (pt_primary_ray, set up in C++ outside the timed window, pixel-major with a pixel's samples
consecutive: the order path ids have in the render).  Every measurement is one child process of tools/rays_bench.cpp's helper (built here with
hipcc), a warm-up call and --reps timed calls ending in a synchronise.  With --parent-lib (another build's libptmi.so, e.g. the parent
commit's) the yardstick is timed with BOTH libraries, alternating, --rounds times; the first round also checks the list's radiance against
pt_render_samples word for word and times the shuffled list.

    python tools/rays_bench.py [--parent-lib PATH] [--rounds 3] [--reps 40] [--spp 16] [--probes 16 --probe-spp 1024] [--out file.json]
    python tools/rays_bench.py --only probes      one measurement alone, e.g. under rocprofv3 --kernel-trace --stats -- python ...
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER = os.path.join(ROOT, "tools", "rays_bench_helper")
LIB = os.path.join(ROOT, "path_tracer_amd", "libptmi.so")


def build_helper():
    src = os.path.join(ROOT, "tools", "rays_bench.cpp")
    deps = [src, os.path.join(ROOT, "include", "pt_api.h")]
    if not os.path.exists(HELPER) or any(os.path.getmtime(d) > os.path.getmtime(HELPER) for d in deps):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-o", HELPER, src, "-ldl"], check=True)
    return HELPER


def run(lib, *args, timeout=600):
    p = subprocess.run([HELPER, lib, os.path.join(ROOT, "models", "cornell")] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    if p.returncode:
        raise SystemExit(f"{' '.join(str(a) for a in args)} with {lib}: exit {p.returncode}\n{p.stderr[-2000:]}")
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    rec["lib"] = os.path.relpath(lib, ROOT)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--probes", type=int, default=16, help="probes per axis of the grid")
    ap.add_argument("--probe-spp", type=int, default=1024)
    ap.add_argument("--only", choices=["render", "rays", "shuffled", "probes"])
    ap.add_argument("--out")
    a = ap.parse_args()
    build_helper()
    frame = (a.width, a.height, a.spp, a.reps)
    if a.only:
        what = {"render": ("render",) + frame, "rays": ("rays",) + frame, "shuffled": ("rays",) + frame + ("shuffle",), "probes": ("probes", a.probes, a.probe_spp)}[a.only]
        run(LIB, *what)
        return
    res = dict(width=a.width, height=a.height, spp=a.spp, reps=a.reps, rounds=[], records=[])
    for k in range(a.rounds):           # alternating: whatever else the machine does falls on every variant
        row = {}
        if a.parent_lib:
            row["parent_render"] = run(os.path.abspath(a.parent_lib), "render", *frame)
        row["render"] = run(LIB, "render", *frame)
        row["rays"] = run(LIB, "rays", *frame, *(["check"] if k == 0 else []))
        if k == 0:
            row["rays_shuffled"] = run(LIB, "rays", *frame, "shuffle")
        res["records"] += list(row.values())
        res["rounds"].append({name: rec["ms_per_call"] for name, rec in row.items()})
    base = "parent_render" if a.parent_lib else "render"
    col = lambda name: [r[name] for r in res["rounds"] if name in r]
    med = lambda v: sorted(v)[len(v) // 2]
    res["yardstick"] = base
    res["yardstick_ms"] = dict(min=min(col(base)), median=med(col(base)), max=max(col(base)))
    res["rays_ms"] = dict(min=min(col("rays")), median=med(col("rays")), max=max(col("rays")))
    res["rays_over_yardstick"] = res["rays_ms"]["median"] / res["yardstick_ms"]["median"]
    res["shuffled_over_rays"] = col("rays_shuffled")[0] / res["rays_ms"]["median"]
    res["probes"] = run(LIB, "probes", a.probes, a.probe_spp)
    print(json.dumps({k: v for k, v in res.items() if k != "records"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
