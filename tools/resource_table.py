#!/usr/bin/env python3
"""Resource table of every kernel of a source file for two sets of compiler flags (compile only, no GPU), as markdown:
waves per SIMD / scratch bytes per lane / VGPRs (spilled VGPRs), and per kernel the static counts of VALU instructions, v_mov_b32,
packed fp32 operations and scratch accesses.  The flags are csrc/Makefile's FLAGS plus what is given.

    python tools/resource_table.py [--src pt_kernels.hip] [--a=<flags>] [--b=<flags>] [--only-changed] [--keep DIR] [--csrc-a DIR]
    python tools/resource_table.py --twins [--axis SURFACE] [--only NAME] [--b=<flags>]   ONE build: every k_shade_surface instantiation whose named axis (QCLASS, MEDIA,
                                                              SHADOW, PATHS, FIRST or SURFACE: the kernel's template parameters in order) is above its base
                                                              value beside its twin, the same instantiation with that axis AT its base value (--only:
                                                              kernels whose name contains NAME)

The default, --a=-fslp-vectorize --b= , compares the SLP vectoriser's pairing with the build's flags (profiles/r08_fp32_pairing.md);
--csrc-a takes the left column's sources (not its flags) from another checkout's path_tracer_amd/csrc."""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_tracer_amd", "csrc")


def makefile_flags():
    """FLAGS of csrc/Makefile (continuation lines joined, make variables expanded with their defaults)."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*\??=\s*(.*)$", text, re.M)}
    return shlex.split(re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["FLAGS"]))


def compile_one(src, extra, keep, csrc=CSRC):
    out = os.path.join(keep, os.path.splitext(src)[0] + ("_b" if extra[1] else "_a") + ".s")
    cmd = [var_hipcc()] + makefile_flags() + shlex.split(extra[0]) + ["-S", "--cuda-device-only", "-o", out, "-x", "hip", src, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if p.returncode:
        raise SystemExit(p.stderr[-2000:])
    return parse_remarks(p.stderr), static_counts(out)


def var_hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def parse_remarks(log):
    res, cur = {}, None
    for line in log.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(":")
        if k == "Function Name":
            cur = res.setdefault(v.strip(), {})
        elif cur is not None:
            cur[k.strip()] = v.strip()
    return res


def static_counts(path):
    out = {}
    s = open(path).read()
    for m in re.finditer(r"^(_Z[^\n:]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M):
        ins = [l.split(";")[0].split() for l in m.group(2).split("\n")]
        ops = [i[0] for i in ins if i and not i[0].startswith(".") and not i[0].endswith(":")]
        out[m.group(1)] = {"valu": sum(o.startswith("v_") for o in ops), "mov": ops.count("v_mov_b32_e32") + ops.count("v_mov_b32"),
                           "pk": sum(bool(re.match(r"v_pk_(mul|add|fma)_f32", o)) for o in ops), "scratch": sum(o.startswith("scratch_") for o in ops)}
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, p):
        d = re.sub(r"\(anonymous namespace\)::|pt::", "", re.sub(r"^void ", "", d))
        short[n] = re.sub(r"\(.*", "", d)   # template arguments identify the variant; the parameter list does not
    return short


SHADE_AXES = ["QCLASS", "MEDIA", "SHADOW", "PATHS", "FIRST", "SURFACE"]   # k_shade_surface's template parameters, in order
AXIS_BASE = {"QCLASS": "1u"}                                            # Q_LAMBERT; every other axis starts at 0


def twin_of(short, axis):
    """the name of a k_shade_surface instantiation with `axis` at its base value, or None if it is there already (or is another kernel)"""
    m = re.fullmatch(r"(k_shade_surface)<(.*)>", short)
    if not m:
        return None
    args = m.group(2).split(", ")
    k, base = SHADE_AXES.index(axis), AXIS_BASE.get(axis, "0u")
    if len(args) != len(SHADE_AXES) or args[k] == base:
        return None
    return f"{m.group(1)}<{', '.join(args[:k] + [base] + args[k + 1:])}>"


def cell(r):
    return f"{r['Occupancy [waves/SIMD]']} / {r['ScratchSize [bytes/lane]']} / {r['VGPRs']}" + (f" ({r['VGPRs Spill']} spilled)" if r["VGPRs Spill"] != "0" else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default="pt_kernels.hip")
    ap.add_argument("--a", default="-fslp-vectorize", help="extra flags of the left column")
    ap.add_argument("--b", default="", help="extra flags of the right column")
    ap.add_argument("--only-changed", action="store_true")
    ap.add_argument("--csrc-a", default=CSRC, help="source directory of the left column (another checkout's path_tracer_amd/csrc)")
    ap.add_argument("--keep", default=None, help="directory that keeps the two assembly files")
    ap.add_argument("--twins", action="store_true", help="one build (--b): k_shade_surface variants beside their twins with --axis at its base value")
    ap.add_argument("--axis", default="SURFACE", choices=SHADE_AXES, help="with --twins: the axis whose base value makes the twin")
    ap.add_argument("--only", default="", help="with --twins: only kernels whose demangled name contains this")
    args = ap.parse_args()
    keep = args.keep or tempfile.mkdtemp(prefix="resource_table_")
    os.makedirs(keep, exist_ok=True)
    if args.twins:
        rb, cb = compile_one(args.src, (args.b, 1), keep)
        names = demangle(list(rb))
        by_short = {names[n]: n for n in rb}
        print(f"`{args.src}`: waves per SIMD / scratch B per lane / VGPRs of the twin ({args.axis} at its base value) and of the variant; static VALU, scratch accesses\n")
        print("| variant | twin | variant | VALU | scratch ops |\n|---|---|---|---|---|")
        n_pairs = fewer_waves = more_scratch = 0
        for n in rb:
            twin = twin_of(names[n], args.axis)
            if twin is None or args.only not in names[n]:
                continue
            t = by_short.get(twin)
            if t is None:
                continue
            a, b = rb[t], rb[n]
            n_pairs += 1
            worse = []
            if int(b["Occupancy [waves/SIMD]"]) < int(a["Occupancy [waves/SIMD]"]):
                fewer_waves += 1; worse.append("fewer waves")
            if int(b["ScratchSize [bytes/lane]"]) > int(a["ScratchSize [bytes/lane]"]):
                more_scratch += 1; worse.append("more scratch")
            print(f"| `{names[n]}`{' **' + ', '.join(worse) + '**' if worse else ''} | {cell(a)} | {cell(b)} | {cb[t]['valu']} -> {cb[n]['valu']} | {cb[t]['scratch']} -> {cb[n]['scratch']} |")
        print(f"\n{n_pairs} variants with a twin; fewer waves per SIMD: {fewer_waves}; more scratch: {more_scratch}")
        return
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        fa, fb = ex.submit(compile_one, args.src, (args.a, 0), keep, os.path.abspath(args.csrc_a)), ex.submit(compile_one, args.src, (args.b, 1), keep)
        (ra, ca), (rb, cb) = fa.result(), fb.result()
    names = demangle(list(rb))
    print(f"`{args.src}`: waves per SIMD / scratch B per lane / VGPRs; static VALU, `v_mov_b32`, packed fp32 (`v_pk_{{mul,add,fma}}_f32`), scratch accesses\n")
    print(f"| kernel | `{args.a or '(build flags)'}` | `{args.b or '(build flags)'}` | VALU | v_mov | packed | scratch ops |\n|---|---|---|---|---|---|---|")
    n_changed = fewer_waves = more_scratch = 0
    for n in rb:
        a, b = ra.get(n), rb[n]
        if a is None:
            continue
        changed = cell(a) != cell(b)
        n_changed += changed
        worse = []
        if int(b["Occupancy [waves/SIMD]"]) < int(a["Occupancy [waves/SIMD]"]):
            fewer_waves += 1; worse.append("fewer waves")
        if int(b["ScratchSize [bytes/lane]"]) > int(a["ScratchSize [bytes/lane]"]):
            more_scratch += 1; worse.append("more scratch")
        if args.only_changed and not changed:
            continue
        x, y = ca[n], cb[n]
        print(f"| `{names[n]}`{' **' + ', '.join(worse) + '**' if worse else ''} | {cell(a)} | {cell(b)} | {x['valu']} -> {y['valu']} | {x['mov']} -> {y['mov']} | {x['pk']} -> {y['pk']} | {x['scratch']} -> {y['scratch']} |")
    print(f"\n{len(rb)} kernels, {n_changed} with a different resource line; fewer waves per SIMD: {fewer_waves}; more scratch: {more_scratch}")


if __name__ == "__main__":
    main()
