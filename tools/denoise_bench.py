"""Denoiser record (profiles/r07_denoise.md): quality and cost of pt_render_guides + pt_denoise.

Quality: RMSE of the noisy mean and of the denoised frame against a many-sample render of the same scene, for several sample counts and
both variance sources (spatial variance; moments of PT_FLAG_ADAPTIVE), in linear radiance and in display space (the library's own GT tonemap,
what pt_present shows).  The noisy frames use samples after the reference's, so the two are independent.
Timing: wall clock of the blocking calls at the given size (median of --reps), guides and the filter separately.

--albedo adds the demodulated filter (pt_denoise_albedo, profiles/r13_denoise_albedo.md): its RMSE with the albedo guide and with the mean
albedo beside pt_denoise's, its cost beside pt_denoise's, and the cost of one sample of pt_accumulate_albedo beside one pt_render_guides.

--follow K takes the guides (and the mean albedo) through mirrors and glass, up to K per pixel (pt_render_guides_followed,
profiles/r16_followed_guides.md), and adds the cost of the guides on the mixed Cornell box at the timing size: the plain call and max_hops
1, 2 and 8 measured in turn, --reps rounds (median, min and max of each).

--temporal adds the temporal stage (pt_frame_temporal, profiles/r20_temporal.md): the display-space RMSE of the last of --temporal-frames
1-spp frames of a slow camera pan against a many-sample render of the last pose, for the raw frame, for pt_frame_moving + pt_denoise over
the same sequence and for pt_frame_temporal; and at the timing size the whole calls in turn, round by round: pt_frame_moving + pt_denoise,
pt_frame_temporal in steady state, and pt_frame_temporal on the frames right after a cut (pt_reset_temporal), where every pixel still walks
the 7 x 7 spatial variance.  It then measures the stage's options (rescue, length_rule, demodulate; profiles/r21_temporal_options.md): the same
pan under each option set on the Cornell box and on the checker-textured one (scenes.checker_textured), and at the timing size
pt_frame_temporal in steady state and after a cut with no option, each option and all three, one after the other in every round.

    python tools/denoise_bench.py [--albedo] [--follow K] [--temporal] [--size 256] [--ref-spp 4096] [--spp 1,4,16,64] [--width 1920 --height 1080 --reps 20] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def quality(api, scenes, name, size, ref_spp, spps, depth, albedo=False, follow=0):
    sc = {"cornell": scenes.cornell_box, "mixed": scenes.cornell_mixed}[name](size, size)
    ref = api.Renderer(sc, size, size, max_bounces=depth)
    racc, _, _ = ref.render(0, ref_spp, want_position=False)
    ref_mean = racc / racc[..., 3:4]
    ref_disp = ref.post_tonemap(racc)
    rows = []
    for spp in spps:
        for flags, source in ((0, "spatial"), (api.FLAG_ADAPTIVE, "moments")):
            r = api.Renderer(sc, size, size, max_bounces=depth, flags=flags)
            acc, _, _ = r.render(ref_spp, spp, want_position=False)
            r.render_guides(ref_spp + spp - 1, follow=follow)
            den = r.denoise()
            noisy = acc / acc[..., 3:4]
            row = dict(follow=follow, scene=name, size=size, spp=spp, variance=source, rmse_noisy=rmse(noisy, ref_mean), rmse_denoised=rmse(den, ref_mean),
                       display_rmse_noisy=rmse(r.post_tonemap(acc), ref_disp), display_rmse_denoised=rmse(r.post_tonemap(den), ref_disp))
            row["ratio"] = row["rmse_denoised"] / row["rmse_noisy"]
            row["display_ratio"] = row["display_rmse_denoised"] / row["display_rmse_noisy"]
            if albedo:
                r.accumulate_albedo(ref_spp, spp, follow=follow)
                for key, src in (("guide", api.ALBEDO_GUIDE), ("mean", api.ALBEDO_MEAN)):
                    dal = r.denoise_albedo(src)
                    row[f"rmse_albedo_{key}"] = rmse(dal, ref_mean)
                    row[f"display_rmse_albedo_{key}"] = rmse(r.post_tonemap(dal), ref_disp)
            print(json.dumps(row), flush=True)
            rows.append(row)
            r.close()
    ref.close()
    return rows


def timing(api, scenes, w, h, reps, depth, albedo=False):
    out = {}
    for flags, source in ((0, "spatial"), (api.FLAG_ADAPTIVE, "moments")):
        r = api.Renderer(scenes.cornell_box(w, h), w, h, max_bounces=depth, flags=flags)
        r.render(0, 1, want_position=False)
        tg, td = [], []
        for k in range(reps + 2):
            t0 = time.perf_counter(); r.render_guides(k); t1 = time.perf_counter()
            r.denoise(download=False); t2 = time.perf_counter()
            if k >= 2:
                tg.append(t1 - t0); td.append(t2 - t1)
        out[source] = dict(ms_guides=1e3 * float(np.median(tg)), ms_denoise=1e3 * float(np.median(td)))
        if albedo:
            ta, tdg, tdm = [], [], []
            for k in range(reps + 2):
                t0 = time.perf_counter(); r.accumulate_albedo(4 * k, 4); t1 = time.perf_counter()
                r.denoise_albedo(api.ALBEDO_GUIDE, download=False); t2 = time.perf_counter()
                r.denoise_albedo(api.ALBEDO_MEAN, download=False); t3 = time.perf_counter()
                if k >= 2:
                    ta.append((t1 - t0) / 4); tdg.append(t2 - t1); tdm.append(t3 - t2)
            out[source].update(ms_accumulate_albedo_per_sample=1e3 * float(np.median(ta)), ms_denoise_albedo_guide=1e3 * float(np.median(tdg)),
                               ms_denoise_albedo_mean=1e3 * float(np.median(tdm)))
        r.close()
    row = dict(width=w, height=h, reps=reps, **{f"{k}_{s}": v for s, d in out.items() for k, v in d.items()})
    print(json.dumps(row), flush=True)
    return row


def follow_timing(api, scenes, w, h, reps, depth):
    """pt_render_guides and pt_render_guides_followed at max_hops 1, 2, 8 on the mixed Cornell box, one after the other in every round"""
    r = api.Renderer(scenes.cornell_mixed(w, h), w, h, max_bounces=depth)
    hops = (0, 1, 2, 8)
    t = {k: [] for k in hops}
    for k in range(reps + 2):
        for f in hops:
            t0 = time.perf_counter(); r.render_guides(k, follow=f); t1 = time.perf_counter()
            if k >= 2:
                t[f].append(1e3 * (t1 - t0))
    followed = float((r.read_guide_hops() > 0).mean())
    r.close()
    row = dict(scene="mixed", width=w, height=h, reps=reps, followed_fraction_at_8=followed)
    for f in hops:
        row[f"ms_guides_follow_{f}"] = dict(median=float(np.median(t[f])), min=float(np.min(t[f])), max=float(np.max(t[f])))
    print(json.dumps(row), flush=True)
    return row


PAN = (1.0, 0.0, 4.0e-7)   # EV_MOUSE_MOTION per frame: 0.004 rad, half a pixel of a 128-pixel, 60-degree frame


OPTION_SETS = [("plain", {}), ("rescue", dict(rescue=1)), ("mean", dict(length_rule=1)), ("rescue+mean", dict(rescue=1, length_rule=1)),
               ("demodulate", dict(demodulate=1)), ("all", dict(rescue=1, length_rule=1, demodulate=1))]


def temporal_quality(api, scenes, size, frames, ref_spp, depth, feedback=0, pan=True, scene="cornell", **params):
    sc = scenes.cornell_box(size, size)
    if scene == "checker":
        sc = scenes.checker_textured(sc)
    t = api.Renderer(sc, size, size, max_bounces=depth); m = api.Renderer(sc, size, size, max_bounces=depth)
    ref = api.Renderer(sc, size, size, max_bounces=depth)
    last_t, last_m = t.inv_projection(), m.inv_projection()
    for k in range(frames):
        if k and pan:
            for r in (t, m, ref):
                r.camera_input(api.EV_MOUSE_MOTION, *PAN)
        data, _, _, out = t.frame_temporal(k, last_t, feedback=feedback, **params)
        m.frame_moving(k, last_m, download=False)
        last_t, last_m = t.inv_projection(), m.inv_projection()
    den = m.denoise()
    hist = t.read_temporal()[0]
    n = hist[..., 3]
    hist = np.concatenate([hist[..., :3], np.ones_like(hist[..., 3:])], -1)     # (with feedback: level 0's output)
    racc, _, _ = ref.render(1 << 20, ref_spp, want_position=False)
    ref_disp = ref.post_tonemap(racc)
    row = dict(scene=scene, size=size, frames=frames, ref_spp=ref_spp, feedback=feedback, pan=pan, params=params, display_rmse_history=rmse(t.post_tonemap(hist), ref_disp), display_rmse_raw=rmse(t.post_tonemap(data), ref_disp),
               display_rmse_moving_denoise=rmse(m.post_tonemap(den), ref_disp), display_rmse_temporal=rmse(t.post_tonemap(out), ref_disp),
               mean_history=float(n.mean()), disoccluded=int((n == 1).sum()))
    for r in (t, m, ref):
        r.close()
    print(json.dumps(row), flush=True)
    return row


def temporal_timing(api, scenes, w, h, reps, depth):
    sc = scenes.cornell_box(w, h)
    m = api.Renderer(sc, w, h, max_bounces=depth); t = api.Renderer(sc, w, h, max_bounces=depth); c = api.Renderer(sc, w, h, max_bounces=depth)
    last = {id(r): r.inv_projection() for r in (m, t, c)}
    tm, td, ts, tc = [], [], [], []
    for k in range(reps + 4):
        for r in (m, t, c):
            r.camera_input(api.EV_MOUSE_MOTION, *PAN)
        t0 = time.perf_counter(); m.frame_moving(k, last[id(m)], download=False); t1 = time.perf_counter()
        m.denoise(download=False); t2 = time.perf_counter()
        t.frame_temporal(k, last[id(t)], download=False); t3 = time.perf_counter()
        c.reset_temporal()
        c.frame_temporal(k, last[id(c)], download=False); t4 = time.perf_counter()
        for r in (m, t, c):
            last[id(r)] = r.inv_projection()
        if k >= 4:
            tm.append(t1 - t0); td.append(t2 - t1); ts.append(t3 - t2); tc.append(t4 - t3)
    young = float((t.read_temporal()[0][..., 3] < 4).mean())
    for r in (m, t, c):
        r.close()
    med = lambda v: dict(median=1e3 * float(np.median(v)), min=1e3 * float(np.min(v)), max=1e3 * float(np.max(v)))
    row = dict(width=w, height=h, reps=reps, ms_frame_moving=med(tm), ms_denoise=med(td), ms_frame_temporal_steady=med(ts), ms_frame_temporal_after_cut=med(tc),
               steady_fraction_below_4=young)
    print(json.dumps(row), flush=True)
    return row


def temporal_option_timing(api, scenes, w, h, reps, depth):
    """pt_frame_temporal under every option set, steady and right after a cut, in turn in every round (the plain stage is one of the sets)"""
    sc = scenes.cornell_box(w, h)
    steady = {n: api.Renderer(sc, w, h, max_bounces=depth) for n, _ in OPTION_SETS}
    cut = {n: api.Renderer(sc, w, h, max_bounces=depth) for n, _ in OPTION_SETS}
    everyone = list(steady.values()) + list(cut.values())
    last = {id(r): r.inv_projection() for r in everyone}
    ts = {n: [] for n, _ in OPTION_SETS}; tc = {n: [] for n, _ in OPTION_SETS}
    for k in range(reps + 4):
        for r in everyone:
            r.camera_input(api.EV_MOUSE_MOTION, *PAN)
        for n, opt in OPTION_SETS:
            t0 = time.perf_counter(); steady[n].frame_temporal(k, last[id(steady[n])], download=False, **opt); t1 = time.perf_counter()
            cut[n].reset_temporal()
            cut[n].frame_temporal(k, last[id(cut[n])], download=False, **opt); t2 = time.perf_counter()
            if k >= 4:
                ts[n].append(t1 - t0); tc[n].append(t2 - t1)
        for r in everyone:
            last[id(r)] = r.inv_projection()
    lost = float((steady["plain"].read_temporal()[0][..., 3] == 1).mean())
    for r in everyone:
        r.close()
    med = lambda v: dict(median=1e3 * float(np.median(v)), min=1e3 * float(np.min(v)), max=1e3 * float(np.max(v)))
    row = dict(width=w, height=h, reps=reps, plain_fraction_restarted=lost, steady={n: med(v) for n, v in ts.items()}, after_cut={n: med(v) for n, v in tc.items()})
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--spp", default="1,4,16,64")
    ap.add_argument("--scenes", default="cornell,mixed")
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--albedo", action="store_true", help="also measure pt_accumulate_albedo and pt_denoise_albedo")
    ap.add_argument("--follow", type=int, default=0, help="follow up to K mirror / glass surfaces per pixel in the guides (0..8)")
    ap.add_argument("--temporal", action="store_true", help="also measure pt_frame_temporal against pt_frame_moving + pt_denoise")
    ap.add_argument("--temporal-size", type=int, default=128)
    ap.add_argument("--temporal-frames", type=int, default=16)
    ap.add_argument("--temporal-ref-spp", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    from path_tracer_amd import api, scenes
    res = dict(quality=[], timing=None)
    if not a.no_quality:
        for name in a.scenes.split(","):
            res["quality"] += quality(api, scenes, name, a.size, a.ref_spp, [int(s) for s in a.spp.split(",")], a.bounces, a.albedo, a.follow)
    if a.reps > 0:
        res["timing"] = timing(api, scenes, a.width, a.height, a.reps, a.bounces, a.albedo)
        if a.follow:
            res["follow_timing"] = follow_timing(api, scenes, a.width, a.height, a.reps, a.bounces)
    if a.temporal:
        if not a.no_quality:
            res["temporal_quality"] = [temporal_quality(api, scenes, a.temporal_size, a.temporal_frames, a.temporal_ref_spp, a.bounces, feedback=f) for f in (0, 1)]
            res["temporal_option_quality"] = [temporal_quality(api, scenes, a.temporal_size, a.temporal_frames, a.temporal_ref_spp, a.bounces, scene=sc, **opt)
                                              for sc in ("cornell", "checker") for _, opt in OPTION_SETS]
        if a.reps > 0:
            res["temporal_timing"] = temporal_timing(api, scenes, a.width, a.height, a.reps, a.bounces)
            res["temporal_option_timing"] = temporal_option_timing(api, scenes, a.width, a.height, a.reps, a.bounces)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
