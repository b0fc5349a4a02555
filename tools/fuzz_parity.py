"""Extended randomized parity run (not part of the test suite): random scenes, per-sample radiance + frame + ray tallies, GPU vs oracle.
Usage: python tools/fuzz_parity.py [--media] [--identity] [first_seed] [n_seeds] [width height]   (default: tiny frames, 40x24 / 64x20; a few hundred
pixels a side exercise the striped tails, tapered chunks and dynamic claims that tiny queues never reach).
--media: scenes.media_scene (2-9 overlapping / nested volume-bearing models, shared materials, instances).  A scene in which the oracle
sees a path inside more than 8 volumes must fail with PT_ERR_LIMIT instead (counted apart, not a mismatch).
--identity: every model is instanced once, by the identity: the scenes whose TLASes the one-ray walk (IDENT kernels) takes."""
import dataclasses
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from oracle import oracle as O
from path_tracer_amd import api, scenes

media = "--media" in sys.argv
if media:
    sys.argv.remove("--media")
identity = "--identity" in sys.argv
if identity:
    sys.argv.remove("--identity")
first = int(sys.argv[1]) if len(sys.argv) > 1 else 100
count = int(sys.argv[2]) if len(sys.argv) > 2 else 40
size = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else None
every = 500 if size is None else 20
O.build()


def bits(a):
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


bad = 0
too_deep = 0
depths = {}
n_general = 0   # instance matrices that are rotations about a general axis (nine non-zero entries), summed over the scenes
with_general = 0
n_ident = 0     # scenes whose world and lights TLAS both took the one-ray walk
t0 = time.time()
for seed in range(first, first + count):
    w, h = size if size else ((40, 24) if seed % 3 else (64, 20))
    sc = scenes.media_scene(seed, w, h) if media else scenes.random_scene(seed, w, h, with_media=(seed % 2 == 0))
    if identity:
        from path_tracer_amd.scene_desc import IDENTITY_3x4
        sc = dataclasses.replace(sc, models=[dataclasses.replace(m, matrices=IDENTITY_3x4[None].copy()) for m in sc.models])
    g = sum(int(np.count_nonzero(m[:, :3]) > 3) for mo in sc.models for m in mo.matrices)
    n_general += g
    with_general += 1 if g else 0
    o = O.Oracle(sc)
    # every fourth scene keeps its BVH in global memory (the kernels the mesh configurations run)
    r = api.Renderer(sc, w, h, max_bounces=6 + seed % 9, flags=api.FLAG_NO_LDS_SCENE if seed % 4 == 3 else 0)
    mb = 6 + seed % 9
    if media:
        octr = o.render(w, h, 3, max_bounces=mb)[3]
        depths[int(octr[8])] = depths.get(int(octr[8]), 0) + 1
        if octr[8] > 8:
            try:
                r.render(0, 3)
                ok = False
            except api.PtError as e:
                ok = e.code == -5
            too_deep += 1
            if not ok:
                bad += 1
                print("MISMATCH (no PT_ERR_LIMIT beyond 8 volumes) seed", seed, flush=True)
            r.close()
            continue
    ok = np.array_equal(bits(r.render_samples(0, 3)), bits(o.render_samples(w, h, 3, max_bounces=mb)))
    r.reset_stats(); r.reset_accumulation()
    acc, pos, idb = r.render(3, 2)
    oacc, opos, oid, octr = o.render(w, h, 2, first_sample=3, max_bounces=mb)
    st = r.stats()
    n_ident += st.ident_tlas == 3
    ok = ok and np.array_equal(bits(acc), bits(oacc)) and np.array_equal(bits(pos), bits(opos)) and np.array_equal(idb, oid)
    ok = ok and (st.rays_closest, st.rays_any, st.rays_light_closest) == (int(octr[0]), int(octr[1]), int(octr[2]))
    if not ok:
        bad += 1
        print("MISMATCH seed", seed, flush=True)
    r.close()
    if (seed - first + 1) % every == 0:
        print(f"{seed - first + 1} scenes so far, {bad} mismatches, {time.time() - t0:.1f} s", flush=True)
if media:
    print(f"deepest volume stack per scene: {dict(sorted(depths.items()))}; {too_deep} beyond 8 (PT_ERR_LIMIT checked)")
print(f"{count} scenes ({with_general} with at least one general rigid instance, {n_general} such instances in all; {n_ident} on the one-ray walk), {bad} mismatches, {time.time() - t0:.1f} s")
sys.exit(1 if bad else 0)
