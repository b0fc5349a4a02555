"""Searches (pixel, sample) stream keys whose draws, at the indices the surface materials consume, are extreme: writes
material_edge_keys.npz.  Run once, on the CPU, from the repository root:

    python tests/golden/find_material_edge_keys.py [processes]

Per draw index (the three draws after materials_common.DRAWS_CONSUMED) it keeps a few keys of each kind:
    tiny   0 < u < 1e-6
    big    0.9998 < u < 1.0 (engages the GGX sampler's 0.9999 clamp on sqrt(u1))
    one    u == 1.0 exactly (a u32 draw within 128 of 2^32 rounds to 2^32 as f32)
    zero   u == 0.0 exactly (the u32 draw is 0: one key in 2^32, hence the long search)
It also keeps four keys (nan_pdf_pixel, sample 0) under which materials_common.NAN_PDF_RAY gathers light on the plate of nan_pdf_scene and
then draws exactly 1.0 at the smooth dielectric sheet, beyond the critical angle: the oracle's first hit alone returns light, its whole
path exactly zero.
The fixture holds pixel, sample, index (absolute draw index), kind (0 tiny, 1 big, 2 one, 3 zero) and the u32 drawn;
test_materials_host.py re-derives every draw through the oracle's pto_wyrand, so a stale file fails loudly.
"""
import multiprocessing as mp
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import materials_common as MC  # noqa: E402

SEED = 0x5EED5EED
CHUNK = 1 << 16
KEEP = {0: 4, 1: 4, 2: 3, 3: 1}
KINDS = ("tiny", "big", "one", "zero")


def scan(task):
    sample, first_chunk, n_chunks = task
    found = []
    for c in range(first_chunk, first_chunk + n_chunks):
        pixel = np.arange(c * CHUNK, (c + 1) * CHUNK, dtype=np.uint64)
        s0 = MC.stream_state0(SEED, pixel, sample)
        for j in range(3):
            u = MC.wyrand_u32(s0, MC.DRAWS_CONSUMED + j)
            near = np.flatnonzero((u < 4400) | (u > 4294000000))          # a superset of every kind, so that the f32 tests run on few
            if near.size == 0:
                continue
            pixel_all, pixel, u = pixel, pixel[near], u[near]
            f = MC.u32_to_f32(u)
            for kind, hit in ((0, (f < np.float32(1e-6)) & (u != 0)), (1, (f > np.float32(0.9998)) & (f < np.float32(1.0))),
                              (2, f == np.float32(1.0)), (3, u == 0)):
                idx = np.flatnonzero(hit)[:KEEP[kind]] if kind < 2 else np.flatnonzero(hit)
                found += [(int(pixel[i]), sample, MC.DRAWS_CONSUMED + j, kind, int(u[i])) for i in idx]
            pixel = pixel_all
    return found


NAN_PDF_DRAW = MC.NAN_PDF_DRAW   # the sheet draws the ninth number of the stream


def scan_ones(first_chunk):
    found = []
    for c in range(first_chunk, first_chunk + 256):
        pixel = np.arange(c * CHUNK, (c + 1) * CHUNK, dtype=np.uint64)
        u = MC.wyrand_u32(MC.stream_state0(SEED, pixel, 0), NAN_PDF_DRAW)
        found += [int(pixel[i]) for i in np.flatnonzero(MC.u32_to_f32(u) == np.float32(1.0))]
    return found


def find_nan_pdf_keys(procs, want=4):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from oracle import oracle as O
    O.build()
    orc = O.Oracle(MC.nan_pdf_scene())
    o, d = MC.NAN_PDF_RAY
    keep = []
    with mp.Pool(procs) as pool:
        for found in pool.imap(scan_ones, range(0, (1 << 32) // CHUNK, 256)):
            for px in found:
                first = orc.integrate(o, d, px, 0, MC.DRAWS_CONSUMED, max_bounces=0)[0]
                whole = orc.integrate(o, d, px, 0, MC.DRAWS_CONSUMED, max_bounces=6)[0]
                if (first[:3] > 0).any() and (whole[:3] == 0).all():
                    keep.append(px)
            if len(keep) >= want:
                break
        pool.terminate()
    return np.array(keep[:want], np.uint32)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, (os.cpu_count() or 2) - 1)
    per_task = 256
    tasks = ((s, c, per_task) for s in range(1 << 20) for c in range(0, (1 << 32) // CHUNK, per_task))
    have = {}
    done = lambda: all(len(have.get((j, k), [])) >= KEEP[k] for j in range(3) for k in KEEP)
    with mp.Pool(procs) as pool:
        for n, found in enumerate(pool.imap_unordered(scan, tasks)):
            for px, sm, index, kind, u in found:
                rows = have.setdefault((index - MC.DRAWS_CONSUMED, kind), [])
                if len(rows) < KEEP[kind]:
                    rows.append((px, sm, index, kind, u))
            if n % 16 == 0:
                print(n * per_task * CHUNK, "keys;", {f"{KINDS[k]}{j}": len(v) for (j, k), v in sorted(have.items())}, flush=True)
            if done():
                break
        pool.terminate()
    nan_pdf = find_nan_pdf_keys(procs)
    rows = np.array(sorted(r for v in have.values() for r in v), np.uint64)
    np.savez(MC.EDGE_KEYS, pixel=rows[:, 0].astype(np.uint32), sample=rows[:, 1].astype(np.uint32), index=rows[:, 2].astype(np.uint32),
             kind=rows[:, 3].astype(np.uint32), u32=rows[:, 4].astype(np.uint32), seed=np.uint64(SEED), nan_pdf_pixel=nan_pdf)
    print("wrote", MC.EDGE_KEYS, len(rows), "keys")


if __name__ == "__main__":
    main()
