"""Shared by tests/test_gather_host.py and tests/test_gpu_gather.py: the baked rays and the final-gather bake of include/pt_api.h
(pt_baked_rays, pt_bake_lightmap_gather) composed from the restatements the tree already has.  Nothing here calls the library's device code:
the chain and its value are baked_common.baked over the oracle's trace_closest, the hop count and the first hit guides_follow_common.chains,
the rays lightmap_common.bake_rays, the light sample, its shadow ray and the fold lightmap_direct_common's."""
import numpy as np

import baked_common as BC
import guides_follow_common as G
import lightmap_common as LC
import lightmap_direct_common as LD

F = np.float32
UNLIT = (0.25, 0.5, 0.125)
HOPS = (0, 1, 2, 8)
# chosen on the RESTATEMENT (tests/test_gpu_gather.py asserts it): under this seed every ending of baked_common.ENDINGS ends at least 8 of
# the N_RAYS rays at max_hops = 2
RAY_SEED = 6
N_RAYS = 700


def room_rays(n=N_RAYS, seed=RAY_SEED):
    """n rays from inside baked_common.mapped_room: origins in a box around its camera, unit directions (binary32, used as given) towards
    points spread over the furniture in front of the back wall and, for one in eight, anywhere"""
    rng = np.random.default_rng(seed)
    o = rng.uniform((-3.0, -2.0, 9.0), (3.0, 4.0, 14.0), (n, 3)).astype(F)
    target = rng.uniform((-18.0, -8.0, -13.0), (14.0, 14.0, -5.0), (n, 3))
    glassy = rng.uniform((-16.0, -4.0, -12.0), (1.0, 4.0, -8.0), (n, 3))      # the two mirrors and the slab: the chains that go on
    i = np.arange(n)
    d = np.where((i % 2 == 0)[:, None], glassy, target) - o.astype(np.float64)
    anywhere = rng.normal(size=(n, 3))
    d = np.where((i % 8 == 7)[:, None], anywhere, d)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(F)
    return o, d


def chain_ends(orc, desc, o, d, max_hops):
    """(hops [n] the hop every chain ended at, id [n] uint8 the first hit's id byte: the model index's low byte, 255 for a miss)"""
    g = G.chains(orc, desc, o, d, max_hops)
    first = g["hop_model"][:, 0]
    return g["hops"].astype(np.uint32), np.where(first < 0, 255, first & 0xFF).astype(np.uint8)


def random_maps(sizes, seed):
    """seeded random maps {(model, ordinal): [h, w, 3]} for sizes {(model, ordinal): (w, h)}"""
    rng = np.random.default_rng(seed)
    return {key: rng.uniform(0.0, 1.0, (h, w, 3)).astype(F) for key, (w, h) in sizes.items()}


def table_of(desc, model, instance, w, h):
    m = desc.models[model]
    return LC.texels(m.positions, m.normals, m.uvs, m.matrices[instance], w, h)


def gather_samples(O, orc, desc, maps, table, n_samples, first_sample=0, key_base=0, bias=0.0, follow=0, unlit=(0.0, 0.0, 0.0), direct=True,
                   light_key_base=None):
    """every sample of a gather bake over a texel table, texel-major with a texel's samples consecutive: dict(k covered texel indices,
    X [c * n, 3], G (after the zeroing), D, B (the chains' values), zeroed, ending, hops, ids)"""
    h, w = table[0].shape
    k, o, d, keys, smp = LC.bake_rays(O, table, n_samples, first_sample, key_base, bias)
    B, ending = BC.baked(orc, desc, maps, o, d, follow, unlit)
    hops, ids = chain_ends(orc, desc, o, d, follow)
    out = dict(k=k, B=B, ending=ending, hops=hops, ids=ids)
    if not direct:
        out.update(X=B, G=B, D=np.zeros_like(B), zeroed=np.zeros(len(B), bool))
        return out
    if light_key_base is None:
        light_key_base = key_base + w * h
    nrm = np.repeat(table[3].reshape(-1, 3)[k], n_samples, 0)
    ls = LD.light_samples(LD.LightTable(orc, desc), np.repeat((k + light_key_base).astype(np.uint64), n_samples), smp, o, nrm)
    blocked = LD.shadowed(orc, o, ls)
    Dl = np.where((blocked | ~ls["cast"])[:, None], F(0.0), ls["ce"]).astype(F)
    zeroed = LD.emissive_ids(desc)[ids]
    Gz = np.where(zeroed[:, None], F(0.0), B).astype(F)
    X = Gz + Dl
    assert X.dtype == F
    out.update(X=X, G=Gz, D=Dl, zeroed=zeroed, blocked=blocked, cast=ls["cast"])
    return out


def fold(sums, sumsq, s, n_samples):
    return LD.fold(sums, sumsq, s["k"], s["X"], n_samples)


def mean_luminance(sums, cov, n):
    """the covered-texel mean luminance of a map of raw sums over n samples (binary64)"""
    return float(BC.luminance(np.asarray(sums, np.float64)[np.asarray(cov) != 0] / n).mean())
