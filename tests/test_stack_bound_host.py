"""CPU: the chain scenes of stack_bound_common reach the depths they are built for, under libptmi's builders and the oracle's alike, and the
designed rays drive every push discipline to the highest stack level it can reach there: the evidence, without a GPU, that
test_gpu_stack_bound.py would see an entry written one level too high or a bound one too small."""
import numpy as np
import pytest

import stack_bound_common as S
from conftest import assert_bit_equal

NAMES = ["blas_chain_left", "blas_chain_mirrored", "inline_limit_13", "blas_chain_right", "tlas_chain", "tlas_chain_mirrored", "ident_chain", "both_chains", "lights_chain", "forked"]
# the TLAS a scene's chain lives in, where max over the designed rays == reachable is demanded (elsewhere: <=)
CHAIN_TLAS = {"lights_chain": 1}
# reachable() per scene and discipline on that TLAS, MEASURED (closest, any, inline_any, fused_any) beside the bound of flatten's formula for that walk:
# the per-discipline gap of DESIGN.md section 2.  closest stops one short of the bound wherever a BLAS chain is on top (a followed triangle leaf is
# never pushed), the any-walks likewise; the fused launch's any-phase, which pushes both children of every node, reaches the bound exactly
REACH = {
    "blas_chain_left": ((28, 4, 4, 5), 29), "blas_chain_mirrored": ((28, 28, 28, 29), 29), "inline_limit_13": ((12, 12, 12, 13), 13), "blas_chain_right": ((61, 61, 61, 62), 62), "tlas_chain": ((17, 2, 2, 2), 17),
    "tlas_chain_mirrored": ((17, 2, 2, 2), 17), "ident_chain": ((17, 2, 2, 2), 17), "both_chains": ((41, 3, 3, 4), 42),
    "lights_chain": ((12, 2, 2, 2), 12),
}


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


@pytest.fixture(scope="module")
def built(api):
    """name -> (scene, renderer, Trees), built once"""
    cache = {}

    def get(name):
        if name not in cache:
            sc = S.scene(name)
            r = api.Renderer(sc, 16, 12)
            cache[name] = (sc, r, S.Trees(r, sc))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def walked(built):
    """(name, which, discipline) -> the WalkResults of every designed ray (closest: with t_max = +inf and with the ray's own)"""
    cache = {}

    def get(name, which, discipline):
        key = (name, which, discipline)
        if key not in cache:
            tr = built(name)[2]
            o, d, t = S.designed(name)
            rays = [(o[i], d[i], t[i]) for i in range(len(o))]
            if discipline == "closest":
                rays += [(o[i], d[i], np.inf) for i in range(len(o))]
            cache[key] = [S.walk(tr, which, ray, discipline) for ray in rays]       # a MarginError fails the test: no designed ray is dropped
        return cache[key]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_constructions_reach_their_depths(built, oracle_mod, name):
    sc, r, tr = built(name)
    o = oracle_mod.Oracle(sc)
    for b in range(r.blas_count()):
        a, c = r.blas_dump(b), o.blas_dump(b)
        for k in a:
            assert_bit_equal(np.asarray(a[k]), np.asarray(c[k]), f"{name} blas{b}.{k}")
    for which in (0, 1):
        a, c = r.tlas_dump(which), o.tlas_dump(which)
        for k in a:
            assert_bit_equal(np.asarray(a[k]), np.asarray(c[k]), f"{name} tlas{which}.{k}")
    dt = [tr.depth(t) for t in tr.tlas]
    db = max(tr.depth(b) for b in tr.blas)
    if name == "blas_chain_right":
        assert db >= 60 and dt == [1, 1] and tr.bound() == db      # the model is the only leaf of both TLASes
    elif name in ("blas_chain_left", "blas_chain_mirrored"):
        assert db == 28 and dt[0] == 2          # no overflow, no pure chain: what the SAH sweep makes of a 1 : 2 progression (0.44 levels per plate)
    elif name in ("tlas_chain", "tlas_chain_mirrored", "ident_chain"):
        assert dt[0] == tr.leaves(tr.tlas[0]) == 17 and db == 1
    elif name == "both_chains":
        assert dt[0] == tr.leaves(tr.tlas[0]) == S.BOTH_INSTANCES + 1 and db == 15 and tr.bound() >= 40
        mats = sc.models[0].matrices
        assert any((m[:, :3] == np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])).all() for m in mats)              # a quarter turn
        from path_tracer_amd.scene_desc import is_rigid
        assert all(is_rigid(m) for m in mats) and sum(1 for m in mats if 0.05 < abs(m[1, 2]) < 0.95) >= 4        # general rotations
    elif name == "lights_chain":
        assert dt[1] == tr.leaves(tr.tlas[1]) == S.LAMPS and dt[0] < dt[1]
        assert tr.bound() == dt[1]              # tlas_depth is the LIGHTS' depth here
    elif name == "inline_limit_13":
        assert tr.bound() == 13
    elif name == "forked":
        assert sc.models[0].positions.shape[0] >= 4096 and db >= 20


@pytest.mark.parametrize("levels", range(9, 17))
def test_inline_limit_scenes_have_the_levels_they_are_named_for(api, levels):
    sc = S.inline_limit(levels)
    assert S.Trees(api.Renderer(sc, 16, 12), sc).bound() == levels


def test_forked_and_single_thread_builds_agree(api, monkeypatch):
    """the depth the bound rests on comes from the SAH run's depth_out, forked subtrees included: the same tree and the same dumps whatever the thread count"""
    dumps = []
    for threads in ("1", "8"):
        monkeypatch.setenv("PTMI_BUILD_THREADS", threads)
        sc = S.scene("forked")
        r = api.Renderer(sc, 16, 12)
        dumps.append(r.blas_dump(0))
    for k in dumps[0]:
        assert_bit_equal(np.asarray(dumps[0][k]), np.asarray(dumps[1][k]), f"forked blas.{k}")


@pytest.mark.parametrize("discipline", S.DISCIPLINES)
@pytest.mark.parametrize("name", NAMES)
def test_designed_rays_reach_the_highest_level(built, walked, name, discipline):
    tr = built(name)[2]
    chain = CHAIN_TLAS.get(name, 0)
    for which in (0, 1):
        if tr.tlas[which]["kind"].size == 0:
            continue
        got = max(w.max_held for w in walked(name, which, discipline))
        reach = S.reachable(tr, which, discipline)
        bound = tr.bound_of(which)
        print(f"{name} tlas{which} {discipline}: designed rays hold {got}, reachable {reach}, bound of this walk {bound}, stack_entries {tr.bound()}")
        assert got <= reach <= bound <= tr.bound()
        if name == "forked" and which == 0:
            # the sweep splits the chain's large plates off together with the clump, so inside this model the 40 plates are a chain of 18 levels under a
            # clump of 22: the designed rays go down the plates (what they hold there is pinned), nothing is designed for the clump
            assert got == (16, 4, 4, 5)[S.DISCIPLINES.index(discipline)]
        if which == chain and name != "forked":
            assert got == reach
            want, want_bound = REACH[name]
            assert (reach, bound) == (want[S.DISCIPLINES.index(discipline)], want_bound)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "forked"])
def test_a_bound_one_lower_would_be_exceeded(built, walked, name):
    """the power of the GPU test, shown here: were the stack one entry shorter than what the walks reach, designed rays would write past it"""
    tr = built(name)[2]
    which = CHAIN_TLAS.get(name, 0)
    top = max(S.reachable(tr, which, d) for d in S.DISCIPLINES)
    over = [d for d in S.DISCIPLINES for w in walked(name, which, d) if w.max_held > top - 1]
    assert over, name
    # ... and the scene's stack_entries is reached to within the measured gap by SOME walk: the fused any-phase where a BLAS is on top, closest in a TLAS
    assert top >= tr.bound() - 1


@pytest.mark.parametrize("name", [n for n in NAMES if n != "forked"])
def test_every_split_of_the_stack_is_crossed(built, walked, name):
    """stack_lds_levels in {1, 2, E-1, E}: designed rays write AND read the last LDS level and the first spilled one (where a walk can reach them)"""
    tr = built(name)[2]
    which = CHAIN_TLAS.get(name, 0)
    e = tr.bound()
    for discipline in S.DISCIPLINES:
        reach = S.reachable(tr, which, discipline)
        written = set().union(*(w.written for w in walked(name, which, discipline)))
        read = set().union(*(w.read for w in walked(name, which, discipline)))
        for lds in (1, 2, e - 1, e):
            for level in (lds - 1, lds):
                if level < reach:
                    assert level in written, (name, discipline, lds, level)
                    # (an any-walk that ends on a hit leaves its entries unread: its top level may be one that only such a ray reaches)
                    assert level in read or (discipline != "closest" and level == reach - 1), (name, discipline, lds, level)
    levels = set().union(*(w.written for d in S.DISCIPLINES for w in walked(name, which, d)))
    assert e - 2 in levels      # the last LDS level of the split at E - 1, whatever the gap
    assert (e - 1 in levels) == (max(S.reachable(tr, which, d) for d in S.DISCIPLINES) == e)


def test_the_disciplines_differ(built, walked):
    """the any-walks push the left child and follow the right whatever the distances: a chain off left children never fills their stack, one off right
    children does; the closest walk follows the nearer child and fills it in both"""
    left = {d: max(w.max_held for w in walked("blas_chain_left", 0, d)) for d in S.DISCIPLINES}
    mirrored = {d: max(w.max_held for w in walked("blas_chain_mirrored", 0, d)) for d in S.DISCIPLINES}
    right = {d: max(w.max_held for w in walked("blas_chain_right", 0, d)) for d in S.DISCIPLINES}
    e_left, e_right = built("blas_chain_left")[2].bound(), built("blas_chain_right")[2].bound()
    assert left["closest"] == e_left - 1 and left["any"] <= 5 and left["inline_any"] <= 5
    assert mirrored == {"closest": e_left - 1, "any": e_left - 1, "inline_any": e_left - 1, "fused_any": e_left}      # the same tree, left and right exchanged
    assert right["closest"] == right["any"] == right["inline_any"] == e_right - 1 and right["fused_any"] == e_right
    # PT_BRANCH_LEVELS: the 4-level and the 6-level walk push the followed child at different levels of the same chain
    wa = set().union(*(frozenset(w.written) for w in walked("blas_chain_right", 0, "any")))
    assert wa == set(range(e_right - 1))


def test_margin_is_enforced():
    """a ray that grazes a box face is refused, not decided"""
    box = np.array([0, 0, 0, 1, 1, 1], np.float64)
    with pytest.raises(S.MarginError):
        S._slab(box, np.array([-1.0, 0.5, 1.0 + 1e-5]), np.array([1.0, 0.0, 0.0]), np.inf, "graze")
    with pytest.raises(S.MarginError):
        S._slab(box, np.array([-1.0, -1.0, 0.5]), np.array([1.0, 0.5 * (1 + 1e-5), 0.0]), np.inf, "edge")
    assert S._slab(box, np.array([-1.0, 0.5, 0.5]), np.array([1.0, 0.0, 0.0]), np.inf, "through") == (True, 1.0)
