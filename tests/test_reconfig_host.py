"""CPU: the host side of pt_set_config's contract (include/pt_api.h).  After every accepted step of the walk of tests/reconfig_common.py the
row table is the numpy model's and the host-evaluated rays (which read width, height, seed and n_sobol) are a fresh context's; a refused call
changes neither the library's configuration nor the wrapper's; and the walk itself holds the steps tests/test_gpu_reconfig.py needs.  No call
here needs a GPU."""
import numpy as np
import pytest

import reconfig_common as RC
from conftest import assert_bit_equal


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _cfg_fields(api, r):
    return {name: getattr(r.cfg, name) for name, _ in api.Config._fields_}


# ---------------------------------------------------------------------------------------------------------------- accepted calls
def test_rows_and_host_rays_after_every_step_are_a_fresh_contexts(api):
    cfgs = RC.configs()
    r = RC.renderer(api, cfgs[0])
    for i, ((kind, change), cfg) in enumerate(zip(RC.WALK, cfgs)):
        if i:
            r.set_config(**change)
        what = f"step {i} ({kind} {change})"
        want = RC.model_rows(cfg)
        assert r.local_rows().tolist() == want, what
        assert all(getattr(r.cfg, k) == v for k, v in cfg.items()), what
        fresh = RC.renderer(api, cfg)
        assert fresh.local_rows().tolist() == want, what + ", fresh"
        a, b = RC.host_products(r, cfg), RC.host_products(fresh, cfg)
        assert a.keys() == b.keys()
        for k in a:
            assert_bit_equal(a[k], b[k], f"{what}: {k}")
        fresh.close()
    r.close()


def test_the_host_rays_read_what_the_walk_changes(api):
    """the comparison above can fail: a new width, height, seed or n_sobol each changes some host-evaluated ray"""
    base = dict(RC.BASE)
    r0 = RC.renderer(api, base)
    for change in (dict(width=24, height=32), dict(seed=RC.SEED1), dict(n_sobol=64)):
        cfg = dict(base, **change)
        r1 = RC.renderer(api, cfg)
        # the same pixels and samples in both (those of the base frame: 768 pixels either way)
        a, b = RC.host_products(r0, base), RC.host_products(r1, base)
        assert any(a[k].tobytes() != b[k].tobytes() for k in a), change
        r1.close()
    r0.close()


# ----------------------------------------------------------------------------------------------------------------- refused calls
REFUSALS = [("width 0", dict(width=0)), ("height 0", dict(height=0)), ("rank = world_size", dict(world_size=2, rank=2)),
            ("rank beyond the world", dict(rank=5)), ("more than 2^31 - 1 pixels", dict(width=65536, height=65536)),
            ("more than 2^30 - 1 pixels on the rank", dict(width=40000, height=40000, world_size=1, rank=0)),
            ("a smaller frame and a bad rank", dict(width=8, height=8, rank=3, max_bounces=1, seed=1, n_sobol=64))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[n for n, _ in REFUSALS])
@pytest.mark.parametrize("start", [0, 9], ids=["one rank", "rank 1 of 2"])
def test_a_refused_call_changes_nothing(api, start, name, change):
    cfg = RC.configs()[start]
    r = RC.renderer(api, cfg)
    before_cfg, before_rows, before_rays = _cfg_fields(api, r), r.local_rows().tolist(), RC.host_products(r, cfg)
    with pytest.raises(api.PtError) as e:
        r.set_config(**change)
    assert e.value.code == RC.ERR_ARG
    # the wrapper first: every read method sizes its host buffers from it
    assert _cfg_fields(api, r) == before_cfg, f"{name}: the wrapper's cfg changed"
    assert r.local_rows().tolist() == before_rows == RC.model_rows(cfg), name
    after = RC.host_products(r, cfg)
    for k in before_rays:
        assert_bit_equal(after[k], before_rays[k], f"{name}: {k}")
    # ... and the context still takes an accepted call as a fresh one does
    r.set_config(max_bounces=2)
    assert r.cfg.max_bounces == 2 and r.local_rows().tolist() == before_rows
    r.close()


def test_an_unknown_field_is_an_error_not_a_silent_attribute(api):
    r = RC.renderer(api, RC.BASE)
    with pytest.raises(AttributeError):
        r.set_config(widht=16)
    assert r.cfg.width == 32
    r.close()


# ------------------------------------------------------------------------------------------------------- what each step must drop
def test_the_walk_holds_every_kind_of_step():
    drops = RC.drops()
    assert len(drops) == len(RC.WALK) - 1 and any(drops) and not all(drops)
    same = RC.same_count_steps()
    assert set(same) == {"shape", "rank", "strip"}, same        # 32 x 24 -> 24 x 32, rank 0 -> 1 of 2, strip_rows 4 -> 2
    cfgs = RC.configs()
    for kind, i in same.items():
        a, b = cfgs[i - 1], cfgs[i]
        assert a["width"] * len(RC.model_rows(a)) == b["width"] * len(RC.model_rows(b)) and RC.pixel_set(a) != RC.pixel_set(b), kind
    # the steps that keep the set change none of the five fields, or change them to the same effect
    for i, d in enumerate(drops, 1):
        if not d:
            assert RC.WALK[i][0] not in ("shape", "size", "shard", "rank", "strip"), RC.WALK[i]
    # every kind of step stands at least once right after a step of another kind
    kinds = [k for k, _ in RC.WALK]
    for k in set(kinds) - {"start"}:
        assert any(kinds[i] == k and kinds[i - 1] != k for i in range(1, len(kinds))), k
    # the steps the issue names
    flags = [c["flags"] for c in cfgs]
    for bit in (RC.FLAG_NO_LDS_SCENE, RC.FLAG_NO_PRIMARY_CULL, RC.FLAG_GENERAL_WALK, RC.FLAG_ADAPTIVE):
        on = [bool(f & bit) for f in flags]
        assert any(not a and b for a, b in zip(on, on[1:])) and any(a and not b for a, b in zip(on, on[1:])), bit
    assert [c["pipelines"] for c in cfgs if c["batch_spp"] == 1][:3] == [1, 1, 3] and 2 in [c["pipelines"] for c in cfgs]
    assert {c["max_bounces"] for c in cfgs} == {1, 3, 6} and {c["n_sobol"] for c in cfgs} == {512, 64}
    assert {(c["width"], c["height"]) for c in cfgs} == {(32, 24), (24, 32), (40, 24), (16, 12), (32, 16)}


def test_the_row_model_is_the_librarys_rule():
    """rows_of_rank (path_tracer_amd.dist) states the same rule; heights that are no multiple of the strip, more ranks than strips"""
    from path_tracer_amd.dist import rows_of_rank
    for h, world, strip in ((16, 2, 4), (16, 2, 2), (30, 3, 4), (7, 2, 4), (5, 4, 2), (24, 1, 4)):
        seen = []
        for rank in range(world):
            rows = RC.model_rows(dict(height=h, world_size=world, strip_rows=strip, rank=rank))
            assert rows == rows_of_rank(h, rank, world, strip).tolist()
            seen += rows
        assert sorted(seen) == list(range(h))
    assert RC.model_rows(dict(height=9, world_size=0, strip_rows=0, rank=0)) == list(range(9))
