"""GPU (-m gpu): instances of a built scene moved with pt_set_instances + pt_build, and pt_frame_moving.  A moved scene IS a fresh scene with
other matrices: every expected value comes from an oracle scene built from nothing with the matrices of that step; the motion-aware frame is
composed from the oracle's render, post_velocity and post_reproject and the numpy restatement of x_prev in tests/test_instances_host.py.
Everything is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from instances_common import QUARTER_X, QUARTER_Y, apply, chain, move, placed, shifted
from test_instances_host import case_exact, case_hand_worked, case_untouched, x_prev_numpy

pytestmark = pytest.mark.gpu

F = np.float32
W, H, DEPTH = 48, 32, 4
MISS = 0xFFFFFFFF
I34 = np.eye(3, 4, dtype=np.float32)


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _rays(box, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    ext = hi - lo
    o = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d = (d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]).astype(F)
    tmax = np.where(np.arange(n) % 3 == 0, np.inf, rng.uniform(50, 800, n)).astype(F)
    key = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sample = rng.integers(0, 2000, n).astype(np.uint32)
    return o, d, tmax, key, sample


def _expected(O, desc, box, probes):
    """what a scene built from nothing with these matrices gives, all from the oracle"""
    o = O.Oracle(desc)
    e = {}
    e["samples"] = o.render_samples(W, H, 2, first_sample=3, max_bounces=DEPTH)
    e["acc"], e["pos"], e["id"], e["ctr"] = o.render(W, H, 3, max_bounces=DEPTH)
    ro, rd, tmax, key, sample = _rays(box, 2048, 17)
    e["closest"] = [o.trace_closest(ro, rd, None, which) for which in (0, 1)]
    e["any"] = [o.trace_any(ro, rd, tmax, which) for which in (0, 1)]
    n = 96
    rad = np.zeros((n, 4), F); pos = np.zeros((n, 4), F); idb = np.zeros(n, np.uint8)
    for i in range(n):
        rad[i], pos[i], idb[i] = o.integrate(ro[i], rd[i], int(key[i]), int(sample[i]), 1, max_bounces=DEPTH)
    e["rays"] = (rad, pos, idb)
    if probes is not None:
        from test_rays_host import probe_rays
        count = 8
        keys = np.repeat(np.arange(len(probes)) + 50, count); samples = np.tile(np.arange(count), len(probes))
        d, y = probe_rays(O, keys, samples)
        sh = np.zeros((len(probes), 9, 3), F)
        prad = np.zeros((len(keys), 4), F)
        for i in range(len(keys)):
            prad[i] = o.integrate(np.repeat(probes, count, 0)[i], d[i], int(keys[i]), int(samples[i]), 1, max_bounces=DEPTH)[0]
        prad = prad.reshape(len(probes), count, 4); y = y.reshape(len(probes), count, 9)
        for s in range(count):
            sh = sh + prad[:, s, None, :3] * y[:, s, :, None]
        e["sh"] = sh
    return e


def _check(r, e, box, probes, what):
    assert_bit_equal(r.render_samples(3, 2), e["samples"], what + ": render_samples")
    r.reset_accumulation(); r.reset_stats()
    acc, pos, idb = r.render(0, 3)
    assert_bit_equal(acc, e["acc"], what + ": accumulation"); assert_bit_equal(pos, e["pos"], what + ": position")
    assert np.array_equal(idb, e["id"]), what + ": id"
    st = r.stats()
    assert (st.rays_closest, st.rays_any, st.rays_light_closest) == tuple(int(x) for x in e["ctr"][:3]), what + ": ray tallies"
    ro, rd, tmax, key, sample = _rays(box, 2048, 17)
    for which in (0, 1):
        got = r.trace_closest(ro, rd, None, which)
        for k in ("t", "u", "v", "inst", "prim"):
            assert_bit_equal(got[k], e["closest"][which][k], f"{what}: trace_closest[{which}].{k}")
        assert np.array_equal(r.trace_any(ro, rd, tmax, which), e["any"][which]), f"{what}: trace_any[{which}]"
    n = len(e["rays"][2])
    rad, rpos, rid = r.integrate_rays(ro[:n], rd[:n], key[:n], sample[:n], draws_consumed=1)
    assert_bit_equal(rad, e["rays"][0], what + ": integrate_rays radiance"); assert_bit_equal(rpos, e["rays"][1], what + ": integrate_rays position")
    assert np.array_equal(rid, e["rays"][2]), what + ": integrate_rays id"
    if probes is not None:
        assert_bit_equal(r.bake_probes(probes, 8, key_base=50), e["sh"], what + ": bake_probes")


_CACHE = {}
BOX = np.array([-700, -700, -700, 700, 700, 700], F)     # rays start in and around the room wherever its models have been moved to
# batch_spp=1 cuts a 3-sample render into three batches, which alternate over the two default pipelines (a whole 48 x 32 frame is one batch
# and would run on one); pipelines=1 is strictly one batch after another
CONTEXTS = [dict(batch_spp=1), dict(flags=2, batch_spp=1), dict(pipelines=1), dict(flags=2, pipelines=1)]


def _pipelines_of_a_render(r, monkeypatch, capfd):
    """how many pipelines the library's batch plan gives render(0, 3), from its own PTMI_DEBUG_BATCH line"""
    import re
    capfd.readouterr()
    monkeypatch.setenv("PTMI_DEBUG_BATCH", "1")
    r.reset_accumulation()
    r.render(0, 3)
    monkeypatch.delenv("PTMI_DEBUG_BATCH")
    m = re.findall(r"batch \d+ x (\d+) on (\d+) pipelines", capfd.readouterr().err)
    assert m, "no batch plan line"
    return int(m[-1][0]), int(m[-1][1])


def _chain_case(name):
    from path_tracer_amd import scenes
    desc = scenes.cornell_instanced(W, H) if name == "cornell_instanced" else scenes.random_scene(int(name[6:]), W, H)
    steps = chain(desc, 5)
    descs = []
    d = desc
    for step in steps:
        d = apply(d, step)
        descs.append(d)
    return desc, steps, descs


@pytest.mark.parametrize("name,ctx", [("cornell_instanced", 0), ("cornell_instanced", 1), ("cornell_instanced", 2), ("cornell_instanced", 3), ("random3", 0),
                                      ("random3", 1), ("random11", 3)])
def test_a_moved_scene_is_a_fresh_scene(api, oracle_mod, monkeypatch, capfd, name, ctx):
    """every step of the chain (one model, all models, identity -> general -> identity, 1 -> 3 -> 0 -> 2 instances, the emissive model):
    render_samples, render (accumulation, position, id, tallies), trace_closest / trace_any on both TLASes, integrate_rays and one bake_probes
    equal the oracle built fresh with those matrices, with the BVH in LDS and in global memory, on one and on two pipelines"""
    desc, steps, descs = _chain_case(name)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH, **CONTEXTS[ctx])
    r.render(0, 1)                                                  # the scene is resident before the first move
    n_models = len(desc.models)
    probes = np.array([[0, 0, 0], [100, -100, 50], [-150, 200, -100]], F)
    for k, step in enumerate(steps):
        move(r, step)
        if (name, k) not in _CACHE:
            _CACHE[(name, k)] = _expected(oracle_mod, descs[k], BOX, probes if k == 3 else None)
        _check(r, _CACHE[(name, k)], BOX, probes if k == 3 else None, f"{name} step {k} ({CONTEXTS[ctx]})")
        assert r.scene_info().blas_builds == n_models
    info = r.scene_info()
    assert info.uploads_patched >= 4 and info.uploads_full >= 2, info.as_dict()   # both paths were taken along the chain
    assert _pipelines_of_a_render(r, monkeypatch, capfd) == ((3, 2) if "batch_spp" in CONTEXTS[ctx] else (1, 1))


def _depth(d):
    if len(d["kind"]) == 0:
        return 0
    children = {i: (int(d["a"][i]), int(d["b"][i])) for i in range(len(d["kind"])) if d["kind"][i] == 0}
    stack, best = [(int(d["root"]), 1)], 0
    while stack:
        i, n = stack.pop()
        best = max(best, n)
        if i in children:
            stack += [(children[i][0], n + 1), (children[i][1], n + 1)]
    return best


def test_a_patch_that_deepens_the_tlas_creates_the_spill_area(api, oracle_mod, monkeypatch, capfd, cornell64):
    """eight short boxes bunched in the room, then strung out along x at doubling distances: the agglomerative TLAS degenerates into a chain.
    stack_lds_levels is set to what the bunched scene needs, so the first build spills nothing and the patch has to create the spill area,
    which batches on two pipelines then use side by side"""
    near = np.stack([placed(I34, (x, 0, z)) for x in (-60, -20, 20, 60) for z in (-30, 30)])
    line = np.stack([placed(I34, (100.0 * 2 ** k, 0, 0)) for k in range(8)])
    desc = apply(cornell64, [(5, near)])
    probe = api.Renderer(desc, W, H, max_bounces=DEPTH)
    probe.render(0, 1)
    need = probe.stats().stack_entries
    d0 = _depth(probe.tlas_dump(0))
    probe.close()
    for flags in (0, 2):
        r = api.Renderer(desc, W, H, max_bounces=DEPTH, stack_lds_levels=need, flags=flags, batch_spp=1)   # three batches over two pipelines
        r.render(0, 3)
        assert r.stats().stack_entries == need
        move(r, [(5, line)])
        assert _depth(r.tlas_dump(0)) > d0
        moved = apply(desc, [(5, line)])
        if "deep" not in _CACHE:
            _CACHE["deep"] = _expected(oracle_mod, moved, np.array([-700, -700, -700, 13500, 700, 700], F), None)
        _check(r, _CACHE["deep"], np.array([-700, -700, -700, 13500, 700, 700], F), None, f"deepened TLAS, flags {flags}")
        info = r.scene_info()
        assert (info.uploads_full, info.uploads_patched) == (1, 1), info.as_dict()
        assert r.stats().stack_entries > need                                # deeper than the LDS levels: the walk spills, correctly
        assert _pipelines_of_a_render(r, monkeypatch, capfd) == (3, 2)       # ... in the spill regions of two pipelines


def test_atrium_with_three_columns_toppled_between_two_renders(api, oracle_mod):
    from path_tracer_amd import scenes
    Wa, Ha = 64, 36
    desc = scenes.atrium(Wa, Ha, statue_level=0)
    r = api.Renderer(desc, Wa, Ha, max_bounces=DEPTH)
    o = oracle_mod.Oracle(desc)
    acc, pos, idb = r.render(0, 2)
    oacc, opos, oid, _ = o.render(Wa, Ha, 2, max_bounces=DEPTH)
    assert_bit_equal(acc, oacc, "atrium before"); assert_bit_equal(pos, opos, "atrium before: position"); assert np.array_equal(idb, oid)
    state = r.stats().state_bytes
    step = []
    for mi, q, t in ((7, (2, -1, -2, 3), (-100.0, 60.0, 200.0)), (8, (3, 2, -1, 3), (90.0, 70.0, -100.0)), (9, (4, -2, 2, 6), (-40.0, 80.0, -400.0))):
        mats = desc.models[mi].matrices.copy()
        mats[0] = scenes.rigid_from_quat(*q, t)                              # an upright column of each of three variants, toppled into the aisle
        step.append((mi, mats))
    move(r, step)
    r.reset_accumulation()
    acc, pos, idb = r.render(0, 2)
    oacc, opos, oid, _ = oracle_mod.Oracle(apply(desc, step)).render(Wa, Ha, 2, max_bounces=DEPTH)
    assert_bit_equal(acc, oacc, "atrium toppled"); assert_bit_equal(pos, opos, "atrium toppled: position"); assert np.array_equal(idb, oid)
    info = r.scene_info()
    assert (info.blas_builds, info.uploads_full, info.uploads_patched) == (len(desc.models), 1, 1), info.as_dict()
    n_inst = [len(r.tlas_instances(w)["matrix"]) for w in (0, 1)]
    assert info.last_upload_bytes == 32 * sum(2 * n - 1 for n in n_inst) + 144 * sum(n_inst)
    assert r.stats().state_bytes == state


def test_which_path_ran(api, cornell64):
    r = api.Renderer(cornell64, W, H, max_bounces=DEPTH)
    r.render(0, 1)
    info = r.scene_info()
    assert (info.blas_builds, info.tlas_builds, info.uploads_full, info.uploads_patched) == (6, 1, 1, 0)
    full_bytes = info.last_upload_bytes
    st = r.stats()
    state = st.state_bytes
    assert st.ident_tlas == 3                                               # every instance an identity: both TLASes on the one-ray walk
    n_nodes = [len(r.tlas_dump(w)["kind"]) for w in (0, 1)]
    n_inst = [len(r.tlas_instances(w)["matrix"]) for w in (0, 1)]
    assert n_nodes == [2 * n - 1 for n in n_inst]
    patch = 32 * sum(n_nodes) + 144 * sum(n_inst)
    for k, (mats, ident) in enumerate([(shifted(I34, (30, 0, -10)), 2), (placed(QUARTER_Y, (0, 0, 0))[None], 2), (I34[None], 3)]):
        move(r, [(5, mats)])
        r.render(0, 1)
        info = r.scene_info()
        assert (info.blas_builds, info.tlas_builds, info.uploads_full, info.uploads_patched) == (6, k + 2, 1, k + 1), info.as_dict()
        assert info.last_upload_bytes == patch and patch < full_bytes
        st = r.stats()
        assert st.state_bytes == state and st.ident_tlas == ident, (k, st.ident_tlas)
    before = r.scene_info().as_dict()
    frame = r.render_samples(0, 1)
    bad = I34[None].copy(); bad[0, 1, 1] = 3.0
    for model, mats in ((5, bad), (99, I34[None])):                          # refused: the scene stays built, resident and renders as before
        with pytest.raises(api.PtError):
            r.set_instances(model, mats)
    assert_bit_equal(r.render_samples(0, 1), frame, "render after refused moves")
    assert r.scene_info().as_dict() == before
    move(r, [(0, shifted(cornell64.models[0].matrices, (0, -5, 0)))])       # the light is a leaf of both TLASes: neither is all-identity now
    r.render(0, 1)
    assert r.stats().ident_tlas == 0 and r.scene_info().uploads_patched == 4
    move(r, [(5, np.stack([I34, shifted(I34, (0, 100, 0))[0]]))])           # a count change: everything moves in the blob
    r.render(0, 1)
    info = r.scene_info()
    assert (info.blas_builds, info.uploads_full, info.uploads_patched) == (6, 2, 4), info.as_dict()
    assert info.last_upload_bytes > full_bytes
    move(r, [(5, np.stack([I34, shifted(I34, (0, 120, 0))[0]]))])           # and the new layout is patched in turn
    r.render(0, 1)
    assert (r.scene_info().uploads_full, r.scene_info().uploads_patched) == (2, 5)


def _primary(o, k):
    ro = np.zeros((W * H, 3), F); rd = np.zeros((W * H, 3), F)
    for p in range(W * H):
        ro[p], rd[p] = o.primary_ray(W, H, p, k)
    return ro, rd


def test_guides_go_stale_and_the_instance_guide_names_the_leaf(api, oracle_mod):
    from path_tracer_amd import scenes
    desc = scenes.cornell_instanced(W, H)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH)
    r.render(0, 2)
    r.render_guides(1)
    r.denoise()
    step = [(4, shifted(desc.models[4].matrices, (15, 5, -10))), (6, desc.models[6].matrices[::-1].copy())]
    move(r, step)
    with pytest.raises(api.PtError) as e:
        r.denoise()
    assert e.value.code == -3 and "stale" in str(e.value)
    r.render_guides(1)
    inst = r.read_guide_instances()
    pos, _, model = r.read_guides()
    o = oracle_mod.Oracle(apply(desc, step))
    ro, rd = _primary(o, 1)
    want = o.trace_closest(ro, rd)
    assert np.array_equal(inst.reshape(-1), want["inst"])
    assert_bit_equal(pos[..., 3].reshape(-1), np.where(want["inst"] == MISS, F(1e5), want["t"]).astype(F), "guide t")
    hit = inst != MISS
    assert hit.any()
    blas = r.instance_materials(0)["blas"]
    assert np.array_equal(model[hit], blas[inst[hit]]) and (model[~hit] == MISS).all()
    assert len(np.unique(inst[hit])) > 6                                    # several instances of one model are told apart


@pytest.mark.parametrize("w,h", [(48, 32), (1, 1), (37, 19)])
def test_post_motion_kernel(api, cornell64, w, h):
    r = api.Renderer(cornell64, 16, 16)
    from path_tracer_amd import scenes
    rng = np.random.default_rng(w * 7 + h)
    n = 9
    cur = np.stack([scenes.general_turn(rng) for _ in range(n)]); prv = np.stack([scenes.general_turn(rng) for _ in range(n)])
    inv = np.stack([scenes.general_turn(rng) for _ in range(n)])           # any table: the kernel multiplies what it is given
    prv[2] = cur[2]
    has = np.ones(n, np.uint8); has[5] = 0
    pos = rng.uniform(-600, 600, (h, w, 4)).astype(F)
    inst = rng.integers(0, n + 1, (h, w)).astype(np.uint32)
    inst[inst == n] = MISS
    want = x_prev_numpy(pos, inst, cur, inv, prv, has)
    got = r.post_motion(pos, inst, cur, inv, prv, has)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if w * h > 100:
        moved = (got[..., :3] != pos[..., :3]).any(-1)
        assert moved.any() and not moved[(inst == 2) | (inst == 5) | (inst == MISS)].any()
        args, exact = case_exact()
        assert np.array_equal(r.post_motion(*args).view(np.uint32), exact.view(np.uint32))
        args, exact = case_hand_worked()
        assert np.array_equal(r.post_motion(*args).view(np.uint32), exact.view(np.uint32))
        for flag in (True, False):
            args = case_untouched(flag)
            got = r.post_motion(*args); want = x_prev_numpy(*args)
            # untouched points come back with the very bits (a NaN's payload included); computed ones as conftest.bits compares them
            keep = np.array([[True, True, not flag]])
            assert np.array_equal(got[keep].view(np.uint32), args[0][keep].view(np.uint32))
            assert_bit_equal(got, want, "moved point through NaN / -0")


def _moved_cam(cam, dx):
    from path_tracer_amd.scene_desc import Camera
    return Camera.new((cam.origin[0] + dx, cam.origin[1], cam.origin[2] - 2 * dx), (cam.target[0] + 0.3 * dx, cam.target[1], cam.target[2]),
                      cam.fov, cam.aspect_ratio)


def test_frame_moving_equals_frame_where_nothing_moved(api, cornell64):
    """the sequence of test_frame_sequence_static_then_moving_camera (three frames at rest, three with the camera moving), word for word"""
    a = api.Renderer(cornell64, 64, 64, max_bounces=4); b = api.Renderer(cornell64, 64, 64, max_bounces=4)
    cams = [cornell64.camera] * 3 + [_moved_cam(cornell64.camera, d) for d in (8.0, 20.0, 20.0)]
    id_a = np.zeros((64, 64), np.uint32); id_b = np.zeros((64, 64), np.uint32)
    last = a.inv_projection()
    for k, cam in enumerate(cams):
        a.set_camera(cam); b.set_camera(cam)
        da, pa, id_a = a.frame(k, last, id_a)
        db, pb, id_b = b.frame_moving(k, last, id_b)
        assert_bit_equal(db, da, f"frame {k} data"); assert_bit_equal(pb, pa, f"frame {k} position"); assert np.array_equal(id_b, id_a)
        assert_bit_equal(b.read_accumulation(), a.read_accumulation(), f"frame {k} accumulation")
        last = a.inv_projection()
    assert_bit_equal(b.present(), a.present(), "present")
    b.rebuild()                                                             # a rebuild that moved nothing is still nothing moved
    da, pa, id_a = a.frame(6, last, id_a); db, pb, id_b = b.frame_moving(6, last, id_b)
    assert_bit_equal(b.read_accumulation(), a.read_accumulation(), "after an idle rebuild")


def _run_moving(api, O, desc0, poses, cams, box_model=5):
    """poses[k]: matrices of `box_model` in frame k (None: as in the frame before); cams[k]: the camera of frame k.  The expected frame: input,
    position and id history from a fresh oracle scene per pose; x_prev from the test's restatement on the oracle's instance image; velocity =
    post_velocity(x_prev | t), output = post_reproject"""
    r = api.Renderer(desc0, W, H, max_bounces=DEPTH)
    desc = apply(desc0, [])                                                  # (a copy: the camera is set on it below)
    acc = np.zeros((H, W, 4), F)
    id_g = np.zeros((H, W), np.uint32); id_o = np.zeros((H, W), np.uint32)
    last = O.Oracle(desc0).inv_projection()
    prev_tables = None
    branches = []
    for k, (pose, cam) in enumerate(zip(poses, cams)):
        if pose is not None:
            desc = apply(desc, [(box_model, pose)])
            move(r, [(box_model, pose)])
        desc.camera = cam
        r.set_camera(cam)
        o = O.Oracle(desc)
        data_g, pos_g, id_g = r.frame_moving(k, last, id_g)
        data_o, pos_o, id_o, _ = o.render(W, H, 1, first_sample=k, max_bounces=DEPTH, ident=id_o)
        assert_bit_equal(data_g, data_o, f"frame {k} data"); assert_bit_equal(pos_g, pos_o, f"frame {k} position"); assert np.array_equal(id_g, id_o)
        tabs = o.tlas_instances(0)
        models = r.instance_materials(0)["blas"]
        cur_o = o.inv_projection()
        cam_moved = not np.array_equal(cur_o, last)
        world_moved, same_count = False, True
        if prev_tables is not None:
            same_count = len(prev_tables[0]) == len(tabs["matrix"])          # (only box_model ever changes its count here)
            world_moved = (not same_count) or prev_tables[0].tobytes() != tabs["matrix"].tobytes()
        if not (cam_moved or world_moved):
            acc = O.post_accumulate(data_o, acc); branches.append("accumulate")
        else:
            x_prev = pos_o
            if world_moved:
                ro, rd = _primary(o, k)
                inst = o.trace_closest(ro, rd)["inst"].reshape(H, W)
                assert np.array_equal(r.read_guide_instances(), inst), f"frame {k}: instance guide"
                if same_count:
                    prv, has = prev_tables[0], np.ones(len(models), np.uint8)
                else:                                                        # the model whose count changed has no previous matrices
                    prv, has = tabs["matrix"], (models != box_model).astype(np.uint8)
                    assert all(np.array_equal(tabs["matrix"][i], prev_tables[0][j]) for i, j in
                               zip(np.flatnonzero(models != box_model), np.flatnonzero(prev_tables[1] != box_model)))
                x_prev = x_prev_numpy(pos_o, inst, tabs["matrix"], tabs["inv_matrix"], prv, has)
                assert_bit_equal(r.post_motion(pos_o, inst, tabs["matrix"], tabs["inv_matrix"], prv, has), x_prev, f"frame {k}: post_motion")
                on_box = (inst != MISS) & (models[np.minimum(inst, len(models) - 1)] == box_model)
                vel = O.post_velocity(x_prev, last)
                assert_bit_equal(vel[~on_box], O.post_velocity(pos_o, last)[~on_box], f"frame {k}: velocity off the moved model is frame's")
                if same_count:
                    assert on_box.any() and not np.array_equal(vel[on_box], O.post_velocity(pos_o, last)[on_box])
                else:
                    assert np.array_equal(x_prev.view(np.uint32), pos_o.view(np.uint32))
            acc = O.post_reproject(data_o, acc, O.post_velocity(x_prev, last), id_o); branches.append("reproject")
        assert_bit_equal(r.read_accumulation(), acc, f"frame {k} accumulation ({branches[-1]})")
        prev_tables = (tabs["matrix"].copy(), models.copy())
        last = cur_o
        assert_bit_equal(r.inv_projection(), last, "inv_projection")
    return r, branches


def _poses():
    from path_tracer_amd import scenes
    rng = np.random.default_rng(12)
    g1 = scenes.general_turn(rng, 30); g2 = scenes.general_turn(rng, 30)
    return [None, shifted(I34, (25, 0, -15)), g1[None], None, g2[None], shifted(I34, (-10, 0, 5))]


def test_frame_moving_static_camera_box_through_four_poses(api, oracle_mod, cornell64):
    cam = cornell64.camera
    _, branches = _run_moving(api, oracle_mod, cornell64, _poses(), [cam] * 6)
    assert branches == ["accumulate", "reproject", "reproject", "accumulate", "reproject", "reproject"]


def test_frame_moving_camera_and_box_both_moving(api, oracle_mod, cornell64):
    cam = cornell64.camera
    cams = [cam, cam, _moved_cam(cam, 8.0), _moved_cam(cam, 20.0), _moved_cam(cam, 20.0), _moved_cam(cam, 26.0)]
    _, branches = _run_moving(api, oracle_mod, cornell64, _poses(), cams)
    assert branches == ["accumulate"] + ["reproject"] * 5


def test_frame_moving_instance_count_change_reprojects_with_x(api, oracle_mod, cornell64):
    cam = cornell64.camera
    poses = [None, None, np.stack([I34, shifted(I34, (0, 110, 0))[0]]), None, I34[None]]
    _, branches = _run_moving(api, oracle_mod, cornell64, poses, [cam] * 5)
    assert branches == ["accumulate", "accumulate", "reproject", "accumulate", "reproject"]


def _one_of_several():
    """poses of cornell_instanced's four-instance box model in which only its third instance moves (leaf 6 of the world TLAS)"""
    from path_tracer_amd import scenes
    base = scenes.cornell_instanced(W, H).models[4].matrices
    a = base.copy(); a[2] = shifted(base[2], (-20, 15, 10))[0]
    b = a.copy(); b[2] = scenes.rigid_from_quat(2, -5, -3, 4, (25.0, -130.0, 140.0))
    return [None, a, b, None]


def test_frame_moving_one_instance_of_several(api, oracle_mod):
    """the previous matrix of a leaf is matrix j of ITS model: a model with four instances of which the third moves, behind four models with
    one instance each and before one with two"""
    from path_tracer_amd import scenes
    desc = scenes.cornell_instanced(W, H)
    r, branches = _run_moving(api, oracle_mod, desc, _one_of_several(), [desc.camera] * 4, box_model=4)
    assert branches == ["accumulate", "reproject", "reproject", "accumulate"]
    inst = r.read_guide_instances()
    assert (inst == 6).any() and (inst == 4).any() and (inst == 7).any()          # the moved leaf and its siblings are all in view


def test_frame_moving_leaves_the_guides_valid(api, cornell64):
    r = api.Renderer(cornell64, W, H, max_bounces=DEPTH)
    r.frame_moving(0)
    move(r, [(5, shifted(I34, (20, 0, 0)))])
    _, pos, _ = r.frame_moving(1)
    first = r.denoise()                                                      # the recipe: frame_moving(k), denoise
    gpos = r.read_guides()[0]
    assert_bit_equal(gpos, pos, "the guides are this sample's")
    r.render_guides(1)
    assert_bit_equal(r.denoise(), first, "frame_moving(k), render_guides(k), denoise")


def test_multi_renders_the_moved_scene(api, cornell64):
    step = [(5, placed(QUARTER_Y, (40, 0, -20))[None]), (4, shifted(I34, (-30, 0, 10)))]
    m = api.MultiRenderer(cornell64, W, H, [0, 0], max_bounces=DEPTH, strip_rows=4)
    m.render(0, 2)
    move(m.rank0, step)
    m.reset_accumulation()
    got = m.render(0, 3)
    m.close()
    want = api.Renderer(apply(cornell64, step), W, H, max_bounces=DEPTH).render(0, 3)[0]
    assert_bit_equal(got, want, "pt_multi over a duplicated device after a move")
    assert not np.array_equal(want, api.Renderer(cornell64, W, H, max_bounces=DEPTH).render(0, 3)[0])


def test_headless_slide_writes_what_the_python_route_predicts(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    frames, dx, dz = 4, 7.5, -3.25
    exe = B.build_host_driver()
    out = tmp_path / "slide.png"
    run = subprocess.run([exe, "--width", str(W), "--height", str(H), "--frames", str(frames), "--bounces", str(DEPTH), "--slide", str(dx), str(dz),
                          "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(W / H))
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    last = r.inv_projection()
    for f in range(frames):
        if f >= 1:
            r.set_instances(5, placed(I34, (F(f) * F(dx), 0.0, F(f) * F(dz)))[None])
            r.rebuild()
        r.frame_moving(f, last, download=False)
        last = r.inv_projection()
    want = tmp_path / "python.png"
    r.write_image(want)
    assert out.read_bytes() == want.read_bytes()
    assert r.scene_info().uploads_patched == frames - 1
