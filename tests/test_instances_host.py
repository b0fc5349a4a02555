"""CPU: pt_set_instances and the incremental pt_build against builds from nothing (the oracle's and a fresh context's), the state and argument
errors of the new entry points, and pt_frame_moving's x_prev arithmetic restated in numpy (kept here: every product and sum one np.float32
operation).  No compute call needs a GPU here; the post_motion value tests that do are in tests/test_gpu_instances.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from instances_common import QUARTER_X, QUARTER_Y, apply, chain, move, placed, shifted

NEW_SYMBOLS = ["pt_set_instances", "pt_get_scene_info", "pt_read_guide_instances", "pt_frame_moving", "pt_post_motion"]


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def test_new_symbols_exported_and_bound(api):
    L = C.CDLL(api._build.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(L, name), name
        assert getattr(api.lib(), name).argtypes is not None, name
    for meth in ("set_instances", "scene_info", "read_guide_instances", "frame_moving", "post_motion", "rebuild"):
        assert callable(getattr(api.Renderer, meth)), meth
    assert C.sizeof(api.SceneInfo) == 64


def _cmp(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert_bit_equal(np.asarray(a[k]), np.asarray(b[k]), f"{what}.{k}")


def _tables(x, materials=True):
    out = {}
    for which in (0, 1):
        for k, v in x.tlas_dump(which).items():
            out[f"tlas{which}.{k}"] = v
        for k, v in x.tlas_instances(which).items():
            out[f"inst{which}.{k}"] = v
        if materials:
            for k, v in x.instance_materials(which).items():
                out[f"mat{which}.{k}"] = v
    for k, v in x.light_cdf().items():
        out[f"lights.{k}"] = v
    return out


def _scene(name):
    from path_tracer_amd import scenes
    if name == "cornell_instanced":
        return scenes.cornell_instanced(32, 32), None
    if name.startswith("random"):
        sc = scenes.random_scene(int(name[6:]))
        return sc, None
    sc = scenes.atrium(64, 36, statue_level=0)
    return sc, [7, 8, 9, 10]       # the four column models (72 + 3 instances)


@pytest.mark.parametrize("name", ["cornell_instanced", "random3", "random11", "random29", "atrium"])
def test_moved_scene_builds_what_a_fresh_scene_builds(api, oracle_mod, name):
    """after every step of a chain of moves the two TLASes, their leaves' matrices and materials and the light sampler are, bit for bit, the
    oracle's and a fresh context's for a scene built from nothing with those matrices; no BLAS is ever built twice"""
    desc, movable = _scene(name)
    r = api.Renderer(desc, 32, 32)
    n_models = len(desc.models)
    dumped = [b for b in range(n_models)] if n_models < 32 else [0, 4, 7, 10, n_models - 1]
    blas0 = {b: r.blas_dump(b) for b in dumped}
    assert r.scene_info().blas_builds == n_models and r.scene_info().tlas_builds == 1
    steps = chain(desc, 5, movable)
    for k, step in enumerate(steps):
        desc = apply(desc, step)
        move(r, step)
        info = r.scene_info()
        assert info.blas_builds == n_models, (k, info.as_dict())
        assert info.tlas_builds == k + 2
        got = _tables(r)
        fresh = api.Renderer(desc, 32, 32)
        _cmp(got, _tables(fresh), f"{name} step {k} vs a fresh context")
        o = oracle_mod.Oracle(desc)
        _cmp(_tables(r, materials=False), _tables_oracle(o), f"{name} step {k} vs the oracle")
        fresh.close()
    for b in dumped:
        _cmp(r.blas_dump(b), blas0[b], f"{name} blas {b} after the chain")


def _tables_oracle(o):
    out = {}
    for which in (0, 1):
        for k, v in o.tlas_dump(which).items():
            out[f"tlas{which}.{k}"] = v
        for k, v in o.tlas_instances(which).items():
            out[f"inst{which}.{k}"] = v
    for k, v in o.light_cdf().items():
        out[f"lights.{k}"] = v
    return out


def test_refused_moves_change_nothing(api, cornell64):
    r = api.Renderer(cornell64, 16, 16)
    before = _tables(r)
    good = np.eye(3, 4, dtype=np.float32)[None]
    scaled = good.copy(); scaled[0, 0, 0] = 2.0
    for model, mats, code in ((-1, good, -1), (len(cornell64.models), good, -1), (5, scaled, -4), (5, np.stack([good[0], scaled[0]]), -4)):
        with pytest.raises(api.PtError) as e:
            r.set_instances(model, mats)
        assert e.value.code == code, (model, e.value)
    assert api.lib().pt_set_instances(r.ctx, 5, None, 1) == -1                      # NULL matrices with n_instances > 0
    # r saw only refused calls: it is still built (the builder dumps answer) and unchanged
    assert r.blas_count() == len(cornell64.models)
    _cmp(_tables(r), before, "after refused moves")
    assert r.scene_info().tlas_builds == 1


def test_accepted_move_needs_a_build_before_a_render(api, cornell64):
    r = api.Renderer(cornell64, 16, 16)
    r.set_instances(5, shifted(np.eye(3, 4, dtype=np.float32), (10, 0, 0)))
    for call in (lambda: r.render(0, 1), lambda: r.frame(0), lambda: r.frame_moving(0), lambda: r.render_guides(0),
                 lambda: r.trace_closest(np.zeros((1, 3), np.float32), np.array([[0, 0, -1]], np.float32))):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == -3, e.value                                          # PT_ERR_STATE, decided before any device call
    assert api.lib().pt_blas_count(r.ctx) == -3                                     # un-built, like after pt_add_model
    r.rebuild()
    assert r.blas_count() == len(cornell64.models) and r.scene_info().blas_builds == len(cornell64.models)


def test_frame_moving_and_guide_instances_state_errors(api, cornell64):
    from path_tracer_amd.scene_desc import SceneDesc
    r = api.Renderer(SceneDesc.new(cornell64.models, None), 16, 16)
    with pytest.raises(api.PtError) as e:
        r.frame_moving(0)
    assert e.value.code == -3 and "pt_set_camera" in str(e.value)                   # as pt_frame
    with pytest.raises(api.PtError) as e:
        r.read_guide_instances()
    assert e.value.code == -3 and "pt_render_guides" in str(e.value)                # as pt_read_guides
    r2 = api.Renderer(cornell64, 16, 16, rank=1, world_size=2)
    with pytest.raises(api.PtError) as e:
        r2.frame_moving(0)
    assert e.value.code == -3 and "one rank" in str(e.value)
    assert api.lib().pt_frame_moving(None, 0, None, None, None, None) == -1
    assert api.lib().pt_read_guide_instances(None, None) == -1
    assert api.lib().pt_get_scene_info(r.ctx, None) == -1


def test_post_motion_argument_checks(api, cornell64):
    r = api.Renderer(cornell64, 16, 16)
    L = api.lib()
    pos = np.zeros((2, 2, 4), np.float32); inst = np.zeros((2, 2), np.uint32); out = np.zeros((2, 2, 4), np.float32)
    tab = np.eye(3, 4, dtype=np.float32).reshape(1, 12).copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pt_post_motion(None, 2, 2, p(pos), p(inst), 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    assert L.pt_post_motion(r.ctx, 2, 2, None, p(inst), 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    assert L.pt_post_motion(r.ctx, 2, 2, p(pos), None, 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    assert L.pt_post_motion(r.ctx, 2, 2, p(pos), p(inst), 1, p(tab), p(tab), p(tab), None, None) == -1
    assert L.pt_post_motion(r.ctx, 0, 2, p(pos), p(inst), 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    assert L.pt_post_motion(r.ctx, 2, 0, p(pos), p(inst), 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    for k in range(3):
        tabs = [p(tab)] * 3
        tabs[k] = None
        assert L.pt_post_motion(r.ctx, 2, 2, p(pos), p(inst), 1, *tabs, None, p(out)) == -1
    inst[1, 1] = 1                                                                  # neither a miss nor below n_instances
    assert L.pt_post_motion(r.ctx, 2, 2, p(pos), p(inst), 1, p(tab), p(tab), p(tab), None, p(out)) == -1
    assert "instance" in L.pt_last_error(r.ctx).decode()


def test_incremental_flatten_is_the_flatten_from_nothing_under_sanitizers():
    """the host side of a chain of random moves in the ASan + UBSan build of the host code: after every incremental build (BLAS part of the
    flattened scene kept, or laid out again after a count change) every table of the flattened scene equals, byte for byte, the one a scene
    built from nothing with those matrices flattens to; three BLASes are built once"""
    import json
    import os
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "path_tracer_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    for seed in (1, 2):
        run = subprocess.run([os.path.join(ROOT, "path_tracer_amd", "host_sanitize"), "moves", "60", str(seed)], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stdout, run.stderr[-3000:])
        res = json.loads(run.stdout.strip().split("\n")[-1])
        assert res["blas_builds"] == 3 and 15 < res["kept_blas_part"] < 60, res


# ---- x_prev restated: binary32, every product and sum a separate np.float32 operation, in the order include/pt_api.h writes
def x_prev_numpy(position, instance, matrix12, inv_matrix12, prev12, has_prev=None):
    f = np.float32
    pos = np.ascontiguousarray(position, np.float32)
    out = pos.copy()
    flat_in = pos.reshape(-1, 4); flat_out = out.reshape(-1, 4)
    inst = np.ascontiguousarray(instance, np.uint32).reshape(-1)
    M = np.asarray(matrix12, np.float32).reshape(-1, 3, 4); I = np.asarray(inv_matrix12, np.float32).reshape(-1, 3, 4)
    P = np.asarray(prev12, np.float32).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        for p in range(flat_in.shape[0]):
            i = int(inst[p])
            if i == 0xFFFFFFFF or (has_prev is not None and not has_prev[i]) or M[i].tobytes() == P[i].tobytes():
                continue                                                            # x_prev = x, no arithmetic
            x = [f(v) for v in flat_in[p, :3]]
            o = [f(f(f(I[i, k, 0] * x[0]) + f(I[i, k, 1] * x[1])) + f(I[i, k, 2] * x[2])) + I[i, k, 3] for k in range(3)]
            for k in range(3):
                flat_out[p, k] = f(f(f(P[i, k, 0] * o[0]) + f(P[i, k, 1] * o[1])) + f(P[i, k, 2] * o[2])) + P[i, k, 3]
    return out


def _inverse_exact(m):
    """inverse of a quarter turn + integer translation, exact in binary32"""
    r = m[:, :3].T.copy()
    out = np.zeros((3, 4), np.float32)
    out[:, :3] = r
    out[:, 3] = -(r.astype(np.float64) @ m[:, 3].astype(np.float64))
    return out


def case_exact():
    """small-integer points under quarter turns and integer translations: the composition is exact in binary32"""
    rng = np.random.default_rng(3)
    cur = np.stack([placed(QUARTER_Y, (3, -2, 7)), placed(QUARTER_X, (0, 5, -4)), placed(np.eye(3, 4, dtype=np.float32), (1, 1, 1))])
    prv = np.stack([placed(QUARTER_X, (-6, 0, 2)), placed(QUARTER_X, (0, 5, -4)), placed(QUARTER_Y, (9, -9, 0))])
    inv = np.stack([_inverse_exact(m) for m in cur])
    pos = rng.integers(-50, 51, (5, 7, 4)).astype(np.float32)
    inst = rng.integers(0, 3, (5, 7)).astype(np.uint32)
    inst[0, 0] = 0xFFFFFFFF
    want = pos.copy()
    for y in range(5):
        for x in range(7):
            i = int(inst[y, x])
            if i != 0xFFFFFFFF:
                obj = inv[i, :, :3].astype(np.float64) @ pos[y, x, :3].astype(np.float64) + inv[i, :, 3]
                want[y, x, :3] = prv[i, :, :3].astype(np.float64) @ obj + prv[i, :, 3]          # integers below 2^24: exact
    return (pos, inst, cur, inv, prv, None), want


def case_hand_worked():
    """a vector where every other association of the sums gives another float: ((a + b) + c) + d with a = 2^24, b = 1, c = 1, d = -2^24.
    inv row 0 = (1, 1, 1 | -2^24) on x = (2^24, 1, 1): (2^24 + 1) rounds to 2^24, + 1 again 2^24, - 2^24 = 0; any other order gives 1 or 2.
    Then o = (0, 1, 1); x_prev.y = ((2^24 * 0 + 1 * 1) + 1 * 1) + -2^24 = 2 - 2^24 (exact); x_prev.z = 1 + 0.5"""
    big = np.float32(2.0 ** 24)
    inv = np.zeros((1, 3, 4), np.float32); inv[0, 0] = [1, 1, 1, -big]; inv[0, 1] = [0, 1, 0, 0]; inv[0, 2] = [0, 0, 1, 0]
    prv = np.zeros((1, 3, 4), np.float32); prv[0, 0] = [1, 0, 0, 0]; prv[0, 1] = [big, 1, 1, -big]; prv[0, 2] = [0, 0, 1, 0.5]
    cur = np.eye(3, 4, dtype=np.float32)[None]
    pos = np.array([[[big, 1, 1, 42.0]]], np.float32)
    want = np.array([[[0.0, np.float32(2.0) - big, 1.5, 42.0]]], np.float32)
    return (pos, np.zeros((1, 1), np.uint32), cur, inv, prv, None), want


def case_untouched(second_has_prev):
    """an unmoved instance (previous matrix bit-equal), a miss and a moved instance, on points holding -0 and a NaN with a payload"""
    cur = np.stack([placed(QUARTER_Y, (3, -2, 7)), placed(QUARTER_X, (1, 2, 3))])
    inv = np.stack([_inverse_exact(m) for m in cur])
    prv = np.stack([cur[0], placed(QUARTER_X, (1, 2, 4))])
    nan = np.array([0x7FA00001], np.uint32).view(np.float32)[0]
    pos = np.array([[[-0.0, nan, 5.0, 1.0], [-0.0, 2.0, 3.0, 4.0], [-0.0, nan, 1.0, 2.0]]], np.float32)
    inst = np.array([[0, 0xFFFFFFFF, 1]], np.uint32)
    return pos, inst, cur, inv, prv, np.array([1, 1 if second_has_prev else 0], np.uint8)


def test_x_prev_restatement_is_exact_where_the_answer_is_representable():
    args, want = case_exact()
    got = x_prev_numpy(*args)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[..., :3], args[0][..., :3])


def test_x_prev_operation_order_hand_worked():
    args, want = case_hand_worked()
    assert x_prev_numpy(*args)[0, 0].tolist() == want[0, 0].tolist() == [0.0, 2.0 - 2.0 ** 24, 1.5, 42.0]


def test_x_prev_passes_unmoved_points_on_untouched():
    """bit-equal matrices (and misses, and instances without a previous matrix) return x itself, also a -0 and a NaN arithmetic would change"""
    args = case_untouched(True)
    pos = args[0]
    got = x_prev_numpy(*args)
    assert np.array_equal(got[0, :2].view(np.uint32), pos[0, :2].view(np.uint32))   # unmoved instance, miss: the very bits
    assert not np.array_equal(got[0, 2, :3].view(np.uint32), pos[0, 2, :3].view(np.uint32))   # the moved one went through the arithmetic
    got = x_prev_numpy(*case_untouched(False))
    assert np.array_equal(got.view(np.uint32), pos.view(np.uint32))                 # no previous matrix: x itself
