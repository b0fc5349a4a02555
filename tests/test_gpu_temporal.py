"""GPU (-m gpu): the temporal stage of the denoiser.  The kernels (pt_post_temporal(on_device = 1)) against the host path and the numpy
restatement of tests/temporal_common.py on the cases of tests/test_temporal_host.py; pt_frame_temporal over a sequence with the camera and an
instance moving, every frame's state and result against the restatement fed the frame's own sample, guides and velocity; what the new calls
must leave alone; and the quality the stage exists for.  Everything but the quality case is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from instances_common import move, shifted
from temporal_common import MISS, F, carried_normal, empty_state, frame_temporal, post_temporal, random_case
from test_temporal_host import SIZES

pytestmark = pytest.mark.gpu

W, H, DEPTH = 48, 32, 4


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


# ---------------------------------------------------------------- the kernels on caller images
@pytest.mark.parametrize("wh", SIZES)
def test_device_path_equals_the_host_path_and_the_restatement(api, oracle_mod, cornell64, wh):
    w, h = wh
    r = api.Renderer(cornell64, 16, 16)
    for seed in range(3):
        prev, cur, xprev, nprev, vel = random_case(np.random.default_rng(100 * w + seed), w, h)
        for mode, kw in (("velocity", dict(xprev=xprev, nprev=nprev, velocity=vel)), ("rest", dict(xprev=xprev, nprev=nprev)), ("plain", dict(velocity=vel))):
            if seed == 0:
                kw = dict(kw, alpha=0.5, alpha_moments=0.05, normal_min=-1.0, plane_max=0.5, sigma_normal=8, sigma_plane=0.25)
            want = post_temporal(prev, cur, **kw)
            host = r.post_temporal(prev, cur, on_device=False, **kw)
            dev = r.post_temporal(prev, cur, on_device=True, **kw)
            for d, hs, wt, name in zip(dev, host, want, ("history", "moments", "variance")):
                assert_bit_equal(d, hs, f"{w}x{h} {mode} seed {seed}: {name}, device against host")
                assert_bit_equal(d, wt, f"{w}x{h} {mode} seed {seed}: {name}, device against the restatement")
    r.close()


# ---------------------------------------------------------------- pt_frame_temporal over a sequence
def _events(api):
    """eight frames: two at rest, three after camera events, two after the third instance of the four-instance box model moved, one at rest"""
    from path_tracer_amd import scenes
    base = scenes.cornell_instanced(W, H).models[4].matrices
    a = base.copy(); a[2] = shifted(base[2], (-6, 4, 3))[0]
    b = a.copy(); b[2] = scenes.rigid_from_quat(1, -7, -3, 2.2, (14.0, -136.0, 146.0))
    cam = [(api.EV_KEY_W, 0.0, 0.0, 2.0e-6), (api.EV_MOUSE_MOTION, 1.0, 0.25, 1.0e-6)]
    return [None, None, ("camera", cam), ("camera", cam[1:]), ("camera", cam[:1]), ("world", a), ("world", b), None]


def _table_moved(cur, prv):
    return np.array([c.tobytes() != p.tobytes() for c, p in zip(cur, prv)], bool)


@pytest.mark.parametrize("flags", ["lds", "global"])
@pytest.mark.parametrize("feedback", [0, 1])
def test_sequence_equals_the_restatement(api, oracle_mod, feedback, flags):
    from path_tracer_amd import scenes
    desc = scenes.cornell_instanced(W, H)
    r = api.Renderer(desc, W, H, max_bounces=DEPTH, flags=api.FLAG_NO_LDS_SCENE if flags == "global" else 0)
    ident = np.zeros((H, W), np.uint32)
    last = r.inv_projection()
    state = empty_state(W, H)
    prev_tab = None
    seen = {"disoccluded": 0, "four_taps": 0}
    branches = []
    kw = dict(iterations=3)
    for k, ev in enumerate(_events(api)):
        if ev and ev[0] == "camera":
            for e in ev[1]:
                assert r.camera_input(*e)
        if ev and ev[0] == "world":
            move(r, [(4, ev[1])])
        data, pos, ident, out = r.frame_temporal(k, last, ident, feedback=feedback, **kw)
        gpos, gnrm, gmodel = r.read_guides()
        inst = r.read_guide_instances()
        hit = gmodel != MISS
        assert_bit_equal(gpos[hit], pos[hit], f"frame {k}: the guides are this sample's")
        assert np.array_equal(gmodel[hit] & 0xFF, ident[hit] & 0xFF)
        tabs = r.tlas_instances(0)
        cur_inv = r.inv_projection()
        cam_moved = not np.array_equal(cur_inv, last)
        rows = _table_moved(tabs["matrix"], prev_tab) if prev_tab is not None else np.zeros(len(tabs["matrix"]), bool)
        world_moved = bool(rows.any())
        xprev, nprev, vel = None, None, None
        if world_moved:
            xprev = r.post_motion(pos, inst, tabs["matrix"], tabs["inv_matrix"], prev_tab)
            nprev = carried_normal(gnrm, inst, tabs["inv_matrix"], prev_tab, rows)
            assert not np.array_equal(nprev, gnrm)
        if cam_moved or world_moved:
            vel = r.post_velocity(pos if xprev is None else xprev, last)
        branches.append("rest" if vel is None else ("world" if world_moved else "camera"))
        st = {}
        state, var, want = frame_temporal(state, (data, gpos, gnrm, gmodel), xprev, nprev, vel, feedback=feedback, stats=st, **kw)
        if k > 0:
            seen = {n: seen[n] + st[n] for n in seen}
        cn, mom, v = r.read_temporal()
        assert_bit_equal(cn, state[0], f"frame {k} ({branches[-1]}): history")
        assert_bit_equal(mom, state[1], f"frame {k}: moments")
        assert_bit_equal(v, var, f"frame {k}: variance")
        assert_bit_equal(out, want, f"frame {k}: result")
        prev_tab = tabs["matrix"].copy()
        last = cur_inv
    assert branches == ["rest", "rest", "camera", "camera", "camera", "world", "world", "rest"]
    assert seen["disoccluded"] > 0 and seen["four_taps"] > 0, seen     # the sequence cannot pass on rest frames alone
    assert state[0][..., 3].max() >= 5 and state[0][..., 3].min() >= 1
    r.close()


# ---------------------------------------------------------------- what the new calls leave alone
def test_the_accumulation_and_the_moments_are_untouched(api, cornell64):
    r = api.Renderer(cornell64, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    r.render(0, 3)
    acc, q = r.read_accumulation(), r.read_moments()
    r.render_guides(2)
    before = r.denoise()                                       # with the moments: they are valid
    last = r.inv_projection()
    I34 = np.eye(3, 4, dtype=F)
    r.frame_temporal(3, last)
    move(r, [(5, shifted(I34, (20, 0, -10)))])
    r.frame_temporal(4, last)                                  # a moved frame: every kernel of the stage has run
    assert (r.read_temporal()[0][..., 3] == 1).any() and (r.read_temporal()[0][..., 3] == 2).any()
    r.post_temporal(empty_state(4, 4), (np.ones((4, 4, 4), F), np.zeros((4, 4, 4), F), np.zeros((4, 4, 3), F), np.zeros((4, 4), np.uint32)), on_device=True)
    assert_bit_equal(r.read_accumulation(), acc, "accumulation")
    assert_bit_equal(r.read_moments(), q, "Q")
    move(r, [(5, I34[None])])                                  # the scene of the accumulation again, to the bit
    r.render_guides(2)
    assert_bit_equal(r.denoise(), before, "pt_denoise still has its moments")   # moments_valid was not cleared
    assert_bit_equal(r.read_accumulation(), acc, "accumulation")
    r.close()


def test_frame_moving_and_denoise_are_what_they_were(api, cornell64):
    """a pt_frame_moving + pt_denoise sequence on a context that also runs the temporal stage between the frames gives the bits of a context that
    never heard of it (whose own bits tests/test_gpu_instances.py and tests/test_gpu_denoise.py hold to the oracle)"""
    a = api.Renderer(cornell64, W, H, max_bounces=DEPTH); b = api.Renderer(cornell64, W, H, max_bounces=DEPTH)
    I34 = np.eye(3, 4, dtype=F)
    id_a = np.zeros((H, W), np.uint32); id_b = np.zeros((H, W), np.uint32)
    last = a.inv_projection()
    b.frame_temporal(7, last); b.frame_temporal(8, last)       # (they advance the id history, which the frames below are handed anew)
    for k in range(5):
        if k == 2:
            for r in (a, b):
                r.camera_input(api.EV_MOUSE_MOTION, 1.0, 0.25, 1.0e-6)
        if k == 3:
            for r in (a, b):
                move(r, [(5, shifted(I34, (20, 0, -10)))])
        da, pa, id_a = a.frame_moving(k, last, id_a)
        db, pb, id_b = b.frame_moving(k, last, id_b)
        assert_bit_equal(db, da, f"frame {k}: data"); assert np.array_equal(id_a, id_b)
        assert_bit_equal(b.read_accumulation(), a.read_accumulation(), f"frame {k}: accumulation")
        assert_bit_equal(b.denoise(), a.denoise(), f"frame {k}: denoise")
        b.post_temporal(empty_state(3, 3), (np.ones((3, 3, 4), F), np.zeros((3, 3, 4), F), np.zeros((3, 3, 3), F), np.zeros((3, 3), np.uint32)), on_device=True)
        last = a.inv_projection()
    a.close(); b.close()


def test_the_history_drops_on_the_listed_events_only(api, cornell64):
    r = api.Renderer(cornell64, W, H, max_bounces=DEPTH)
    I34 = np.eye(3, 4, dtype=F)

    def alive():
        try:
            return r.read_temporal()[0][..., 3].max()
        except api.PtError as e:
            assert e.code == -3
            return 0

    k = 0

    def step():
        nonlocal k
        r.frame_temporal(k, r.inv_projection()); k += 1

    assert alive() == 0
    step(); step()
    assert alive() == 2
    # events that keep it
    r.camera_input(api.EV_KEY_W, 0.0, 0.0, 2.0e-6); assert alive() == 2
    move(r, [(5, shifted(I34, (5, 0, 0)))]); assert alive() == 2
    r.set_camera(cornell64.camera); assert alive() == 2       # (sets the lens in force again)
    r.set_config(max_bounces=3); assert alive() == 2
    r.render_guides(0); r.reset_accumulation(); r.frame_moving(k, None); r.denoise(); assert alive() == 2
    step()
    assert alive() == 3
    # events that drop it
    r.reset_temporal(); assert alive() == 0
    step(); assert alive() == 1
    r.set_lens(2.0, 900.0); assert alive() == 0
    step(); step(); assert alive() == 2
    r.set_lens(0.0, 0.0); assert alive() == 0
    step(); assert alive() == 1
    r.set_projection(api.PROJ_PANORAMA); assert alive() == 0
    r.set_projection(api.PROJ_PERSPECTIVE)
    step(); step(); assert alive() == 2
    r.set_config(width=W // 2); assert alive() == 0
    r.close()


def test_the_refusals_under_a_projected_camera_are_frame_movings(api, cornell64):
    r = api.Renderer(cornell64, W, H, max_bounces=DEPTH)
    r.set_projection(api.PROJ_ORTHOGRAPHIC, ortho_height=500.0)
    last = r.inv_projection()
    r.frame_temporal(0, last); r.frame_temporal(1, last)       # at rest it works
    assert r.read_temporal()[0][..., 3].max() == 2
    r.camera_input(api.EV_KEY_W, 0.0, 0.0, 2.0e-6)
    with pytest.raises(api.PtError) as e:
        r.frame_temporal(2, last)
    assert e.value.code == -3
    r.close()


# ---------------------------------------------------------------- examples/headless --temporal
def test_headless_temporal_writes_what_the_python_route_gives(api, tmp_path):
    from path_tracer_amd import build as B, scenes
    from path_tracer_amd.scene_desc import Model, SceneDesc
    from instances_common import placed
    frames, dx, dz = 4, 7.5, -3.25
    exe = B.build_host_driver()
    out = tmp_path / "temporal.png"
    run = subprocess.run([exe, "--width", str(W), "--height", str(H), "--frames", str(frames), "--bounces", str(DEPTH), "--slide", str(dx), str(dz),
                          "--temporal", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr
    src = scenes.cornell_models()
    sc = SceneDesc.new([Model.from_obj(os.path.join(ROOT, "models", "cornell", m.name + ".obj"), m.material) for m in src], scenes.reference_camera(W / H))
    r = api.Renderer(sc, W, H, max_bounces=DEPTH)
    I34 = np.eye(3, 4, dtype=F)
    last = r.inv_projection()
    for f in range(frames):
        if f >= 1:
            r.set_instances(5, placed(I34, (F(f) * F(dx), 0.0, F(f) * F(dz)))[None])
            r.rebuild()
        r.frame_temporal(f, last, download=False)
        last = r.inv_projection()
    want = tmp_path / "python.png"
    r.write_denoised_image(want)
    assert out.read_bytes() == want.read_bytes()
    r.close()


# ---------------------------------------------------------------- quality: what profiles/r20_temporal.md records
def _rmse(a, ref):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))


def test_quality_after_a_slow_pan(api):
    """128 x 128 Cornell box, 16 frames of 1 spp, the camera turning 0.004 rad (half a pixel) per frame; display-space RMSE (the library's GT
    tonemap) of the last frame against 1024 spp of the last pose.  Measured (profiles/r20_temporal.md): the raw frame 0.05453, pt_frame_moving +
    pt_denoise over the same sequence 0.02081, pt_frame_temporal 0.03584 (feedback 1: 0.03541).  The stage beats the raw frame, and the bound
    below is the raw frame's figure less half the measured gap.  It does NOT beat the existing recipe: the guides are one jittered sample's, so
    silhouette pixels fail the model test frame after frame, restart at N = 1, and drag their neighbours' N down through Nmin; the recipe's
    clamped blend knows no such restart.  That is a finding, stated in DESIGN.md section 20, and nothing here asserts it either way."""
    size, frames, depth = 128, 16, 3
    from path_tracer_amd import scenes
    sc = scenes.cornell_box(size, size)
    t = api.Renderer(sc, size, size, max_bounces=depth); m = api.Renderer(sc, size, size, max_bounces=depth); ref = api.Renderer(sc, size, size, max_bounces=depth)
    last_t, last_m = t.inv_projection(), m.inv_projection()
    for k in range(frames):
        if k:
            for r in (t, m, ref):
                r.camera_input(api.EV_MOUSE_MOTION, 1.0, 0.0, 4.0e-7)
        data, _, _, out = t.frame_temporal(k, last_t)
        m.frame_moving(k, last_m, download=False)
        last_t, last_m = t.inv_projection(), m.inv_projection()
    den = m.denoise()
    racc, _, _ = ref.render(1 << 20, 1024, want_position=False)
    want = ref.post_tonemap(racc)
    raw, recipe, new = _rmse(t.post_tonemap(data), want), _rmse(m.post_tonemap(den), want), _rmse(t.post_tonemap(out), want)
    print(f"display rmse after the pan: raw {raw:.5f} frame_moving + denoise {recipe:.5f} frame_temporal {new:.5f}")
    for r in (t, m, ref):
        r.close()
    assert new < raw - 0.5 * (0.05453 - 0.03584)
