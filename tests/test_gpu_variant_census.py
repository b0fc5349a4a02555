"""GPU: the variant census (tests/variant_census_common.py).  One test per case of the table, three statements each:
 (a) what the case computes is the oracle's, bit for bit (textured rooms against the oracle's render of the untextured equivalent);
 (b) the launch log (pt_last_launches: the axis values the dispatchers computed) holds exactly the case's set of variants, so a case that
     silently moves to another kernel fails;
 (c) every logged surface pass had entries in its queue (pt_last_batch_counters), and every variant of the other launchers was launched on
     a non-empty queue at least once: a launch over an empty queue proves nothing and does not count.  (The one launch a scene cannot feed,
     Case.idle, is named in the table and held to be idle.)"""
import numpy as np
import pytest

from conftest import assert_bit_equal
from variant_census_common import CASES, DEPTH, H, M, SPILL_LEVELS, W, cameras_of, expect, room, textured

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _renderer(api, case):
    r = api.Renderer(textured(case.room, case.surface), W, H, max_bounces=DEPTH, flags=case.config_flags, stack_lds_levels=SPILL_LEVELS if case.spill else 0)
    lens, cams = cameras_of(case.room)
    if case.camera == "lens":
        r.set_lens(*lens)
    elif case.camera != "pinhole":
        r.set_projection(*cams[case.camera])
    return r


class Seen:
    """the variants a case's requests launched, and those launched with work"""

    def __init__(self, r, api):
        self.r, self.api = r, api
        self.all, self.worked, self.idle_surface, self.queues = set(), set(), [], {}

    def batch(self):
        """after a request that ran wavefront batches: the last batch's log against its counter rows"""
        rows = self.r.last_batch_counters().astype(np.int64)
        log = self.r.last_launches()
        assert log, "a batch logs its launches"
        for launcher, b, axes in log:
            v = (launcher, axes)
            self.all.add(v)
            if launcher == "shade":
                work = rows[b][8 + axes[0]] > 0
                if not work:
                    self.idle_surface.append((b, axes))
            elif launcher == "terminal":
                work = rows[b][8] > 0
            elif launcher == "closest":
                work = rows[b][4] > 0 if axes[0] == 1 else rows[b][0] > 0      # the NEE rays' queue / the closest-hit queue
            elif launcher == "any":
                work = rows[b][2] > 0
            elif launcher == "fused":
                work = rows[b][0] > 0 and rows[b - 1][4] > 0
            else:                                                              # generate, accumulate: one thread (or four) per path / pixel
                work = True
            self.queues.setdefault(v, []).append((b, [int(x) for x in rows[b][[0, 2, 4, 8]]]))
            if work:
                self.worked.add(v)

    def hook(self, n):
        """after a request through the hook queue with n rays"""
        log = self.r.last_launches(self.api.LAUNCHES_HOOK)
        assert log and n > 0
        for launcher, _, axes in log:
            self.all.add((launcher, axes))
            self.worked.add((launcher, axes))

    def check(self, case):
        want = case.variants()
        assert self.all == want, f"{case.id}: launched but not expected {sorted(self.all - want)}, expected but not launched {sorted(want - self.all)}"
        assert not self.idle_surface, f"{case.id}: surface passes over an empty queue (bounce, axes): {self.idle_surface}"
        missing = [(v, self.queues.get(v)) for v in sorted(want - case.idle() - self.worked)]
        assert not missing, f"{case.id}: never launched with work (variant, [(bounce, [closest, shadow, NEE, terminal slots])]): {missing}"
        assert not self.worked & case.idle(), f"{case.id}: the table calls these idle, yet they had work: {sorted(self.worked & case.idle())}"


def _render(api, O, case, r, seen):
    ex = expect(O, case.room, case.camera)
    got = r.render_samples(0, M)
    seen.batch()
    assert_bit_equal(got, np.stack([ex.sample(s)[0] for s in range(M)]), f"{case.id}: per-sample radiance")
    r.reset_accumulation()
    acc, pos, idb = r.render(0, M, ident=np.zeros((H, W), np.uint32))
    seen.batch()
    oacc, opos, oid = ex.frame(M)
    assert_bit_equal(acc, oacc, f"{case.id}: accumulation")
    assert_bit_equal(pos, opos, f"{case.id}: position")
    assert np.array_equal(idb, oid), f"{case.id}: id history"


def _adaptive(api, O, case, r, seen):
    """two rounds of pt_render_adaptive (the second over an adaptive list): every pixel ends with exactly pt_render(0, n_p)'s bits, n_p its
    own count (test_gpu_shade_variants.test_two_adaptive_rounds' statement)"""
    ex = expect(O, case.room, case.camera)
    first = np.stack([ex.sample(s)[0] for s in range(M)])
    lum = 0.2126 * first[..., 0] + 0.7152 * first[..., 1] + 0.0722 * first[..., 2]
    rel = np.sqrt(lum.var(0) / M) / np.maximum(lum.mean(0), 1e-3)
    threshold = float(np.quantile(rel[rel > 0], 0.5))     # the median relative error of the noisy pixels: the second round is a proper subset
    assert 0 < int((rel > threshold).sum()) < W * H, "the oracle's own error should split the frame"
    assert r.render_adaptive(M, threshold, 0.0, M, 0) == W * H
    seen.batch()
    second = r.render_adaptive(M, threshold, 0.0, M, 0)
    seen.batch()
    assert 0 < second < W * H, second
    acc, pos, idb = r.read_frame()
    counts = np.rint(acc[..., 3]).astype(np.int64)
    assert set(np.unique(counts)) == {M, 2 * M}, np.unique(counts)
    assert int((counts == 2 * M).sum()) == second
    for n in (M, 2 * M):
        sel = counts == n
        oacc, opos, oid = ex.frame(n)
        assert_bit_equal(acc[sel], oacc[sel], f"{case.id}: accumulation of the {int(sel.sum())} pixels with {n} samples")
        assert_bit_equal(pos[sel], opos[sel], f"{case.id}: position of the pixels with {n} samples")
        assert np.array_equal(idb[sel], oid[sel]), f"{case.id}: id history of the pixels with {n} samples"


def _rays(api, O, case, r, seen):
    """the lens camera's rays of samples 0 .. M - 1 of every pixel as one table, each under its pixel's key and its sample, two draws consumed:
    every ray comes back as the oracle's walk of it from the same key, sample and draws"""
    from test_lens_host import lens_rays
    ex = expect(O, case.room, "lens")
    pixels = np.arange(W * H, dtype=np.uint32)
    tables = [lens_rays(O, ex.orc, W, H, pixels, s, *cameras_of(case.room)[0]) for s in range(M)]
    assert all(t[2] == 2 for t in tables)
    o, d = np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])
    rad, pos, idb = r.integrate_rays(o, d, np.tile(pixels, M), np.repeat(np.arange(M, dtype=np.uint32), W * H), draws_consumed=2)
    seen.batch()
    for s in range(M):
        col, opos, oid = ex.sample(s)
        part = slice(s * W * H, (s + 1) * W * H)
        assert_bit_equal(rad[part].reshape(H, W, 4), col, f"{case.id}: radiance per ray, sample {s}")
        assert_bit_equal(pos[part].reshape(H, W, 4), opos, f"{case.id}: position per ray, sample {s}")
        assert np.array_equal(idb[part].reshape(H, W), oid & 0xFF), f"{case.id}: id byte per ray, sample {s}"


def _guides(api, O, case, r, seen):
    ex = expect(O, case.room, case.camera)
    r.render_guides(0)
    seen.hook(W * H)
    gpos, _, gmodel = r.read_guides()
    _, opos, oid = ex.sample(0)
    assert_bit_equal(gpos, opos, f"{case.id}: position guide")
    assert np.array_equal(gmodel & 0xFF, oid & 0xFF), f"{case.id}: model guide"


def _hooks(api, O, case, r, seen):
    """rays from about the room's middle in every direction (some reach the light), against both TLASes"""
    orc = expect(O, case.room, "lens").orc
    rng = np.random.default_rng(17)
    n = W * H
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.sqrt((d * d).sum(1))[:, None]).astype(F)
    for which in (0, 1):
        g = r.trace_closest(o, d, which=which)
        seen.hook(len(o))
        c = orc.trace_closest(o, d, which=which)
        for k in ("inst", "prim", "t", "u", "v"):
            assert_bit_equal(g[k], c[k], f"{case.id}: tlas {which} closest.{k}")
        assert (c["inst"] != 0xFFFFFFFF).any()
    tm = np.random.default_rng(3).uniform(0.0, 25.0, len(o)).astype(F)
    got = r.trace_any(o, d, tm)
    seen.hook(len(o))
    want = orc.trace_any(o, d, tm)
    assert np.array_equal(got, want), f"{case.id}: any hit"
    assert want.any() and not want.all()


ROUTE = {"render": _render, "adaptive": _adaptive, "rays": _rays, "guides": _guides, "hooks": _hooks}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case(api, oracle_mod, case):
    r = _renderer(api, case)
    seen = Seen(r, api)
    ROUTE[case.route](api, oracle_mod, case, r, seen)
    st = r.stats()
    assert st.lds_scene == (0 if case.flags & 2 else 1), "every room of the census fits LDS"
    assert not case.spill or st.stack_entries > SPILL_LEVELS, f"stack_entries {st.stack_entries}: nothing spills"
    seen.check(case)
