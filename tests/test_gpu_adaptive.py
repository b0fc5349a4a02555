"""GPU (-m gpu): adaptive sampling (PT_FLAG_ADAPTIVE) against the CPU oracle, bit for bit.  A pixel that holds n samples after any
sequence of pt_render_adaptive calls holds exactly what the oracle's render of samples [0, n) gives it (accumulation, last-sample
first-hit position, id history); its moments are the f32 fold of L * L over the oracle's per-sample radiance; and each round's selection
is the numpy restatement of the criterion (test_adaptive_host.criterion) evaluated on that data."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_adaptive_host import criterion, fold_moments, luminance

pytestmark = pytest.mark.gpu
W, H = 48, 32
DEPTH = 5
F = np.float32


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


class Expect:
    """the oracle's per-sample radiance of a scene, folded per pixel to any count"""

    def __init__(self, oracle_mod, sc, n_max, rows=None, **okw):
        self.o = oracle_mod.Oracle(sc)
        self.okw = okw
        self.rows = rows
        s = self.o.render_samples(W, H, n_max, max_bounces=DEPTH, **okw)
        if rows is not None:
            s = s[:, rows]
        self.samples = s
        # prefix folds: cum_acc[k] / cum_q[k] = accumulation / moments after k samples, each an f32 add per sample in order
        cum_acc = [np.zeros(s.shape[1:], np.float32)]
        cum_q = [np.zeros(s.shape[1:3], np.float32)]
        for k in range(n_max):
            cum_acc.append(cum_acc[-1] + s[k])
            lum = luminance(s[k])
            cum_q.append(cum_q[-1] + lum * lum)
        self.cum_acc = np.stack(cum_acc)
        self.cum_q = np.stack(cum_q)

    def at(self, counts):
        c = counts.astype(np.int64)
        acc = np.take_along_axis(self.cum_acc, c[None, ..., None].repeat(4, axis=-1), axis=0)[0]
        q = np.take_along_axis(self.cum_q, c[None], axis=0)[0]
        return acc, q

    def frame(self, n):
        acc, pos, idb, _ = self.o.render(W, H, n, max_bounces=DEPTH, **self.okw)
        if self.rows is not None:
            acc, pos, idb = acc[self.rows], pos[self.rows], idb[self.rows]
        return acc, pos, idb


def _scene(name):
    from path_tracer_amd import scenes
    return {"cornell_box": lambda: scenes.cornell_box(W, H), "cornell_mixed": lambda: scenes.cornell_mixed(W, H),
            "random_media": lambda: scenes.random_scene(2, W, H)}[name]()


M = 4          # samples per round
ROUNDS = 5
MIN = 4
CAP = 20       # max_samples: a multiple of M, so that no pixel goes past it


def _rel_error(ex):
    """a threshold that the active set crosses gradually: the median relative error of the noisy pixels after MIN samples"""
    acc, q = ex.at(np.full(ex.samples.shape[1:3], MIN))
    n = F(MIN)
    m = luminance(acc) / n
    v = np.maximum(q / n - m * m, 0)
    rel = np.sqrt(v / n) / np.maximum(m, F(1e-3))
    return float(np.quantile(rel[rel > 0], 0.5))


def _rounds(api, ex, r, crit, what):
    """ROUNDS adaptive rounds of M samples, each checked; returns the final per-pixel counts"""
    shape = ex.samples.shape[1:3]
    counts = np.zeros(shape, np.int64)
    history = []
    for rnd in range(ROUNDS):
        acc, q = ex.at(counts)
        want = criterion(acc, q, **crit)
        got = r.adaptive_mask(**crit)
        assert np.array_equal(got, want), f"{what} round {rnd}: {int((got != want).sum())} pixels selected differently"
        n_active = r.render_adaptive(M, **crit)
        assert n_active == int(want.sum()), (what, rnd)
        history.append(n_active)
        counts[want] += M
        acc, q = ex.at(counts)
        gacc = r.read_frame()[0]
        assert_bit_equal(gacc, acc, f"{what} round {rnd} accumulation")
        assert_bit_equal(r.read_moments(), q, f"{what} round {rnd} moments")
    assert history[0] == counts.size, (what, history)
    assert all(b <= a for a, b in zip(history, history[1:])), (what, history)
    assert 0 < history[2] and history[-1] < history[1] < history[0], (what, "the active set does not shrink gradually", history)
    assert counts.max() <= CAP
    return counts


def _final_vs_oracle(ex, r, counts, what):
    acc, pos, idb = r.read_frame()
    for n in np.unique(counts):
        sel = counts == n
        oacc, opos, oid = ex.frame(int(n))
        assert_bit_equal(acc[sel], oacc[sel], f"{what}: accumulation of the {int(sel.sum())} pixels with {n} samples")
        assert_bit_equal(pos[sel], opos[sel], f"{what}: position of the pixels with {n} samples")
        assert np.array_equal(idb[sel], oid[sel]), f"{what}: id history of the pixels with {n} samples"


_EXPECT = {}


def _expect(oracle_mod, name, rows=None, key=None):
    k = (name, key)
    if k not in _EXPECT:
        _EXPECT[k] = Expect(oracle_mod, _scene(name), CAP, rows=rows)
    return _EXPECT[k]


@pytest.mark.parametrize("name", ["cornell_box", "cornell_mixed", "random_media"])
def test_moments_follow_every_render_path(api, oracle_mod, name):
    """pt_render and pt_render_device with the flag: moments = f32 fold of L * L over the oracle's samples; accumulation, position and id
    history identical to a context without the flag"""
    ex = _expect(oracle_mod, name)
    sc = _scene(name)
    plain = api.Renderer(sc, W, H, max_bounces=DEPTH)
    r = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    a0 = plain.render(0, 6)
    a1 = r.render(0, 6)
    for x, y, w in zip(a0, a1, ("accumulation", "position", "id")):
        assert_bit_equal(y, x, f"{name} {w} with the flag")
    assert_bit_equal(r.read_moments(), fold_moments(ex.samples[:6]), f"{name} moments after pt_render")
    d = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE, batch_spp=2)
    d.render_device(0, 3)
    d.render_device(3, 3)
    assert_bit_equal(d.read_frame()[0], a0[0], f"{name} pt_render_device accumulation")
    assert_bit_equal(d.read_moments(), fold_moments(ex.samples[:6]), f"{name} moments after pt_render_device")
    d.reset_accumulation()
    assert not d.read_moments().any()


@pytest.mark.parametrize("name", ["cornell_box", "cornell_mixed", "random_media"])
def test_rounds_against_the_oracle(api, oracle_mod, name):
    ex = _expect(oracle_mod, name)
    crit = dict(rel_error=_rel_error(ex), abs_floor=0.01, min_samples=MIN, max_samples=CAP)
    r = api.Renderer(_scene(name), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    counts = _rounds(api, ex, r, crit, name)
    _final_vs_oracle(ex, r, counts, name)


@pytest.mark.parametrize("variant", ["batches", "no_lds_scene", "general_walk"])
def test_rounds_variants(api, oracle_mod, variant):
    name = "cornell_mixed" if variant != "general_walk" else "cornell_box"
    ex = _expect(oracle_mod, name)
    crit = dict(rel_error=_rel_error(ex), abs_floor=0.01, min_samples=MIN, max_samples=CAP)
    kw = {"batches": dict(batch_spp=1, pipelines=2), "no_lds_scene": dict(flags=api.FLAG_NO_LDS_SCENE),
          "general_walk": dict(flags=api.FLAG_GENERAL_WALK)}[variant]
    flags = api.FLAG_ADAPTIVE | kw.pop("flags", 0)
    r = api.Renderer(_scene(name), W, H, max_bounces=DEPTH, flags=flags, **kw)
    counts = _rounds(api, ex, r, crit, f"{name} {variant}")
    _final_vs_oracle(ex, r, counts, f"{name} {variant}")
    if variant == "general_walk":
        assert r.stats().ident_tlas == 0


def test_rounds_on_a_rank_context(api, oracle_mod):
    from path_tracer_amd.dist import rows_of_rank
    name = "cornell_mixed"
    crit = dict(rel_error=_rel_error(_expect(oracle_mod, name)), abs_floor=0.01, min_samples=MIN, max_samples=CAP)
    for rank in range(2):
        rows = rows_of_rank(H, rank, 2, 4)
        ex = _expect(oracle_mod, name, rows=rows, key=("rank", rank))
        r = api.Renderer(_scene(name), W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE, rank=rank, world_size=2, strip_rows=4)
        assert np.array_equal(r.local_rows(), rows)
        counts = _rounds(api, ex, r, crit, f"rank {rank}")
        _final_vs_oracle(ex, r, counts, f"rank {rank}")


def test_zero_rel_error_is_uniform_rendering(api, oracle_mod):
    """rel_error = 0 and min_samples above the total: every pixel is active in every round, and k rounds of m samples are one
    render(0, k * m)"""
    sc = _scene("cornell_mixed")
    k, m = 3, 3
    r = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE, batch_spp=2)
    for _ in range(k):
        assert r.adaptive_mask(0.0, 0.0, k * m + 1, 0).all()
        assert r.render_adaptive(m, 0.0, 0.0, k * m + 1, 0) == W * H
    want = api.Renderer(sc, W, H, max_bounces=DEPTH).render(0, k * m)
    for x, y, w in zip(r.read_frame(), want, ("accumulation", "position", "id")):
        assert_bit_equal(x, y, f"rel_error 0 {w}")
    # with min_samples = 2 the same data selects exactly the pixels whose variance is not zero
    acc, _, _ = r.read_frame()
    q = r.read_moments()
    assert np.array_equal(r.adaptive_mask(0.0, 0.0, 2, 0), criterion(acc, q, 0.0, 0.0, 2, 0))


def test_checkpoint_resume_and_errors(api, oracle_mod):
    name = "cornell_box"
    ex = _expect(oracle_mod, name)
    sc = _scene(name)
    crit = dict(rel_error=_rel_error(ex), abs_floor=0.01, min_samples=MIN, max_samples=12)
    whole = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    for _ in range(5):
        whole.render_adaptive(M, **crit)
    a = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    for _ in range(2):
        a.render_adaptive(M, **crit)
    frame, q = a.read_frame(), a.read_moments()
    b = api.Renderer(sc, W, H, max_bounces=DEPTH, flags=api.FLAG_ADAPTIVE)
    b.write_accumulation(*frame)
    with pytest.raises(api.PtError) as e:
        b.render_adaptive(M, **crit)
    assert e.value.code == -3, "pt_write_accumulation without pt_write_moments"
    with pytest.raises(api.PtError) as e:
        b.adaptive_mask(**crit)
    assert e.value.code == -3
    b.write_moments(q)
    for _ in range(3):
        b.render_adaptive(M, **crit)
    for x, y, w in zip(b.read_frame(), whole.read_frame(), ("accumulation", "position", "id")):
        assert_bit_equal(x, y, f"resumed {w}")
    assert_bit_equal(b.read_moments(), whole.read_moments(), "resumed moments")
    counts = whole.read_frame()[0][..., 3]
    assert counts.max() <= 12 and counts.min() >= MIN, "max_samples is honoured"
    assert not whole.adaptive_mask(**crit).any(), "after five rounds every pixel has converged or reached the cap"
    _final_vs_oracle(ex, whole, counts.astype(np.int64), "checkpoint")
    # counts beyond 2^24 are not exact in f32: PT_ERR_LIMIT, before anything is rendered
    acc = frame[0].copy()
    acc[3, 5, 3] = float(2 ** 24 + 2)
    b.write_accumulation(acc, frame[1], frame[2])
    b.write_moments(q)
    with pytest.raises(api.PtError) as e:
        b.render_adaptive(M, **crit)
    assert e.value.code == -5
    with pytest.raises(api.PtError) as e:
        b.adaptive_mask(**crit)
    assert e.value.code == -5
    acc[3, 5, 3] = float(2 ** 24)          # the largest exact count is fine
    b.write_accumulation(acc, frame[1], frame[2])
    b.write_moments(q)
    b.adaptive_mask(**crit)
    # pt_frame adds a sample without Q; pt_reset_accumulation makes the moments valid again
    b.reset_accumulation()
    b.frame(0)
    with pytest.raises(api.PtError) as e:
        b.render_adaptive(M, **crit)
    assert e.value.code == -3
    b.reset_accumulation()
    assert b.render_adaptive(M, **crit) == W * H
