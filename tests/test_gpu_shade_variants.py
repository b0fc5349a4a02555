"""GPU: the surface shading variants that no other test launches: a TEXTURED scene under a projection, and a textured scene on an adaptive
list under a lens, a projection or (for textured lights) the pinhole.  Each case is one (surface, camera, route): the texel-corner rooms of
tests/textures_common.py and tests/emission_common.py, plain or under flat normal maps, against the oracle's render of the untextured
equivalent under the same camera, bit for bit.  A launch that reached another valid kernel (another surface, camera or path set) would read
other colours, origins, draw counts or pixels."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from variant_census_common import CAMERAS, DEPTH, EXTRAS, LENS, PinholeExpect, H, M, W  # noqa: F401  (the rooms and expectations are the census's)
from variant_census_common import expect, room, with_all_classes as _with_all_classes  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
# surface -> (room, flat normal maps on top): TEX, TEX + NMAP, TEX + EMTEX, all three.  The corner room keeps its glass boxes (media), the
# lamps room is built without them, so both halves of the variants run
SURFACES = {"tex": ("corner", False), "tex_nmap": ("corner", True), "tex_emtex": ("lamps", False), "tex_emtex_nmap": ("lamps", True)}


@pytest.fixture(scope="module")
def api():
    from path_tracer_amd import api
    api.lib()
    return api


def _room(name):
    """(textured description, untextured equivalent) of a room, both with the two extra boxes (and without the census's panel)"""
    return room(name, panel=False)


def _expect(O, name, camera):
    return expect(O, name, camera, panel=False)


def _textured(surface):
    from test_gpu_normalmap import flat_mapped
    room, flat = SURFACES[surface]
    tex = _room(room)[0]
    return flat_mapped(tex) if flat else tex


def _renderer(api, surface, camera, flags=0):
    r = api.Renderer(_textured(surface), W, H, max_bounces=DEPTH, flags=flags)
    if camera == "lens":
        r.set_lens(*LENS)
    elif camera != "pinhole":
        r.set_projection(*CAMERAS[camera])
    return r


def _assert_all_classes_seen(desc, ex, samples):
    """the camera's first hits reach both extra boxes and a wall: with the GGX boxes in front of the camera no class's queue stays empty"""
    ids = set(int(i) for s in samples for i in np.unique(ex.sample(s)[2]))
    names = [m.name for m in desc.models]
    for want in EXTRAS + ("back", "block"):
        assert names.index(want) in ids, f"no camera ray ends on {want}"


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("surface", list(SURFACES))
def test_samples_and_frame(api, oracle_mod, surface, camera):
    """pt_render_samples and a cleared pt_render of a textured room under a lens or a projection: radiance, accumulation, position, id history"""
    room = SURFACES[surface][0]
    ex = _expect(oracle_mod, room, camera)
    _assert_all_classes_seen(_room(room)[1], ex, range(M))
    r = _renderer(api, surface, camera)
    got = r.render_samples(0, M)
    assert_bit_equal(got, np.stack([ex.sample(s)[0] for s in range(M)]), f"{surface} {camera}: per-sample radiance")
    r.reset_accumulation()
    acc, pos, idb = r.render(0, M, ident=np.zeros((H, W), np.uint32))
    oacc, opos, oid = ex.frame(M)
    assert_bit_equal(acc, oacc, f"{surface} {camera}: accumulation")
    assert_bit_equal(pos, opos, f"{surface} {camera}: position")
    assert np.array_equal(idb, oid), f"{surface} {camera}: id history"


ADAPTIVE = [(s, c) for s in SURFACES for c in CAMERAS] + [("tex_emtex", "pinhole"), ("tex_emtex_nmap", "pinhole")]


@pytest.mark.parametrize("surface,camera", ADAPTIVE)
def test_two_adaptive_rounds(api, oracle_mod, surface, camera):
    """two rounds of pt_render_adaptive (the second over an adaptive list): every pixel ends with exactly pt_render(0, n_p)'s bits, n_p its own
    count (test_gpu_projection.py's statement under a panorama)"""
    ex = _expect(oracle_mod, SURFACES[surface][0], camera)
    first = np.stack([ex.sample(s)[0] for s in range(M)])
    lum = 0.2126 * first[..., 0] + 0.7152 * first[..., 1] + 0.0722 * first[..., 2]
    rel = np.sqrt(lum.var(0) / M) / np.maximum(lum.mean(0), 1e-3)
    threshold = float(np.quantile(rel[rel > 0], 0.5))     # the median relative error of the noisy pixels: the second round is a proper subset
    assert 0 < int((rel > threshold).sum()) < W * H, "the oracle's own error should split the frame"
    r = _renderer(api, surface, camera, flags=api.FLAG_ADAPTIVE)
    assert r.render_adaptive(M, threshold, 0.0, M, 0) == W * H
    second = r.render_adaptive(M, threshold, 0.0, M, 0)
    assert 0 < second < W * H, second
    acc, pos, idb = r.read_frame()
    counts = np.rint(acc[..., 3]).astype(np.int64)
    assert set(np.unique(counts)) == {M, 2 * M}, np.unique(counts)
    assert int((counts == 2 * M).sum()) == second
    for n in (M, 2 * M):
        sel = counts == n
        oacc, opos, oid = ex.frame(n)
        assert_bit_equal(acc[sel], oacc[sel], f"{surface} {camera}: accumulation of the {int(sel.sum())} pixels with {n} samples")
        assert_bit_equal(pos[sel], opos[sel], f"{surface} {camera}: position of the pixels with {n} samples")
        assert np.array_equal(idb[sel], oid[sel]), f"{surface} {camera}: id history of the pixels with {n} samples"
