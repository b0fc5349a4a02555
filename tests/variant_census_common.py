"""The variant census: a static table of small cases that between them launch EVERY kernel the keyed launchers compile (the surface pass's six
axes, the terminal pass, the traversal kernels, k_generate, k_guide_rays, k_accumulate), each with work in its queue, and the set of variants
every case must launch.  tests/test_variant_census_host.py holds the union of those sets to the library's own enumeration
(pt_variant_axes / pt_variant_compiled); tests/test_gpu_variant_census.py runs each case against the oracle bit for bit and holds the
launch log (pt_last_launches) to the case's set.  Nothing here calls the library or the device.

A case's set is stated from the case's own facts (which classes its room holds, media, surface, camera, route, flags), by the rules DESIGN.md
gives for which kernel serves which scene; it never asks the library which points exist.  Axis values are include/pt_api.h's."""
import dataclasses

import numpy as np

from emission_common import emission_corner_scene
from projection_common import ORTHOGRAPHIC, PANORAMA
from textures_common import box, corner_scene

F = np.float32
W, H, DEPTH, M = 32, 24, 4, 3
FLAG_NO_LDS_SCENE, FLAG_TIMING_ALL, FLAG_GENERAL_WALK, FLAG_ADAPTIVE = 2, 4, 16, 32     # include/pt_api.h
SPILL_LEVELS = 2            # pt_config.stack_lds_levels of the spilling cases: every deeper stack level lives in global memory

# ---------------------------------------------------------------------------------------------------------------------------------- cameras
LENS = (0.6, 9.0)
CAMERAS = {"lens": None, "panorama": (PANORAMA, 360.0, 180.0, 0.0), "ortho": (ORTHOGRAPHIC, 0.0, 0.0, 18.0)}
# the Cornell rooms are fifty times the size
LENS_CORNELL = (40.0, 800.0)
CAMERAS_CORNELL = {"lens": None, "panorama": (PANORAMA, 360.0, 180.0, 0.0), "ortho": (ORTHOGRAPHIC, 0.0, 0.0, 600.0)}
CAM_KIND = {"pinhole": 0, "lens": 1, "panorama": 2, "ortho": 3}
FIRST0 = {"pinhole": 0, "lens": 1, "panorama": 2, "ortho": 2}       # the surface pass's `first` axis at bounce 0

# ------------------------------------------------------------------------------------------------------------------------------------ rooms
EXTRAS = ("extra_mirror", "extra_glass")
Q_LAMBERT, Q_SPECULAR, Q_DIELECTRIC, Q_GGX = 1, 2, 3, 4


def with_all_classes(desc):
    """desc plus an untextured mirror box and a smooth glass box (no volume): with the room's Lambertian walls and GGX boxes the scene then
    holds all four shading classes"""
    from path_tracer_amd.scene_desc import Dielectric, Model, SceneDesc, Specular
    mp, mn = box((7.2, -9.99, -6.5), (9.7, 4.0, -3.5))
    gp, gn = box((-9.5, -9.99, -9.5), (-6.5, 2.0, -6.5))
    extras = [Model.new(mp, mn, Specular.new((0.95, 0.9, 0.85)), None, EXTRAS[0]), Model.new(gp, gn, Dielectric.new((0.9, 1.0, 0.95), 1.5), None, EXTRAS[1])]
    return SceneDesc.new(list(desc.models) + extras, desc.camera, desc.name)


def with_panel(desc):
    """desc plus a dim emissive panel on the back wall, in every camera's view: a camera ray that ends on a light is what the terminal pass
    of bounce 0 works on (a miss without an environment map is finished by the traversal kernel)"""
    from path_tracer_amd.scene_desc import Emissive, Model, SceneDesc
    from textures_common import quad
    p, n = quad((-3.0, 2.5, -9.9), (3.0, 2.5, -9.9), (3.0, 6.0, -9.9), (-3.0, 6.0, -9.9))
    return SceneDesc.new(list(desc.models) + [Model.new(p, n, Emissive.new((2.0, 2.5, 3.0)), None, "panel")], desc.camera, desc.name)


def identity_only(desc):
    """desc with ONE identity instance of every model: both TLASes then hold identity instances only (the one-ray walk)"""
    from path_tracer_amd.scene_desc import Model, SceneDesc
    models = [Model.new(m.positions, m.normals, m.material, None, m.name, uvs=m.uvs) for m in desc.models]
    return SceneDesc.new(models, desc.camera, desc.name + ", identity instances")


SMALL = ("light", "floor", "back", "left", "right", "block", "extra_mirror", "extra_glass", "panel")


def small(desc):
    """nine models of the dry corner room (no ceiling, slab or tall box).  The Lambertian pass walks its own shadow rays only where the
    scene's BVH and a workgroup's traversal stacks fit 31 KB of LDS (shade_traces_shadow); the whole room needs about 34 KB, this one 29.5"""
    from path_tracer_amd.scene_desc import SceneDesc
    return SceneDesc.new([m for m in desc.models if m.name in SMALL], desc.camera, desc.name + ", small")


@dataclasses.dataclass(frozen=True)
class RoomFacts:
    classes: tuple          # the shading classes its instances hold
    media: int              # 1: some material has a volume
    ident_world: bool       # every world-TLAS instance is an identity
    ident_lights: bool      # ... every lights-TLAS instance
    inline_fits: bool = False  # the BVH and the traversal stacks fit the inline shadow walk's LDS budget
    cornell: bool = False   # Cornell scale (CAMERAS_CORNELL)


ALL = (Q_LAMBERT, Q_SPECULAR, Q_DIELECTRIC, Q_GGX)
ROOMS = {
    # the texel-corner rooms (textures_common / emission_common), each with the two extra boxes; the corner room's block has a translated
    # second instance and the lamps are turned and doubled, so their TLASes take the general walk
    "corner": RoomFacts(ALL, 1, False, True),
    "corner_dry": RoomFacts(ALL, 0, False, True),
    "lamps": RoomFacts(ALL, 0, False, False),
    "lamps_wet": RoomFacts(ALL, 1, False, False),
    # nine models of the dry corner room, small enough for the inline shadow walk: as they are (the block's second instance: the general
    # walk) and with identity instances only (the one-ray walk)
    "small": RoomFacts(ALL, 0, False, True, True),
    "small_id": RoomFacts(ALL, 0, True, True, True),
    "lamps_id": RoomFacts(ALL, 0, True, True),
    "cornell": RoomFacts((Q_LAMBERT,), 0, True, True, True, True),
}
_ROOMS = {}


def _cornell_lit():
    """the Cornell box with a second, large emitter just inside its right wall (test_gpu_parity's spill scene has the same): enough
    BSDF-sampled NEE rays pass the lights' root box that their launch has work at the last bounce too"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Emissive, Model, SceneDesc
    base = scenes.cornell_box(W, H)
    wall = scenes.cornell_models()[2]
    big = Model.new(wall.positions * F(0.98), wall.normals, Emissive.new((2.0, 1.5, 1.0)), None, "big_light")
    return SceneDesc.new(list(base.models) + [big], base.camera, "cornell, two lights")


def room(name, panel=True):
    """(textured description or None, untextured equivalent) of a room.  panel=False: the corner and lamps rooms as
    tests/test_gpu_shade_variants.py has always rendered them, without the census's emissive panel"""
    key = (name, panel)
    if key not in _ROOMS:
        dress = (lambda d: with_panel(with_all_classes(d))) if panel else with_all_classes
        if name in ("corner", "corner_dry"):
            tex, plain = corner_scene(W, H, media=name == "corner")
            _ROOMS[key] = (dress(tex), dress(plain))
        elif name in ("lamps", "lamps_wet"):
            tex, plain = emission_corner_scene(W, H, media=name == "lamps_wet")
            _ROOMS[key] = (dress(tex), dress(plain))
        elif name in ("small", "small_id"):
            plain = small(room("corner_dry")[1])
            _ROOMS[key] = (None, identity_only(plain) if name == "small_id" else plain)
        elif name == "lamps_id":
            tex, plain = room("lamps")
            _ROOMS[key] = (identity_only(tex), identity_only(plain))
        else:
            assert name == "cornell", name
            _ROOMS[key] = (None, _cornell_lit())
    return _ROOMS[key]


# surface -> (the `surface` axis, emission texture, flat normal maps on top)
SURFACES = {"plain": (0, False, False), "tex": (1, False, False), "tex_emtex": (2, True, False), "tex_nmap": (3, False, True), "tex_emtex_nmap": (4, True, True)}


def textured(room_name, surface):
    """the description a case renders: the room under the surface"""
    tex, plain = room(room_name)
    if surface == "plain":
        return plain
    assert tex is not None and SURFACES[surface][1] == room_name.startswith("lamps"), (room_name, surface)
    if SURFACES[surface][2]:
        from test_gpu_normalmap import flat_mapped
        return flat_mapped(tex)
    return tex


def cameras_of(room_name):
    return (LENS_CORNELL, CAMERAS_CORNELL) if ROOMS[room_name].cornell else (LENS, CAMERAS)


# ------------------------------------------------------------------------------------------------------------------------------ expectations
class PinholeExpect:
    """the oracle's own camera: per-sample radiance and whole frames of the first n samples"""

    def __init__(self, O, scene):
        self.orc = O.Oracle(scene)
        self.samples = self.orc.render_samples(W, H, 2 * M, max_bounces=DEPTH)
        self.frames = {}

    def sample(self, s):
        """radiance, first-hit position and id byte of sample s (a frame of s + 1 samples ends with that sample's position and id)"""
        f = self.frame(s + 1)
        return self.samples[s], f[1], f[2] & np.uint32(0xFFFF)

    def frame(self, n):
        if n not in self.frames:
            self.frames[n] = self.orc.render(W, H, n, max_bounces=DEPTH)[:3]
        return self.frames[n]


_EXPECT = {}


def expect(O, room_name, camera, panel=True):
    """the oracle's expectation of a plain room under a camera, one per (room, camera)"""
    key = (room_name, camera, panel)
    if key not in _EXPECT:
        plain = room(room_name, panel)[1]
        lens, cams = cameras_of(room_name)
        if camera == "pinhole":
            _EXPECT[key] = PinholeExpect(O, plain)
        elif camera == "lens":
            from test_gpu_lens import Expect
            _EXPECT[key] = Expect(O, room_name, lens=lens, w=W, h=H, depth=DEPTH, scene=plain)
        else:
            from test_gpu_projection import Expect
            _EXPECT[key] = Expect(O, room_name, camera, w=W, h=H, depth=DEPTH, scene=plain, params=cams[camera])
    return _EXPECT[key]


# ------------------------------------------------------------------------------------------------------------------------------------ cases
ROUTES = ("render", "adaptive", "rays", "guides", "hooks")


@dataclasses.dataclass(frozen=True)
class Case:
    """one renderer and one route through it:
    render    pt_render_samples(0, M), then a cleared pt_render(0, M)  (the active rectangle; with FLAG_ADAPTIVE the frame keeps moments)
    adaptive  two pt_render_adaptive rounds of M samples, the second over a proper subset of the pixels      (adaptive lists, both rounds)
    rays      pt_integrate_rays of the lens camera's rays of samples 0 .. M - 1 of every pixel, two draws consumed (a ray table; as many
              paths as a render's batch: with the 768 rays of one sample the mirror's queue was measured empty at bounce 4)
    guides    pt_render_guides(0)                                                                          (k_guide_rays + the hook walk)
    hooks     pt_trace_closest against both TLASes and pt_trace_any                                        (the hook walks)"""
    room: str
    surface: str
    camera: str
    route: str
    flags: int = 0
    spill: bool = False

    @property
    def id(self):
        f = "".join(s for bit, s in ((FLAG_NO_LDS_SCENE, "-global"), (FLAG_GENERAL_WALK, "-general"), (FLAG_TIMING_ALL, "-apart"), (FLAG_ADAPTIVE, "-moments")) if self.flags & bit)
        return f"{self.room}-{self.surface}-{self.camera}-{self.route}{f}{'-spill' if self.spill else ''}"

    @property
    def config_flags(self):
        return self.flags | (FLAG_ADAPTIVE if self.route == "adaptive" else 0)

    def idle(self):
        """of variants(), what the case launches over an EMPTY queue by the scene's nature and so does not vouch for: in a scene with media an
        emissive hit belongs to the Lambertian pass (the volume interaction comes first and may scatter the path on), and a miss without an
        environment map is finished by the traversal kernel, so nothing reaches the terminal queue of bounce 0.  Under the pinhole the same
        terminal kernel serves the later bounces, where paths that owe an NEE resolve end; a camera with origins of its own has a kernel of
        its own at bounce 0, and that one idles"""
        first0 = 1 if self.route == "rays" else FIRST0[self.camera]
        if self.route in ("render", "adaptive", "rays") and ROOMS[self.room].media and first0:
            return frozenset({("terminal", (1, 1 if SURFACES[self.surface][1] else 0))})
        return frozenset()

    def variants(self):
        """the exact set of (launcher, axis values) the case must launch; all but idle() with work"""
        facts = ROOMS[self.room]
        surf, emtex, _ = SURFACES[self.surface]
        bvh = 0 if self.flags & FLAG_NO_LDS_SCENE else 1                    # every room here fits LDS (and no walk spills unless told to)
        spill = 1 if self.spill else 0
        general = bool(self.flags & FLAG_GENERAL_WALK)
        iw = 1 if facts.ident_world and not general else 0                   # the one-ray walk of a launch through the world TLAS
        il = 1 if facts.ident_lights and not general else 0
        kind = CAM_KIND[self.camera]
        out = set()
        if self.route == "hooks":
            return frozenset({("closest", (2, bvh, spill, iw)), ("closest", (2, bvh, spill, il)), ("any", (2, bvh, spill, iw))})
        if self.route == "guides":
            return frozenset({("guide_rays", (kind,)), ("closest", (2, bvh, spill, iw))})
        # the Lambertian pass walks its own shadow rays in an untextured scene without media whose BVH and stacks stay in LDS
        inline = surf == 0 and not facts.media and bvh == 1 and not spill and facts.inline_fits
        lambert_shadow = 0 if not inline else 2 if iw else 1
        fused = bvh == 1 and not emtex and not (self.flags & FLAG_TIMING_ALL)   # world closest hit + the NEE rays of the bounce before in one launch
        paths, first0 = {"render": (0, FIRST0[self.camera]), "adaptive": (1, FIRST0[self.camera]), "rays": (2, 1)}[self.route]
        for q in facts.classes:
            for first in (first0, 0):                                    # bounce 0, the later bounces
                out.add(("shade", (q, facts.media, lambert_shadow if q == Q_LAMBERT else 0, paths, first, surf)))
        out.add(("terminal", (1 if first0 else 0, 1 if emtex else 0)))
        out.add(("terminal", (0, 1 if emtex else 0)))
        out.add(("closest", (4 if first0 else 3, bvh, spill, iw)))       # the camera rays / rays with origins of their own
        if fused:
            out.add(("fused", (bvh, spill, iw & il)))
        else:
            out.add(("closest", (5 if emtex else 0, bvh, spill, iw)))
        out.add(("closest", (1, bvh, spill, iw & il)))                   # the NEE rays (a fused batch: those of its last bounce)
        if not inline or Q_GGX in facts.classes:                         # (GGX surfaces always queue their shadow rays)
            out.add(("any", (0, bvh, spill, iw)))
        if self.route != "rays":
            out.add(("generate", (kind, 1 if paths == 1 else 0)))
        if self.route == "render":
            out.add(("accumulate", (kind, 1, 1 if self.flags & FLAG_ADAPTIVE else 0)))
        elif self.route == "adaptive":
            out.add(("accumulate", (kind, 1, 2)))
        return frozenset(out)


def _cases():
    out = []
    pairs = [(route, cam) for route in ("render", "adaptive") for cam in ("pinhole", "lens", "panorama")] + [("rays", "pinhole")]
    for route, cam in pairs:
        # the queued surface passes: classes x media x surfaces
        for wet in (False, True):
            for surface in SURFACES:
                name = ("lamps_wet" if wet else "lamps") if SURFACES[surface][1] else ("corner" if wet else "corner_dry")
                out.append(Case(name, surface, cam, route))
        # the small room's Lambertian pass walks its shadow rays: the general walk, and one ray where every instance is an identity
        out += [Case("small", "plain", cam, route), Case("small_id", "plain", cam, route)]
    # the orthographic camera's generate / accumulate kernels
    out += [Case("corner", "tex", "ortho", "render"), Case("corner", "tex", "ortho", "adaptive")]
    # the Cornell box (with a second light): identity instances, Lambertian surfaces only, so no shadow ray is ever queued
    out.append(Case("cornell", "plain", "pinhole", "render"))
    # a frame that keeps moments (FLAG_ADAPTIVE) and is rendered whole: k_accumulate's second mode, per camera
    out += [Case("corner_dry", "plain", cam, "render", FLAG_ADAPTIVE) for cam in CAM_KIND]
    # the traversal kernels: BVH in LDS / global memory x stack spill x one-ray walk
    for flags in (0, FLAG_NO_LDS_SCENE, FLAG_GENERAL_WALK, FLAG_NO_LDS_SCENE | FLAG_GENERAL_WALK):
        for spill in (False, True):
            if flags or spill:                                                                 # (the shading block has the plain ones)
                out.append(Case("small_id", "plain", "pinhole", "render", flags, spill))      # camera rays, world / fused, lights, shadow
                out.append(Case("small_id", "plain", "pinhole", "rays", flags, spill))        # rays with origins of their own
            out.append(Case("lamps_id", "tex_emtex", "pinhole", "render", flags, spill))   # the world launch of a scene with textured lights
            out.append(Case("small_id", "plain", "pinhole", "hooks", flags, spill))
            if not flags & FLAG_NO_LDS_SCENE:
                out.append(Case("small_id", "plain", "pinhole", "render", flags | FLAG_TIMING_ALL, spill))   # world launches apart with the BVH in LDS
    # k_guide_rays per camera
    out += [Case("corner_dry", "plain", cam, "guides") for cam in CAM_KIND]
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
LAUNCHERS = ("shade", "terminal", "closest", "any", "fused", "generate", "guide_rays", "accumulate")


def table_variants(cases=None):
    """the union of what the cases launch WITH WORK"""
    out = set()
    for c in CASES if cases is None else cases:
        out |= c.variants() - c.idle()
    return out
