"""Chain-shaped ("caterpillar") trees that drive every traversal walk to the top of its per-lane stack, rays designed to get there, and a
walk simulator that is not the kernel: plain Python over the dumped trees, binary64 box and triangle tests, the push disciplines as the
kernels' comments state them (pt_kernels.hip: closest_body, any_body, the fused launch's any-phase, inline_any).

The simulator decides a box or triangle test only where binary64 leaves a margin (MARGIN, relative): a designed ray that comes closer
than that to a decision raises MarginError, it is never dropped.  test_stack_bound_host.py holds the simulated occupancy against
reachable() and against HostScene::flatten's bound; test_gpu_stack_bound.py runs the same rays on the device against the oracle."""
import numpy as np

from path_tracer_amd.scene_desc import affine_from_rotation_translation, is_rigid, quat_unit
from path_tracer_amd.scene_desc import Camera, Emissive, Lambertian, Model, SceneDesc

EPS = 5e-4                      # PT_EPSILON (utility.rs:4)
MARGIN = 1e-3
BRANCH_LEVELS = {"closest": 4, "any": 4, "inline_any": 6, "fused_any": 1}   # PT_BRANCH_LEVELS, _ANY, _INLINE; the fused any-phase expands one node per step
DISCIPLINES = tuple(BRANCH_LEVELS)
F32 = np.float32


class MarginError(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------------ scenes
def _plate(x, h, sign=1.0):
    """an isosceles triangle perpendicular to x at sign * x in the box y, z in [-h, h]: base along z = -h, apex (0, h).  The box's centre is
    well inside it (barycentrics 1/4, 1/4, 1/2), the corners y = +-0.75 h, z = 0.5 h well outside"""
    p = np.array([[sign * x, -h, -h], [sign * x, h, -h], [sign * x, 0.0, h]], np.float64)
    n = np.tile(np.array([[-sign, 0.0, 0.0]]), (3, 1))
    return p, n


def _plates(ks, scale, sign, grow=True):
    P, N = zip(*[_plate(scale * 2.0 ** k, 0.4 * scale * (2.0 ** k if grow else 1.0), sign) for k in ks])
    return np.stack(P).astype(F32), np.stack(N).astype(F32)


GREY = Lambertian.new((0.7, 0.7, 0.7))
SAH_SCALE = 2.0 ** -8           # blas_chain('left'): the smallest plate stays ten times PT_EPSILON from a ray's origin, the largest (2^55) squares inside binary32
GIANT = 2.0 ** 63
GIANTS = (0.5 * GIANT, GIANT)
GLOW = Emissive.new((1.5, 1.25, 1.0))


def _lit_camera(sign, scale, aspect=16 / 12):
    """beside the dense end, looking along the chain at the lit faces of the plates behind the light"""
    return Camera.new((-sign * 0.2 * scale, 3.0 * scale, 1.0 * scale), (sign * 3.0 * scale, 0.0, 0.0), 70.0, aspect)


def _plate_camera(sign, aspect=16 / 12):
    """where the plates do not grow: between the light and the second plate, which fills the frame"""
    return Camera.new((sign * 1.6, 0.15, 0.1), (sign * 2.0, 0.0, -0.1), 90.0, aspect)


def _camera(sign, scale, aspect=16 / 12):
    return Camera.new((-sign * 6.0 * scale, 1.5 * scale, 2.5 * scale), (sign * 16.0 * scale, 0.0, 0.0), 50.0, aspect)


def _light_plate(scale=1.0, grow=True, k=-1, sign=1.0):
    """the emitter: a plate of the chain's own progression at x = sign * 2^k * scale (k = -1: before the first plate; k = 0.5: between the first two,
    where it lights the plates behind it and a ray from the dense end enters the chain's box first, so that the light is pending underneath),
    a model of its own.  A ray has to meet every link of a chain to fill the stack, the light's leaf included, so the light is a link like the
    others and not something beside them"""
    p, n = _plate(2.0 ** k * scale, 0.4 * scale * (2.0 ** k if grow else 1.0), sign)
    return Model.new(p[None].astype(F32), n[None].astype(F32), Emissive.new((12.0, 10.0, 8.0)), None, "light")


def _chain_model(small, name):
    """`small` plates and the two GIANTS behind them: a BLAS that is a chain about as deep as it has plates WHATEVER the small plates' places.  With the
    giants in a node, count * area of every SAH candidate AND the node's own area overflow binary32 (blas_bvh.rs:96-112 as written: the reference's
    tree, the oracle builds the same): every cost is inf / inf = NaN, min_by keeps the FIRST candidate, no leaf cost is below a NaN, and the sweep
    splits off the plate of the smallest x: that leaf is the left child, the rest of the chain the right one.
    Such a model must be the scene's ONLY TLAS leaf: joined to anything its box's area is +inf, and the reference's agglomeration finds no partner
    then (tlas_bvh.rs:56-83 returns usize::MAX and Vec::swap_remove panics).  So the model is its own light: EMISSIVE, and both TLASes hold it."""
    P, N = zip(*(list(small) + [_plate(g, 0.4 * g) for g in GIANTS]))
    return Model.new(np.stack(P).astype(F32), np.stack(N).astype(F32), GLOW, None, name)


def deep_chain_model(n, name="deep_chain"):
    """n - 2 plates of half-size 0.4 at x = 1 .. n - 2, and the giants"""
    return _chain_model([_plate(float(k + 1), 0.4) for k in range(n - 2)], name)


def deep_chain(n):
    return SceneDesc.new([deep_chain_model(n)], _camera(1.0, 0.25), f"deep_chain_{n}")


def blas_chain(side, n=64):
    """ONE model of n plates at identity, half-size 0.4 of their distance.
    'right': at x = 2^k, the last two being the giants of _chain_model: every node splits off its smallest plate as the LEFT leaf and the chain hangs
    off RIGHT children, which is the any-walks' worst case.  The model is the scene's only TLAS leaf and its own light.
    'left': n plates at 2^(k - 8), where nothing overflows: the sweep splits the two or three LARGEST plates off to the right at every level, so the
    (shallower) chain hangs off LEFT children: the closest-walk's worst case and not the any-walks'.
    'mirrored': 'left' at -2^(k - 8): the same tree with left and right exchanged, a chain off RIGHT children whose plates are Lambertian: the shadow and
    next-event rays of its frame are the any-walks' worst case (the overflow chain has no surface that casts one).
    In both the light is the TLAS root's other leaf, between the first two plates: BEHIND the chain's box for the rays that descend it from the dense end."""
    if side == "right":
        model = _chain_model([_plate(2.0 ** k, 0.4 * 2.0 ** k) for k in range(n - 2)], "chain_right")
        return SceneDesc.new([model], _camera(1.0, 1.0), "blas_chain_right")
    sign = {"left": 1.0, "mirrored": -1.0}[side]
    p, nr = _plates(range(n), SAH_SCALE, sign)
    light = _light_plate(SAH_SCALE, True, 0.5, sign)
    return SceneDesc.new([Model.new(p, nr, GREY, None, f"chain_{side}"), light], _lit_camera(sign, SAH_SCALE), f"blas_chain_{side}")


def inline_limit(levels):
    """blas_chain('mirrored') cut to 2 * levels - 8 plates: stack_entries == levels (8 <= levels <= 16; the host test pins it), Lambertian plates under a
    light of their own, so the frame's shadow rays climb a right-hanging chain: the scenes either side of the inline shadow walk's LDS limit"""
    return blas_chain("mirrored", 2 * levels - 8)


def _translations(xs):
    m = np.tile(np.eye(3, 4, dtype=F32), (len(xs), 1, 1))
    m[:, 0, 3] = np.asarray(xs, F32)
    return m


def tlas_chain(side, n=16):
    """one single-triangle model under n translations to x = +-2^k: no instance is an identity, so the general walk.  The agglomeration
    (tlas_bvh.rs:56-136) joins the two nearest and then the next one out, every time: a chain as deep as it has leaves"""
    sign = {"left": 1.0, "right": -1.0}[side]
    p, nr = _plate(0.0, 0.4)
    light = _light_plate(1.0, False, 0.5, sign)
    models = [Model.new(p[None], nr[None], GREY, _translations([sign * 2.0 ** k for k in range(n)]), f"tlas_chain_{side}"), light]
    return SceneDesc.new(models, _plate_camera(sign), f"tlas_chain_{side}")


def ident_chain(side, n=16):
    """n one-plate models, each at identity: the IDENT kernels (PT_FLAG_GENERAL_WALK: the general ones)"""
    sign = {"left": 1.0, "right": -1.0}[side]
    models = []
    for k in range(n):
        p, nr = _plate(2.0 ** k, 0.4, sign)
        models.append(Model.new(p[None], nr[None], GREY, None, f"plate{k}"))
    models.append(_light_plate(1.0, False, 0.5, sign))
    return SceneDesc.new(models, _plate_camera(sign), f"ident_chain_{side}")


BOTH_PLATES, BOTH_INSTANCES = 24, 27
BALLAST = 345
BOTH_SCALE = 2.0 ** -8
BOTH_RATIO = 3.0                # (at exactly 2 a pair of placements and the cluster below them join to boxes of EQUAL area: pairs, not a chain)
BOTH_SPACING = 2.0 ** 19        # the first placement: eight times the model's extent (2^15 = 2^-8 * 2^23); placement k at 2^k times this


def both_rotation():
    """the rotation (glam-built, passes is_rigid) of both_chains' deep instance, the one at the origin: a general angle about x, so that the chain's
    axis is the world's x and the placements along it agglomerate into a pure chain as tlas_chain's do"""
    for w in range(2, 40):
        m = affine_from_rotation_translation(quat_unit(3, 0, 0, w), (0.0, 0.0, 0.0))
        if is_rigid(m) and abs(m[1, 2]) > 0.05:
            return m
    raise AssertionError("no rigid rotation about x found")


def both_chains(ballast=0):
    """a chain BLAS (BOTH_PLATES plates, no overflow: depth about 0.45 per plate) instanced along a TLAS chain: the deep instance sits at the ORIGIN under a
    general rotation (its chain axis is the world direction `a`; rays along it are exact in the model's frame to 1e-7 of a unit), the others at
    2^k * BOTH_SPACING * a with their apex on that line: quarter turns, a second general rotation and the first again, each opening towards +a
    so that the ray enters its box.  BLAS entries then lie on top of every pending TLAS entry."""
    p, nr = _plates(range(BOTH_PLATES), BOTH_SCALE, 1.0)
    R0 = both_rotation()
    a = R0[:, :3].astype(np.float64) @ np.array([1.0, 0.0, 0.0])
    quarter = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0]], F32)       # a quarter turn about x
    turns = [affine_from_rotation_translation(quat_unit(w, 0, 0, 5), (0.0, 0.0, 0.0)) for w in range(1, 30)]
    turns = [m for m in turns if is_rigid(m) and abs(m[1, 2]) > 0.05][:4]     # other general angles about x: every placement's cone holds the axis
    assert len(turns) == 4
    mats = [R0]
    for k in range(BOTH_INSTANCES - 1):
        m = (quarter if k % 5 == 1 else turns[k % 4]).copy()
        m[:, 3] = (a * BOTH_SPACING * BOTH_RATIO ** k).astype(F32)
        mats.append(m)
    light = _light_plate(BOTH_SCALE, True, 0.5)         # between the deep instance's first two plates, in its frame
    if ballast:
        # `ballast` tiny emissive triangles IN the light plate's plane, in a corner of its box no designed ray crosses: no box of the TLAS changes, the
        # staged BVH grows by about 112 bytes each (both_chains_ballast: enough that 64-thread workgroups need more than 64 KiB of LDS)
        rng = np.random.default_rng(23)
        x = light.positions[0, 0, 0]
        c = np.stack([np.full(ballast, x), rng.uniform(-0.5, -0.42, ballast), rng.uniform(0.3, 0.5, ballast)], axis=1)[:, None, :] * [1.0, BOTH_SCALE, BOTH_SCALE]
        tri = c + np.array([[0, 0, 0], [0, 0.004, 0], [0, 0, 0.004]]) * BOTH_SCALE
        light = Model.new(np.concatenate([light.positions, tri.astype(F32)]), np.tile(light.normals[:1], (ballast + 1, 1, 1)), light.material, None, "light")
    light.matrices = R0[None].copy()
    return SceneDesc.new([Model.new(p, nr, GREY, np.stack(mats), "both_chains"), light], _lit_camera(1.0, BOTH_SCALE), "both_chains")


LAMPS = 12


def lights_chain(n=LAMPS):
    """n emissive one-plate models at x = 2^k: the lights TLAS is their chain, n deep.  The world holds them too, and a grey sliver that spans each pair
    (2j, 2j + 1): the agglomeration joins a lamp to its sliver first, so the world's tree is a chain of TRIPLES, shallower than the lights'"""
    models = []
    for k in range(n):
        p, nr = _plate(2.0 ** k, 0.4)
        models.append(Model.new(p[None], nr[None], Emissive.new((4.0, 3.0, 2.0)), None, f"lamp{k}"))
    for j in range(n // 2):
        x0, x1 = 1.02 * 2.0 ** (2 * j), 1.5 * 2.0 ** (2 * j)
        # in the cross-section's bottom face z = -0.4: joined to lamp 2j its box is the lamp's cross-section from x0 to x1; the axis-parallel rays never meet its plane
        p = np.array([[[x0, -0.4, -0.4], [x1, -0.4, -0.4], [x1, 0.4, -0.4]]], F32)
        models.append(Model.new(p, np.tile(np.array([0.0, 0.0, 1.0], F32), (1, 3, 1)), GREY, None, f"sliver{j}"))
    # something for the lamps to light, so that the frame casts next-event rays (the fused launch walks the lights' chain, then the world from an empty stack)
    floor = np.array([[[-2.0, -2.0, -6.0], [40.0, -2.0, -6.0], [-2.0, -2.0, 6.0]]], F32)
    models.append(Model.new(floor, np.tile(np.array([0.0, 1.0, 0.0], F32), (1, 3, 1)), GREY, None, "floor"))
    return SceneDesc.new(models, _camera(1.0, 0.25), "lights_chain")


FORKED_PLATES = 40


def forked(n_clump=4200):
    """one model of more than 4096 triangles (the SAH root forks its subtrees): a compact clump of small triangles off the axis plus blas_chain('left')'s first 40 plates (no giants: their overflow would chain the clump as well)"""
    rng = np.random.default_rng(17)
    c = rng.uniform(-1.0, 1.0, (n_clump, 1, 3)) * 0.05 * SAH_SCALE + np.array([-3.0, 3.0, 3.0]) * SAH_SCALE
    cp = (c + rng.normal(0.0, 0.004 * SAH_SCALE, (n_clump, 3, 3))).astype(F32)
    cn = np.tile(np.array([0.0, 0.0, 1.0], F32), (n_clump, 3, 1))
    p, nr = _plates(range(FORKED_PLATES), SAH_SCALE, 1.0)
    models = [Model.new(np.concatenate([p, cp]), np.concatenate([nr, cn]), GREY, None, "forked"), _light_plate(SAH_SCALE, True, 0.5)]
    return SceneDesc.new(models, _camera(1.0, SAH_SCALE), "forked")


# ------------------------------------------------------------------------------------------------------------------------ dumped trees
class Trees:
    """what the simulator walks: both TLAS dumps, every BLAS dump, the leaves' inverse matrices and models, the models' triangles"""

    def __init__(self, r, desc):
        self.tlas = [r.tlas_dump(0), r.tlas_dump(1)]
        self.blas = [r.blas_dump(b) for b in range(r.blas_count())]
        self.inv = [r.tlas_instances(w)["inv_matrix"].astype(np.float64) for w in (0, 1)]
        # TLAS leaf -> model: the world's arena is the model list; the lights' is the emissive models in model order (HostTlas::models)
        lights = [i for i, m in enumerate(desc.models) if m.material.kind == 1]
        self.model_of = [list(range(len(desc.models))), lights]
        self.tris = [m.positions.astype(np.float64) for m in desc.models]

    @staticmethod
    def depth(d):
        """nodes on the longest root-to-leaf path: HostBlas::depth / HostTlas::depth evaluated from a dump"""
        if d["kind"].size == 0:
            return 0
        best, todo = 0, [(int(d["root"]), 1)]
        while todo:
            n, lv = todo.pop()
            best = max(best, lv)
            if d["kind"][n] == 0:
                todo += [(int(d["a"][n]), lv + 1), (int(d["b"][n]), lv + 1)]
        return best

    @staticmethod
    def leaves(d):
        return int((d["kind"] != 0).sum())

    def bound(self):
        """HostScene::flatten's stack_entries, evaluated from the dumps"""
        dt = max(self.depth(self.tlas[0]), self.depth(self.tlas[1]))
        db = max(self.depth(b) for b in self.blas)
        return max(dt, max(dt - 1, 0) + db)

    def bound_of(self, which):
        """the same formula for a walk that starts in TLAS `which` alone (what that walk could need at most)"""
        dt = self.depth(self.tlas[which])
        db = max(self.depth(self.blas[self.model_of[which][int(b)]]) for k, b in zip(self.tlas[which]["kind"], self.tlas[which]["b"]) if k != 0)
        return max(dt, dt - 1 + db)


# ------------------------------------------------------------------------------------------------------------------------ the walks
def _clear(x, y, what):
    """x and y (a computed distance and what it is compared with) differ by the margin, so binary32 decides as binary64 does"""
    if np.isinf(x) or np.isinf(y):
        if x == y:
            raise MarginError(f"{what}: both infinite")
        return
    if abs(x - y) <= MARGIN * max(abs(x), abs(y)):
        raise MarginError(f"{what}: {x!r} against {y!r}")


def _slab(box, o, d, t_max, what):
    """AABB::intersect_t in binary64 (pt_kernels.hip slab()): hit, t_enter.  Every comparison that decides it must be clear by MARGIN: a
    plane the ray is parallel to against its origin, and every near distance against every far distance of ANOTHER axis, PT_EPSILON
    and t_max (a flat box's own near and far distances are one number in either precision: that comparison is an equality by construction)"""
    tn, tf = np.empty(3), np.empty(3)
    for k in range(3):
        lo, hi = float(box[k]), float(box[3 + k])
        if d[k] == 0.0:
            for face in (lo, hi):
                if abs(o[k] - face) <= MARGIN * max(abs(o[k]), abs(face)):
                    raise MarginError(f"{what}: origin on plane {face!r} of axis {k}")
            if not lo < o[k] < hi:
                return False, np.inf     # beside the slab of an axis it runs along: (+inf, -inf) in either precision
            tn[k], tf[k] = -np.inf, np.inf
        else:
            t0, t1 = (lo - o[k]) / d[k], (hi - o[k]) / d[k]
            tn[k], tf[k] = min(t0, t1), max(t0, t1)
    for i in range(3):
        _clear(tf[i], EPS, f"{what}: far plane against epsilon")
        _clear(tn[i], t_max, f"{what}: near plane against t_max")
        for j in range(3):
            if i != j:
                _clear(tn[i], tf[j], f"{what}: near {i} against far {j}")
    ts = max(tn.max(), EPS)
    tb = min(tf.min(), t_max)
    return bool(ts <= tb), ts


def _triangle(p, o, d, t_max, what):
    """Moeller-Trumbore in binary64: t of a hit in (EPS, t_max) or None; barycentrics and t clear of their bounds by MARGIN"""
    e1, e2 = p[1] - p[0], p[2] - p[0]
    h = np.cross(d, e2)
    det = e1 @ h
    scale = np.linalg.norm(e1) * np.linalg.norm(e2) * np.linalg.norm(d)
    if det == 0.0 and not np.any((np.cross(e1, e2) != 0) & (d != 0)):
        return None                     # exactly parallel, and exactly so in binary32: every product of the determinant is a zero
    if abs(det) <= MARGIN * scale:
        raise MarginError(f"{what}: ray nearly in the triangle's plane")
    s = o - p[0]
    u = (s @ h) / det
    q = np.cross(s, e1)
    v = (d @ q) / det
    t = (e2 @ q) / det
    for name, val in (("u", u), ("v", v), ("1-u-v", 1.0 - u - v)):
        if abs(val) <= MARGIN:
            raise MarginError(f"{what}: barycentric {name} = {val!r}")
    _clear(t, EPS, f"{what}: t against epsilon")
    _clear(t, t_max, f"{what}: t against t_max")
    return t if (u > 0 and v > 0 and u + v < 1 and EPS < t < t_max) else None


class WalkResult:
    def __init__(self):
        self.max_held, self.written, self.read, self.hit = 0, set(), set(), None


def walk(tr, which, ray, discipline):
    """one ray (o[3], d[3], t_max) through TLAS `which` of Trees `tr` under a push discipline.  Returns the largest number of entries held, the
    set of levels written and read (level = index of the entry, as Stack8 counts it) and the answer (closest: t or None; any: bool).

    closest     pop; an entry whose t_enter > t_max is dropped (the popped-entry cull after a hit); an instance sets the object ray and stands
                for its BLAS root, NOT box-tested; up to 4 levels per step: both children met -> the farther is pushed (ties: left is), the
                nearer is followed if it is a triangle leaf or a branch before the 4th level, else pushed; a followed leaf is tested at once
    any         pop, no cull; an instance's BLAS root box IS tested; up to 4 levels: both met -> left pushed, right followed; one met -> it is
                followed; the followed child is pushed when it is an instance or a branch at the 4th level; the first triangle met ends the walk
    inline_any  any, with 6 levels per step
    fused_any   the fused NEE launch's any-phase: pop; instance -> root box test; a branch pushes its met children, left then right"""
    o, d, t_max = np.asarray(ray[0], np.float64), np.asarray(ray[1], np.float64), float(ray[2])
    levels = BRANCH_LEVELS[discipline]
    closest = discipline == "closest"
    tl = tr.tlas[which]
    res = WalkResult()
    stack = []

    def push(e):
        res.written.add(len(stack))
        stack.append(e)
        res.max_held = max(res.max_held, len(stack))

    def pop():
        res.read.add(len(stack) - 1)
        return stack.pop()

    if tl["kind"].size == 0 or np.isnan(t_max):
        return res
    hit, te = _slab(tl["boxes"][tl["root"]], o, d, t_max, "TLAS root")
    if not hit:
        return res
    push((None, int(tl["root"]), 0.0 if closest else te))
    oo, od, model = o, d, None       # the ray in the space of the tree being walked; model None: the TLAS
    blas_base = -1
    best = None
    while stack:
        if model is not None and len(stack) == blas_base:
            model, oo, od = None, o, d
        tree, node, t_enter = pop()
        if closest:
            if t_enter not in (0.0, EPS):
                _clear(t_enter, t_max, "popped-entry cull")
            if t_enter > t_max:
                continue
        cur = tl if tree is None else tr.blas[tree]
        if tree is None and cur["kind"][node] != 0:
            inst = int(cur["a"][node])
            model = tr.model_of[which][int(cur["b"][node])]
            m = tr.inv[which][inst]
            oo, od = m[:, :3] @ o + m[:, 3], m[:, :3] @ d
            blas_base = len(stack)
            cur = tr.blas[model]
            node = int(cur["root"])
            if closest:
                t_enter = 0.0
            else:
                hit, t_enter = _slab(cur["boxes"][node], oo, od, t_max, f"BLAS {model} root")
                if not hit:
                    continue
        tree = model
        lvl = 0
        while node is not None and cur["kind"][node] == 0 and lvl < levels:
            l, r = int(cur["a"][node]), int(cur["b"][node])
            hl, tl_ = _slab(cur["boxes"][l], oo, od, t_max, f"node {l}")
            hr, tr_ = _slab(cur["boxes"][r], oo, od, t_max, f"node {r}")
            nxt = None
            if discipline == "fused_any":
                if hl:
                    push((tree, l, tl_))
                if hr:
                    push((tree, r, tr_))
            elif closest:
                # (an axis-parallel ray that meets two boxes at the SAME plane coordinate computes one number twice, in either precision: a tie, left underneath)
                if hl and hr and not (tl_ == tr_ and np.count_nonzero(od) == 1):
                    _clear(tl_, tr_, f"nearer child of node {node}")
                left_near = tl_ < tr_
                if hl and hr:
                    push((tree, r, tr_) if left_near else (tree, l, tl_))
                if hl or hr:
                    nxt = (l, tl_) if (hl and (left_near or not hr)) else (r, tr_)
            else:
                if hl and hr:
                    push((tree, l, tl_))
                if hl or hr:
                    nxt = (r, tr_) if hr else (l, tl_)
            node = None
            if nxt is not None:
                is_leaf = cur["kind"][nxt[0]] != 0
                if (is_leaf and tree is not None) or (not is_leaf and lvl + 1 < levels):
                    node, t_enter = nxt
                else:
                    push((tree, nxt[0], nxt[1]))
            lvl += 1
        if node is not None and cur["kind"][node] != 0:
            assert tree is not None
            first, count = int(cur["a"][node]), int(cur["b"][node])
            for k in range(count):
                prim = int(cur["prim_ids"][first + k])
                t = _triangle(tr.tris[tree][prim], oo, od, t_max, f"model {tree} triangle {prim}")
                if t is not None:
                    if not closest:
                        res.hit = True
                        return res
                    best = t_max = t
    res.hit = best if closest else False
    return res


def reachable(tr, which, discipline):
    """the largest occupancy ANY ray could cause in TLAS `which` if every box it tests were met and no triangle ever cut the walk short: the
    discipline applied to the tree's shape alone (closest: the worse of the two orders at every branch)"""
    levels = BRANCH_LEVELS[discipline]
    tl = tr.tlas[which]
    memo = {}

    def expand(tree, node, lvl):
        """extra entries (beyond those held) the walk can reach from the moment `node` is followed at step level lvl"""
        key = (tree, node, lvl)
        if key in memo:
            return memo[key]
        cur = tl if tree is None else tr.blas[tree]
        if cur["kind"][node] != 0:
            if tree is not None:
                out = 0
            else:
                model = tr.model_of[which][int(cur["b"][node])]
                out = expand(model, int(tr.blas[model]["root"]), 0)
        else:
            l, r = int(cur["a"][node]), int(cur["b"][node])
            if discipline == "fused_any":
                out = max(2, 1 + expand(tree, r, 0), expand(tree, l, 0))
            else:
                out = 0
                for near, far in ((r, l),) if discipline != "closest" else ((l, r), (r, l)):
                    is_leaf = cur["kind"][near] != 0
                    if (is_leaf and tree is not None) or (not is_leaf and lvl + 1 < levels):
                        m = 1 + expand(tree, near, lvl + 1)
                    else:
                        m = max(2, 1 + expand(tree, near, 0))
                    out = max(out, m, expand(tree, far, 0))
        memo[key] = out
        return out

    if tl["kind"].size == 0:
        return 0
    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        return max(1, expand(None, int(tl["root"]), 0))
    finally:
        sys.setrecursionlimit(old)


# ------------------------------------------------------------------------------------------------------------------------ rays
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def axis_rays(axis, up, side_v, scale, top, gaps, grow, far_off=None):
    """The designed rays of a chain of plates (_plate) perpendicular to `axis` (y along `up`, z along `side_v`) whose first plate is `scale` from the
    origin; `grow`: the plates' size is 0.4 of their distance, else 0.4 * scale.  From the dense end (half a `scale` before the origin):
      * through the triangles (every leaf a hit candidate): along the axis at y = z = -0.1 scale, which is inside the first plate and the centre of a giant one;
      * through the empty part of the boxes (every box met, nothing hit): along the axis at y = z = 0.3 scale where the plates do not grow (a GIANT plate
        is still hit at its centre) and, where they grow, ALSO on the cone y = 0.3 x, z = 0.2 x through the origin, outside every triangle and inside every box;
      * each exactly so and tilted by 1e-3;
      * each with t_max before the first plate, between two plates, beyond the small plates, beyond everything (`gaps`) and +inf.
    Back from the far end (1.5 * top along the axis, `top`: the last plate's place): along the axis at y = z = -0.1 scale (the last plate is hit), and past
    the triangles: a ray from so far away cannot tell the small end's boxes apart by 1e-3 of their distance, so this one stays clear of them: along the
    axis at y = z = far_off (inside the large plates' boxes only), or, where no plate is large, aimed at the last plate's corner on a slope of 2e-3
    that carries it out of the cross-section before the next box.  Returns o, d, t_max as binary32 arrays."""
    far = 1.5 * top
    axis, up, side_v = (np.asarray(v, np.float64) for v in (axis, up, side_v))
    O, D, T = [], [], []
    for empty in (False, True, "cone")[:3 if grow else 2]:
        for tilt in (0.0, 1e-3):
            if empty == "cone":
                d0 = axis + 0.3 * up + 0.2 * side_v
                o = -0.5 * scale * d0
            else:
                d0 = axis
                o = -0.5 * scale * axis + (up + side_v) * (0.3 if empty else -0.1) * scale
            d = _unit(d0 + tilt * (up - 0.5 * side_v))
            for t in list(gaps) + [np.inf]:
                O.append(o); D.append(d); T.append(t)
        d = -axis
        if not empty:
            o = far * axis + (up + side_v) * -0.1 * scale
        elif far_off is not None:
            o = far * axis + (up + side_v) * far_off
        else:
            d = _unit(-axis + 2e-3 * up)
            o = far * axis + (up + side_v) * 0.3 * scale - 2e-3 * (far - top) * up
        O.append(o); D.append(d); T.append(np.inf)
        O.append(o); D.append(d); T.append(far * 0.25)
    return np.asarray(O, F32), np.asarray(D, F32), np.asarray(T, F32)


def random_rays(seed, centre, radius, n=256):
    """seeded rays for the device comparison only (never simulated): origins about the chain's dense end, a tenth of them axis-parallel"""
    rng = np.random.default_rng(seed)
    O = (np.asarray(centre) + rng.normal(size=(n, 3)) * radius).astype(F32)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F32)
    k = n // 10
    D[:k] = np.eye(3, dtype=F32)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1)).astype(F32)
    O[k:2 * k] = (np.asarray(centre) + rng.normal(size=(k, 3)) * radius * 1e-2).astype(F32)
    T = np.where(rng.random(n) < 0.3, np.inf, np.exp(rng.uniform(np.log(radius * 1e-2), np.log(radius * 1e4), n))).astype(F32)
    return O, D, T


X, Y, Z = np.eye(3)

SCENES = {
    "blas_chain_left": lambda: blas_chain("left"), "blas_chain_mirrored": lambda: blas_chain("mirrored"), "blas_chain_right": lambda: blas_chain("right"),
    "tlas_chain": lambda: tlas_chain("left"), "tlas_chain_mirrored": lambda: tlas_chain("right"), "ident_chain": lambda: ident_chain("left"),
    "both_chains": both_chains, "both_chains_ballast": lambda: both_chains(BALLAST), "lights_chain": lights_chain, "forked": forked,
}


def designed(name):
    """(o, d, t_max) of scene `name`'s designed rays (SCENES[name], or deep_chain_<n>)"""
    if name == "blas_chain_right":
        return axis_rays(X, Y, Z, 1.0, GIANT, [0.25, 2.0, 1.5 * 2.0 ** 20, 4.0 * GIANT], True, 0.3 * 2.0 ** 57)
    if name in ("blas_chain_left", "blas_chain_mirrored", "forked") or name.startswith("inline_limit_"):
        plates = FORKED_PLATES if name == "forked" else 2 * int(name.rsplit("_", 1)[1]) - 8 if name.startswith("inline_limit_") else 64
        s, top = SAH_SCALE, 2.0 ** (plates - 1)
        sign = 1.0 if name in ("blas_chain_left", "forked") else -1.0
        return axis_rays(sign * X, Y, Z, s, s * top, [0.25 * s, 2.0 * s, 1.5 * s * 2.0 ** 20, s * 4.0 * top], True, 0.3 * s * top / 64.0)
    if name.startswith("deep_chain_"):
        n = int(name.rsplit("_", 1)[1])
        return axis_rays(X, Y, Z, 1.0, GIANT, [0.25, 2.0, n + 0.25, 4.0 * GIANT], False, 0.3 * 2.0 ** 57)
    if name in ("tlas_chain", "tlas_chain_mirrored", "ident_chain", "lights_chain"):
        sign = -1.0 if name.endswith("mirrored") else 1.0
        top = 2.0 ** (LAMPS - 1 if name == "lights_chain" else 15)
        return axis_rays(sign * X, Y, Z, 1.0, top, [0.25, 2.0, 150.0, 16.0 * top], False)
    if name in ("both_chains", "both_chains_ballast"):
        R = both_rotation()[:, :3].astype(np.float64)
        s = BOTH_SCALE
        top = s * 2.0 ** (BOTH_PLATES - 1)              # (back from the deep instance's own far end, short of the first placement)
        return axis_rays(R @ X, R @ Y, R @ Z, s, top, [0.25 * s, 2.0 * s, 1.5 * s * 2.0 ** 12, 8.0 * BOTH_SPACING * BOTH_RATIO ** BOTH_INSTANCES], True,
                         0.3 * s * 2.0 ** (BOTH_PLATES - 7))
    raise KeyError(name)


def scene(name):
    if name.startswith("deep_chain_"):
        return deep_chain(int(name.rsplit("_", 1)[1]))
    if name.startswith("inline_limit_"):
        return inline_limit(int(name.rsplit("_", 1)[1]))
    return SCENES[name]()


def random_for(name):
    """the 256 seeded rays of a scene: about its dense end, at the size of its smallest plates"""
    radius = 4.0 * SAH_SCALE if name in ("both_chains", "blas_chain_left", "blas_chain_mirrored", "forked") or name.startswith("inline_limit_") else 4.0
    return random_rays(sum(map(ord, name)), np.zeros(3), radius)
