"""pt_set_config on a live context: the configuration walk, a numpy model of the row table and of what every step must drop, and
products(): every product of the library for one configuration as named arrays.  tests/test_reconfig_host.py holds the host side of the
contract (include/pt_api.h at pt_set_config) to these; tests/test_gpu_reconfig.py leads one context through the walk and holds every product
to a context created with the step's configuration, and the render to the oracle.  Nothing at module level calls the library or the device."""
import numpy as np

from variant_census_common import FLAG_ADAPTIVE, FLAG_GENERAL_WALK, FLAG_NO_LDS_SCENE, SPILL_LEVELS, room

F = np.float32
FLAG_NO_PRIMARY_CULL = 8       # include/pt_api.h
ERR_ARG, ERR_STATE = -1, -3
M = 3                          # samples every product is sized for
UNLIT = (0.25, 0.5, 0.125)
SEED0, SEED1 = 0x5EED5EED, 0xC0FFEE1234

# pt_config as Renderer's keywords (device left out: it never changes); the walk starts here
BASE = dict(width=32, height=24, max_bounces=3, n_sobol=512, enable_nee=1, seed=SEED0, rank=0, world_size=1, strip_rows=4, batch_spp=0,
            flags=0, stack_lds_levels=0, queue_slack=0, pipelines=0)

# (kind, what pt_set_config is given on top of the configuration in force).  Every kind occurs right after a step of another kind.
WALK = [
    ("start", {}),
    ("shape", dict(width=24, height=32)),                                   # the same pixel count, other pixels
    ("bounces", dict(max_bounces=1)),
    ("size", dict(width=40, height=24)),                                    # grow
    ("flag", dict(flags=FLAG_NO_LDS_SCENE)),
    ("size", dict(width=16, height=12)),                                    # shrink
    ("flag", dict(flags=0)),
    ("shard", dict(width=32, height=16, world_size=2, rank=0, strip_rows=4)),
    ("seed", dict(seed=SEED1)),
    ("rank", dict(rank=1)),                                                 # the same row count, the other rows
    ("nee", dict(enable_nee=0)),
    ("strip", dict(strip_rows=2)),                                          # the same row count again
    ("nee", dict(enable_nee=1)),
    ("shard", dict(world_size=1, rank=0)),                                  # back to one rank
    ("sobol", dict(n_sobol=64)),
    ("batch", dict(batch_spp=1, pipelines=1)),
    ("spill", dict(stack_lds_levels=SPILL_LEVELS)),
    ("batch", dict(pipelines=3)),
    ("spill", dict(stack_lds_levels=0)),
    ("batch", dict(pipelines=2)),
    ("bounces", dict(max_bounces=6)),
    ("flag", dict(flags=FLAG_GENERAL_WALK)),
    ("size", dict(width=32, height=24, strip_rows=0)),                      # (strip_rows 0: the library's default, 4)
    ("flag", dict(flags=0)),
    ("flag", dict(flags=FLAG_ADAPTIVE)),
    ("bounces", dict(max_bounces=3)),
    ("flag", dict(flags=0)),
    ("flag", dict(flags=FLAG_NO_PRIMARY_CULL)),
    ("batch", dict(batch_spp=0, pipelines=0)),
    ("flag", dict(flags=0)),
]


def configs():
    """the configuration in force after every step of the walk"""
    out, cur = [], dict(BASE)
    for _, change in WALK:
        cur = dict(cur, **change)
        out.append(cur)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the row table
def model_rows(cfg):
    """the local rows of a configuration, the library's defaults applied (world_size 0 -> 1, strip_rows 0 -> 4)"""
    world, strip = cfg["world_size"] or 1, cfg["strip_rows"] or 4
    return [y for y in range(cfg["height"]) if (y // strip) % world == cfg["rank"]]


def pixel_set(cfg):
    return cfg["width"], tuple(model_rows(cfg))


def drops():
    """for every step but the first: does it change the set of local pixels (and so drop the frame state)?"""
    c = configs()
    return [pixel_set(a) != pixel_set(b) for a, b in zip(c, c[1:])]


def same_count_steps():
    """{kind: step index} of the steps that change the set of local pixels and keep its size"""
    c = configs()
    out = {}
    for i, (a, b) in enumerate(zip(c, c[1:]), 1):
        if pixel_set(a) != pixel_set(b) and a["width"] * len(model_rows(a)) == b["width"] * len(model_rows(b)):
            out[WALK[i][0]] = i
    return out


# -------------------------------------------------------------------------------------------------------------------------- the scene
def scene():
    """the census's corner room: Lambertian walls, an emissive panel in view, a mirror box, smooth glass, GGX metal, GGX glass with a volume;
    the block has a translated second instance and the slab a general rigid turn"""
    return room("corner")[1]


def renderer(api, cfg, **kw):
    return api.Renderer(scene(), **dict(cfg, **kw))


def ray_set(n=256, seed=17):
    """n rays from about the room's middle in every direction, a stream key and a sample each"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.sqrt((d * d).sum(1))[:, None]).astype(F)
    tmax = rng.uniform(0.0, 25.0, n).astype(F)
    return o, d, np.arange(n, dtype=np.uint32) * np.uint32(7), (np.arange(n) % M).astype(np.uint32), tmax


PROBES = np.array([[0.0, 0.0, 0.0], [-7.0, 3.0, 2.0], [4.5, -8.0, -1.0], [8.0, 8.0, 8.0]], F)
HOST_KEYS = ((0, 0), (5, 1), (767, 2), (100, 70))       # (stream key, sample) of the host evaluations; sample 70 lies beyond n_sobol = 64


def host_products(r, cfg):
    """what the host evaluates from width, height, seed and n_sobol (no device)"""
    out = {}
    w, h = cfg["width"], cfg["height"]
    for pixel, sample in ((0, 0), (w - 1, 1), (w * (h // 2) + w // 3, 2), (w * h - 1, 70)):
        o, d, n = r.primary_ray(pixel, sample)
        out[f"primary_ray {pixel} {sample}"] = np.concatenate([o, d, [F(n)]])
    for key, sample in HOST_KEYS:
        d, y = r.probe_ray(key, sample)
        out[f"probe_ray {key} {sample}"] = np.concatenate([d, y])
        out[f"lightmap_ray {key} {sample}"] = r.lightmap_ray(key, sample, (0.0, 0.6, 0.8))
    return out


def _refused(api, call, what):
    try:
        call()
    except api.PtError as e:
        assert e.code == ERR_STATE, (what, e.code, str(e))
        return
    raise AssertionError(f"{what}: accepted on a sharded context")


def products(api, r, cfg):
    """every product of renderer `r` under configuration `cfg` (the one in force), each a named array, in one fixed order of calls.  The
    caller of a context that has history clears it first (reset_accumulation, reset_temporal, reset_baked).  Returns (arrays, routes):
    routes holds, from pt_last_launches, the `bvh`, `spill` and lights-TLAS `ident` axis values the traversal launches took."""
    out, routes = {}, {"bvh": set(), "spill": set(), "lights_ident": set()}
    one_rank = (cfg["world_size"] or 1) == 1
    adaptive = bool(cfg["flags"] & FLAG_ADAPTIVE)
    r.reset_stats()

    def walk_axes(log):
        for launcher, _, axes in log:
            if launcher in ("closest", "any"):
                routes["bvh"].add(axes[1]); routes["spill"].add(axes[2])
            elif launcher == "fused":
                routes["bvh"].add(axes[0]); routes["spill"].add(axes[1])

    def tallies(name):
        st = r.stats()
        out[name] = np.array([st.rays_closest, st.rays_any, st.rays_light_closest, st.paths], np.uint64)

    # ---- the path tracer
    out["render_samples"] = r.render_samples(0, M)
    r.reset_accumulation()
    r.reset_stats()
    out["accumulation"], out["position"], out["id"] = r.render(0, M)
    walk_axes(r.last_launches())
    tallies("tallies of the render")
    if adaptive:
        out["moments"] = r.read_moments()
        out["adaptive mask"] = r.adaptive_mask(0.05, 0.0, 2, 0)
        out["adaptive n"] = np.array([r.render_adaptive(M, 0.05, 0.0, 2, 0)], np.uint32)
        walk_axes(r.last_launches())
        out["adaptive accumulation"], out["adaptive position"], out["adaptive id"] = r.read_frame()
        out["adaptive moments"] = r.read_moments()
    # ---- guides, mean albedo, the filters
    r.render_guides(0)
    walk_axes(r.last_launches(api.LAUNCHES_HOOK))
    out["guide position"], out["guide normal"], out["guide model"] = r.read_guides()
    out["guide instances"], out["guide albedo"] = r.read_guide_instances(), r.read_guide_albedo()
    r.accumulate_albedo(0, M)
    out["albedo"] = r.read_albedo()
    if one_rank:
        out["denoise"] = r.denoise(iterations=3)
        out["denoise_albedo"] = r.denoise_albedo(api.ALBEDO_MEAN, iterations=3)
    else:
        _refused(api, lambda: r.denoise(iterations=3), "pt_denoise")
        _refused(api, lambda: r.denoise_albedo(api.ALBEDO_MEAN, iterations=3), "pt_denoise_albedo")
    r.render_guides(1, follow=2)
    out["followed position"], out["followed normal"], out["followed model"] = r.read_guides()
    out["followed hops"] = r.read_guide_hops()
    # ---- State::update and the temporal stage: the second call of each after the camera turned, so the reprojection branch runs
    if one_rank:
        last = r.inv_projection()
        d0, p0, i0 = r.frame(0, last)
        r.camera_input(api.EV_MOUSE_MOTION, 1.0, 0.25, 1.0e-6)
        d1, p1, i1 = r.frame(1, last, ident=i0.copy())
        assert not np.array_equal(r.inv_projection(), last)
        out["frame 0"], out["frame 1"], out["frame 1 position"], out["frame 1 id"] = d0, d1, p1, i1
        out["frame accumulation"] = r.read_accumulation()
        last = r.inv_projection()
        t0 = r.frame_temporal(2, last, iterations=2)
        r.camera_input(api.EV_MOUSE_MOTION, -0.5, 0.5, 1.0e-6)
        t1 = r.frame_temporal(3, last, ident=t0[2].copy(), iterations=2)
        out["temporal 0"], out["temporal 1"], out["temporal 1 data"], out["temporal 1 id"] = t0[3], t1[3], t1[0], t1[2]
        out["temporal history"], out["temporal moments"], out["temporal variance"] = r.read_temporal()
        r.set_camera(scene().camera)                               # the camera of every other product again
    else:
        _refused(api, lambda: r.frame(0, r.inv_projection()), "pt_frame")
        _refused(api, lambda: r.frame_temporal(2, r.inv_projection(), iterations=2), "pt_frame_temporal")
    # ---- the baked view (no map is set: every surface shows `unlit` times its colour)
    out["baked"] = r.render_baked(0, M, follow=2, unlit=UNLIT)
    # ---- caller-supplied rays, the hooks, probes
    o, d, key, sample, tmax = ray_set()
    out["rays radiance"], out["rays position"], out["rays id"] = r.integrate_rays(o, d, key, sample)
    walk_axes(r.last_launches())
    for which in (0, 1):
        g = r.trace_closest(o, d, which=which)
        log = r.last_launches(api.LAUNCHES_HOOK)
        walk_axes(log)
        if which == 1:
            routes["lights_ident"] |= {axes[3] for launcher, _, axes in log if launcher == "closest"}
        for k in ("inst", "prim", "t", "u", "v"):
            out[f"closest {which} {k}"] = g[k]
        out[f"any {which}"] = r.trace_any(o, d, tmax, which=which)
        walk_axes(r.last_launches(api.LAUNCHES_HOOK))
    out["probes"] = r.bake_probes(PROBES, M)
    out.update(host_products(r, cfg))
    tallies("tallies of everything")
    return out, routes
