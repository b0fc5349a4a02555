"""Surface materials at their edges: shared by test_materials_host.py (CPU) and test_gpu_materials.py (GPU).

Three things live here:
  * the WyRand stream restated in numpy uint64 (stream_state0 / wyrand_u32 / stream_f32), so that edge uniforms can be searched for and
    fed to the binary64 statement for thousands of rows at once;
  * material_reference_f64 / bsdf_reference_f64: a binary64 statement of the reference's surface materials, written from material.rs,
    utility.rs and material/onb.rs, and the checkers check_material_eval / check_bsdf_eval built on it;
  * the edge inputs both suites evaluate (edge_inputs, bsdf_inputs) and the designed scenes and rays of the shading-kernel tests.
"""
import os

import numpy as np

F = np.float32
U64 = np.uint64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDGE_KEYS = os.path.join(GOLDEN, "material_edge_keys.npz")
DRAWS_CONSUMED = 1                      # the probes draw where a camera path does: after the jitter's one draw
EPS = 2.0 ** -24                        # half an ulp of a binary32 number in [1, 2): the unit every tolerance below is stated in


# ------------------------------------------------------------------------------------------------------------------ the stream
_M32 = U64(0xFFFFFFFF)


def _mul128(a, b):
    """high and low 64 bits of the 128-bit product of two uint64 arrays (four 32-bit limbs)"""
    a0, a1, b0, b1 = a & _M32, a >> U64(32), b & _M32, b >> U64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> U64(32)) + (p01 & _M32) + (p10 & _M32)
    lo = (p00 & _M32) | (mid << U64(32))
    hi = p11 + (p01 >> U64(32)) + (p10 >> U64(32)) + (mid >> U64(32))
    return hi, lo


def stream_state0(seed, pixel, sample):
    """the stream key of (pixel, sample): splitmix64's finaliser over seed + golden * (sample << 32 | pixel)"""
    with np.errstate(over="ignore"):
        z = U64(seed) + U64(0x9E3779B97F4A7C15) * ((np.asarray(sample, U64) << U64(32)) | np.asarray(pixel, U64))
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def wyrand_u64(s0, k):
    """draw k (zero-based) of the WyRand stream whose state before its first draw is s0"""
    with np.errstate(over="ignore"):
        s = np.asarray(s0, U64) + U64(k + 1) * U64(0xA0761D6478BD642F)
        hi, lo = _mul128(s, s ^ U64(0xE7037ED1A0B428DB))
    return hi ^ lo


def wyrand_u32(s0, k):
    return (wyrand_u64(s0, k) & _M32).astype(np.uint32)


def u32_to_f32(u):
    """generate::<f32>(): (u32 as f32) / 2^32, in [0, 1] with both ends attained"""
    return (np.asarray(u, np.uint32).astype(F) / F(4294967296.0)).astype(F)


def stream_f32(seed, pixel, sample, first, count):
    """[n, count] binary32 uniforms: draws first .. first + count - 1 of each (pixel, sample) stream"""
    s0 = stream_state0(seed, pixel, sample)
    return np.stack([u32_to_f32(wyrand_u32(s0, first + j)) for j in range(count)], 1)


# ------------------------------------------------------------------------------------------- the binary64 statement
LAMBERTIAN, EMISSIVE, SPECULAR, GGX_METAL, GGX_DIELECTRIC, DIELECTRIC = range(6)


class Constants:
    """what a material holds in binary32 (material.rs:290-312: a = roughness^2 clamped to [1e-4, 0.9999]), widened to binary64"""

    def __init__(self, m):
        self.kind = m.kind
        self.colour = np.array([F(c) for c in m.colour], np.float64)
        self.alpha = float(np.clip(F(m.roughness) * F(m.roughness), F(0.0001), F(0.9999)))
        self.ior = float(F(m.ior))
        self.inv_ior = float(F(1.0) / F(m.ior))                       # ior.recip() is one binary32 division of a constant

    def eta_scatter(self, front):                                     # material.rs:328, 498
        return np.where(front, self.inv_ior, self.ior)

    def eta_eval(self, front):                                        # material.rs:368, 390, 409: the other way round
        return np.where(front, self.ior, self.inv_ior)


class _Decide:
    """Every comparison the reference branches on goes through here.  near[name] marks the rows whose two sides lie within `err` (the
    binary32 rounding of the compared quantity) of each other; a name listed in `flip` takes the other branch on exactly those rows."""

    def __init__(self, flip=()):
        self.flip = frozenset(flip)
        self.near = {}

    def __call__(self, name, lhs, op, rhs, err):
        with np.errstate(invalid="ignore"):
            nat = {">": np.greater, "<": np.less, "<=": np.less_equal}[op](lhs, rhs)
            near = np.abs(lhs - rhs) <= err
        self.near[name] = self.near.get(name, False) | near
        return np.where(near, ~nat, nat) if name in self.flip else nat


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _onb(n):
    """glam's Vec3A::any_orthonormal_pair (onb.rs:5): the two columns beside the normal"""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    s = np.where(np.signbit(z), -1.0, 1.0)
    a = -1.0 / (s + z)
    b = x * y * a
    return np.stack([1.0 + s * x * x * a, s * b, -s * x], 1), np.stack([b, s + y * y * a, -y], 1)


def _local(c0, c1, n, v):
    return np.stack([_dot(c0, v), _dot(c1, v), _dot(n, v)], 1)


def _world(c0, c1, n, l):
    return c0 * l[:, 0:1] + c1 * l[:, 1:2] + n * l[:, 2:3]


def _reflect(i, n):                                                   # utility.rs:21
    return i - 2.0 * _dot(n, i)[:, None] * n


def _sqrt_spread(q, dq):
    """how far sqrt moves when its argument moves by dq: the conditioning of every sqrt(1 - x^2) below"""
    return np.sqrt(q + dq) - np.sqrt(np.maximum(q - dq, 0.0))


def _refract(i, n, eta, dec, d_ndi):
    """utility.rs:23-36.  Returns the direction (NaN where k <= 0) and its tolerance; d_ndi is the rounding of dot(n, i)"""
    ndi = _dot(n, i)
    k = 1.0 - eta * eta * (1.0 - ndi * ndi)
    dk = eta * eta * (2.0 * np.abs(ndi) * d_ndi + 8 * EPS)
    nan = dec("k<=0", k, "<=", 0.0, dk)
    with np.errstate(invalid="ignore"):
        r = eta[:, None] * i - (eta * ndi + np.sqrt(np.maximum(k, 0.0)))[:, None] * n     # a row flipped onto this side has k within dk of 0
    r = np.where(nan[:, None], np.nan, r)
    return r, 8 * EPS + (1.0 + eta) * d_ndi + _sqrt_spread(np.maximum(k, 0.0), dk)


def _dielectric_f(cosine, eta, dec, d_cos):
    """Dielectric::f, material.rs:477-489; returns f and its absolute rounding"""
    tir = dec("tir", eta * eta * (1.0 - cosine * cosine), ">", 1.0, eta * eta * (2.0 * np.abs(cosine) * d_cos + 8 * EPS))
    f0 = ((eta - 1.0) / (eta + 1.0)) ** 2
    f = np.where(tir, 1.0, (1.0 - cosine) ** 5 * (1.0 - f0) + f0)
    return f, np.where(tir, 0.0, 5.0 * (1.0 - cosine) ** 4 * d_cos + 8 * EPS * np.abs(f))


def _half_vector(c, incoming, normal, u1, u2, dec):
    """GGX::generate_half_vector, material.rs:248-284, with generate_onb_ggx (onb.rs:9-27).  Returns h in world space and its tolerance:
    24 eps for the polar map, the rounding of v_ over the stretched length (grazing incidence at a small alpha), r times the rounding of phi, the spread of sqrt(1 - p1^2 - p2^2) (its argument is at least 1 - 0.9999^2), and the azimuth of the frame
    around v, which is only as good as v's tangential part (4 eps / |v_.xy|); all of it divided by the length the un-stretch normalises."""
    a = c.alpha
    c0, c1 = _onb(normal)
    v_ = _local(c0, c1, normal, -incoming)
    vs = v_ * np.array([a, a, 1.0])
    stretch = 4 * EPS / np.sqrt(_dot(vs, vs))                                # v_'s rounding, magnified where the stretched vector is short
    v = _unit(vs)
    up = dec("onb_ggx", v[:, 2], ">", float(F(0.99999)), 4 * EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        t1 = _unit(np.stack([v[:, 1], -v[:, 0], np.zeros(len(v))], 1))          # v x Z
    t2 = np.cross(t1, v)
    t1 = np.where(up[:, None], [1.0, 0.0, 0.0], t1)
    t2 = np.where(up[:, None], [0.0, -1.0, 0.0], t2)
    vb = np.where(up[:, None], [0.0, 0.0, 1.0], v)
    a_ = 1.0 / (1.0 + v[:, 2])
    cond = dec("u2<a_", u2, "<", a_, 4 * EPS)
    r = np.minimum(np.sqrt(u1), float(F(0.9999)))
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = np.where(cond, np.pi * u2 / a_, np.pi + ((u2 - a_) / (1.0 - a_)) * np.pi)
        # the second half-disk divides two differences of nearly equal numbers at grazing incidence (a_ -> 1)
        dphi = np.where(cond, 8 * EPS * np.pi, np.pi * 4 * EPS * (1.0 + (u2 - a_) / (1.0 - a_)) / (1.0 - a_) + 8 * EPS * np.pi)
    p1 = r * np.cos(phi)
    p2 = r * np.sin(phi) * np.where(cond, 1.0, v[:, 2])
    q = 1.0 - p1 * p1 - p2 * p2
    h_ = t1 * p1[:, None] + t2 * p2[:, None] + vb * np.sqrt(q)[:, None]
    hs = h_ * np.array([a, a, 1.0])
    length = np.sqrt(_dot(hs, hs))
    with np.errstate(divide="ignore"):
        frame = np.where(up, 0.0, 4 * EPS / np.sqrt(v_[:, 0] ** 2 + v_[:, 1] ** 2))
    tol = 8 * EPS + (24 * EPS + r * dphi + _sqrt_spread(q, 6 * EPS) + frame + stretch) / length
    return _world(c0, c1, normal, hs / length[:, None]), tol


def material_reference_f64(c, incoming, normal, front, u, flip=()):
    """MaterialTrait::scatter_direction of Lambertian (material.rs:104-107 with utility.rs:7-19), Specular (:153), GGX reflective and
    transmissive (:317-347) and Dielectric (:496-509) in binary64, as the reference writes them, fed binary32 constants, directions
    and uniforms u[:, 0:3] (a row uses as many as its material draws).

    Returns direction [n, 3] (NaN where the reference returns NaN), its absolute tolerance [n], draws [n], reflected [n] (meaningful for
    the two dielectrics) and the _Decide holding which rows sit on a threshold.

    What is stated is the reference, not the textbook: GGX::d's `tan_sq` is sqrt(1 - cos^2) / cos^2 (material.rs:197), and the pdf
    get_bsdf_pdf returns is the half-vector pdf although the sampler draws visible normals.  So the GGX lobes here neither integrate to
    one nor conserve energy, and no test built on this file asserts a physical law the reference itself breaks."""
    incoming, normal, u = np.asarray(incoming, np.float64), np.asarray(normal, np.float64), np.asarray(u, np.float64)
    front = np.asarray(front).astype(bool)
    n = len(incoming)
    dec = _Decide(flip)
    reflected = np.ones(n, bool)
    if c.kind == LAMBERTIAN:
        r = np.sqrt(u[:, 0])
        q = 1.0 - r * r
        phi = 2.0 * np.pi * u[:, 1]
        c0, c1 = _onb(normal)
        d = _world(c0, c1, normal, np.stack([np.cos(phi) * r, np.sin(phi) * r, np.sqrt(np.maximum(q, 0.0))], 1))
        return d, 24 * EPS + _sqrt_spread(np.maximum(q, 0.0), 4 * EPS), np.full(n, 2), reflected, dec
    if c.kind == SPECULAR:
        return _reflect(incoming, normal), np.full(n, 12 * EPS), np.zeros(n, int), reflected, dec
    if c.kind == DIELECTRIC:
        eta = c.eta_scatter(front)
        f, df = _dielectric_f(-_dot(incoming, normal), eta, dec, 4 * EPS)
        reflected = dec("u<F", u[:, 0], "<", f, df + 2 * EPS)
        refr, tol = _refract(incoming, normal, eta, dec, 4 * EPS)
        return np.where(reflected[:, None], _reflect(incoming, normal), refr), np.where(reflected, 12 * EPS, tol), np.ones(n, int), reflected, dec
    h, th = _half_vector(c, incoming, normal, u[:, 0], u[:, 1], dec)
    refl = _reflect(incoming, h)
    if c.kind == GGX_METAL:
        return refl, 12 * EPS + 4.0 * th, np.full(n, 2), reflected, dec
    eta = c.eta_scatter(front)
    f0 = ((eta - 1.0) / (eta + 1.0)) ** 2
    cosine = -_dot(incoming, h)
    f = (1.0 - cosine) ** 5 * (1.0 - f0) + f0
    refr, tol = _refract(incoming, h, eta, dec, 4 * EPS + th)
    tir = np.isnan(refr).any(1)
    reflected = tir | dec("u<F", u[:, 2], "<", f, 5.0 * (1.0 - cosine) ** 4 * (4 * EPS + th) + 8 * EPS * f)
    return np.where(reflected[:, None], refl, refr), np.where(reflected, 12 * EPS + 4.0 * th, tol + 2.0 * th), np.where(tir, 2, 3), reflected, dec


def bsdf_reference_f64(c, incoming, outgoing, normal, front, flip=()):
    """MaterialTrait::get_bsdf_pdf(-incoming, outgoing, hit) in binary64 (material.rs:109-115, :155, :349-450, :511-527): `incoming` is
    the direction the ray travels in, as the probes take it.  Returns bsdf [n, 3], pdf [n], rel_bsdf [n, 3], rel_pdf [n] (the relative
    rounding the binary32 evaluation may show, derived per row from the formula's conditioning, see check_bsdf_eval), abs_pdf [n],
    degenerate [n] (a denominator within rounding of zero) and the _Decide."""
    incoming, outgoing, normal = np.asarray(incoming, np.float64), np.asarray(outgoing, np.float64), np.asarray(normal, np.float64)
    front = np.asarray(front).astype(bool)
    n = len(incoming)
    dec = _Decide(flip)
    zero, one = np.zeros(n), np.ones(n)
    col = np.broadcast_to(c.colour, (n, 3))
    none = np.zeros(n, bool)
    if c.kind == LAMBERTIAN:
        cosine = _dot(outgoing, normal)
        return col / np.pi, cosine / np.pi, np.full((n, 3), 4 * EPS), np.full(n, 4 * EPS), np.full(n, 4 * EPS), none, dec
    if c.kind == SPECULAR:
        return col + 0.0, one, np.zeros((n, 3)), zero, zero, none, dec
    if c.kind == DIELECTRIC:
        eta = c.eta_scatter(front)
        f, df = _dielectric_f(_dot(incoming, outgoing), eta, dec, 4 * EPS)
        up = dec("dot>0", _dot(outgoing, normal), ">", 0.0, 4 * EPS)
        t = 1.0 - f
        with np.errstate(invalid="ignore", divide="ignore"):
            rel_f, rel_t = df / np.abs(f) + 4 * EPS, np.where(t == 0.0, 0.0, df / np.abs(t)) + 8 * EPS
        bsdf = np.where(up[:, None], f[:, None], col * (t / (eta * eta))[:, None])
        return bsdf, np.where(up, f, t), np.where(up, rel_f, rel_t)[:, None] + zero[:, None] * np.zeros(3), np.where(up, rel_f, rel_t), df, none, dec
    # ---- GGX, material.rs:349-450
    a = c.alpha
    transmissive = c.kind == GGX_DIELECTRIC
    c0, c1 = _onb(normal)
    wi = _local(c0, c1, normal, outgoing)
    wo = _local(c0, c1, normal, -incoming)
    e4 = 4 * EPS
    transmitted = dec("wi.z<0", wi[:, 2], "<", 0.0, e4)
    eta = c.eta_eval(front)
    s = np.where((transmitted & transmissive)[:, None], eta[:, None] * wi + wo, wi + wo)
    length = np.sqrt(_dot(s, s))
    with np.errstate(invalid="ignore", divide="ignore"):
        h = s / length[:, None]
        dh = 2 * e4 * (1.0 + eta) / length + 2 * EPS                               # rounding of each component of h
        if transmissive:
            neg = transmitted & dec("h_.z<0", h[:, 2], "<", 0.0, dh)               # _h * _h.z.signum(): -0.0 counts as negative
            neg = neg | (transmitted & (h[:, 2] == 0.0) & np.signbit(h[:, 2]))
            h = np.where(neg[:, None], -h, h)
        idh, odh = _dot(wi, h), _dot(wo, h)
        dd = dh + e4                                                               # rounding of a dot product with h
        # GGX::d: sqrt(1 - cos^2) / cos^2 under the name tan_sq, as written
        hz = h[:, 2]
        d_zero = dec("h.z<=0", hz, "<=", 0.0, dh)
        q = 1.0 - hz * hz
        dq = 2.0 * np.abs(hz) * dh + 2 * EPS

        def d_of(q):
            x = a * a * (1.0 - q) + np.sqrt(np.maximum(q, 0.0))                     # cos^2 * (a^2 + tan_sq), which stays finite at cos = 0
            return a * a / (np.pi * x * x)
        d = np.where(d_zero, 0.0, d_of(q))
        d_lo, d_hi = d_of(np.minimum(q + dq, 1.0)), d_of(np.maximum(q - dq, 0.0))
        rel_d = np.where(d_zero, 0.0, np.maximum(np.abs(d_hi / d - 1.0), np.abs(1.0 - d_lo / d))) * (1.0 + 1e-4) + 16 * EPS   # the interval's end is attained: q rounds to 0
        rel_z = e4 / np.abs(wi[:, 2]) + e4 / np.abs(wo[:, 2])                      # of wi.z * wo.z
        if not transmissive:
            f, rel_f, rel_1f = one, zero, zero
            g_zero = dec("wi.z<=0", wi[:, 2], "<=", 0.0, e4) | dec("wo.z<=0", wo[:, 2], "<=", 0.0, e4)
            y = 1.0 - a * a
            g = np.where(g_zero, 0.0, 2.0 * wi[:, 2] * wo[:, 2] / (wo[:, 2] * np.hypot(a, wi[:, 2] * np.sqrt(y)) + wi[:, 2] * np.hypot(a, wo[:, 2] * np.sqrt(y))))
            rel_g = 2.0 * rel_z + 16 * EPS
        else:
            f0 = ((eta - 1.0) / (eta + 1.0)) ** 2
            xa = np.abs(idh)
            f = (1.0 - xa) ** 5 * (1.0 - f0) + f0
            df = 5.0 * (1.0 - xa) ** 4 * dd + 8 * EPS * f
            rel_f, rel_1f = df / f, df / np.abs(1.0 - f) + 4 * EPS

            def g1(v, vdh, name):
                z = dec(name, v[:, 2] * vdh, "<=", 0.0, np.abs(v[:, 2]) * dd + np.abs(vdh) * e4 + 1e-45)
                big = 1.0 + a * a * (v[:, 2] ** -2 - 1.0)
                return np.where(z, 0.0, 2.0 / (1.0 + np.sqrt(big))), (a * a * 2 * e4 / np.abs(v[:, 2]) ** 3 + 4 * EPS) / big + 8 * EPS
            gi, rgi = g1(wi, idh, "g1(wi)")
            go, rgo = g1(wo, odh, "g1(wo)")
            g, rel_g = gi * go, rgi + rgo
        tiny = 8 * EPS
        degenerate = (np.abs(wi[:, 2]) <= tiny) | (np.abs(wo[:, 2]) <= tiny) | (np.abs(odh) <= dd) | ~(length > 64 * EPS)
        degenerate |= ~d_zero & (np.pi * hz ** 4 < 1.2e-38)                        # GGX::d's cos^4 leaves binary32's normal range
        # the reflection branch: brdf and the half-vector pdf through the reflection Jacobian 1 / (4 |o.h|)
        brdf = f * g * d / (4.0 * np.abs(wi[:, 2] * wo[:, 2]))
        pdf_r = d * hz * f * (1.0 / (4.0 * np.abs(odh)))
        rel_pr = (1.0 + rel_d) * (1.0 + dh / np.abs(hz) + rel_f + dd / np.abs(odh) + 16 * EPS) - 1.0
        rel_br = (1.0 + rel_d) * (1.0 + rel_f + rel_g + rel_z + 16 * EPS) - 1.0
        if transmissive:
            tint, rel_tint = np.ones((n, 3)), np.zeros((n, 3))
        else:
            p5 = (1.0 - np.abs(idh)) ** 5
            tint = col + (1.0 - col) * p5[:, None]
            rel_tint = (5.0 * (1.0 - np.abs(idh)) ** 4 * dd)[:, None] * (1.0 - col) / tint + 8 * EPS
        bsdf = brdf[:, None] * tint
        rel_b = rel_br[:, None] + rel_tint
        pdf, rel_p = pdf_r, rel_pr
        if transmissive:
            # the refraction branch, material.rs:406-427
            w = eta * idh + odh
            dw = (eta + 1.0) * dd + e4
            rel_w2 = 2.0 * dw / np.abs(w)
            degenerate = degenerate | (np.abs(w) <= dw)
            z = (1.0 - f) * g * d
            btdf = (np.abs(idh * odh) * z) / (np.abs(wi[:, 2] * wo[:, 2]) * w * w)
            pdf_t = d * (1.0 - f) * np.abs(hz) * (np.abs(odh) / (w * w))
            rel_bt = (1.0 + rel_d) * (1.0 + dd / np.abs(idh) + dd / np.abs(odh) + rel_1f + rel_g + rel_z + rel_w2 + 24 * EPS) - 1.0
            rel_pt = (1.0 + rel_d) * (1.0 + rel_1f + dh / np.abs(hz) + dd / np.abs(odh) + rel_w2 + 16 * EPS) - 1.0
            bsdf = np.where(transmitted[:, None], col * (btdf * eta * eta)[:, None], bsdf)
            rel_b = np.where(transmitted[:, None], rel_bt[:, None], rel_b)
            pdf, rel_p = np.where(transmitted, pdf_t, pdf), np.where(transmitted, rel_pt, rel_p)
        else:
            bsdf = np.where(transmitted[:, None], 0.0, bsdf)                        # BsdfPdf::invalid()
            pdf = np.where(transmitted, 0.0, pdf)
            degenerate = degenerate & ~transmitted
    return bsdf, pdf, rel_b, rel_p, np.full(n, 1e-37), degenerate, dec


# ----------------------------------------------------------------------------------------------------------- the checkers
# Every tolerance below is DERIVED per row from the conditioning of the formula it guards (see material_reference_f64, _half_vector and
# bsdf_reference_f64); the K_* factors multiply them and are 1.  Beside each stands the largest ratio |oracle - binary64| / tolerance
# measured for the CPU oracle over the committed edge set on rows away from every threshold (never anything a GPU returned; the GPU has to
# equal the oracle bit for bit anyway).  Per material, direction / bsdf / pdf / weakening:
#   lambertian 0.18 0.17 0.16 0.18    specular 0.16 0 0 0            dielectric 0.23 0.35 0.19 0
#   metal 0.0  0.02 1.00 1.00 0.21    glass 0.0  0.02 1.00 1.00 0.23
#   metal 0.03 0.04 1.00 1.00 0.21    glass 0.03 0.04 1.00 1.00 0.21
#   metal 0.2  0.10 0.66 0.66 0.21    glass 0.2  0.09 0.54 0.54 0.21
#   metal 0.4  0.11 0.16 0.16 0.19    glass 0.4  0.11 0.17 0.17 0.21
#   metal 1.0  0.09 0.25 0.25 0.19    glass 1.0  0.10 0.21 0.21 0.21
# The 1.00 of the two smallest alphas is attained, not approached: there the half-vector's cosine rounds to exactly 1 in binary32, GGX::d's
# 1 - cos^2 becomes 0, and the result sits on the end of the interval the tolerance is derived from.
K_DIRECTION = 1.0
K_BSDF = 1.0
K_PDF = 1.0
K_WEAKENING = 1.0     # of 8 eps, absolute


def _flips(near_names):
    names = sorted(near_names)
    yield from ((a,) for a in names)
    yield from ((a, b) for i, a in enumerate(names) for b in names[i + 1:])


def _either_branch(evaluate, n):
    """rows that fail `evaluate(rows, flip)` (a bool array per row, plus the _Decide) with every decision taken as binary64 takes it are
    tried again with each decision, and each pair of decisions, that sits within rounding of its threshold taken the other way: a row
    passes when it equals one of the branches.  Returns the rows that equal none."""
    rows = np.arange(n)
    ok, dec = evaluate(rows, ())
    bad = rows[~ok]
    near = {k: np.broadcast_to(v, (n,)) for k, v in dec.near.items()}
    for flip in _flips(k for k, v in near.items() if v[bad].any()):
        if bad.size == 0:
            break
        sel = bad[np.logical_or.reduce([near[k][bad] for k in flip])]
        if sel.size:
            ok2, _ = evaluate(sel, flip)
            bad = np.setdiff1d(bad, sel[ok2])
    return bad


def _close(out, ref, tol):
    """|out - ref| <= tol where both are finite; non-finite values must be non-finite together (an infinity keeps its sign)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(out) & np.isfinite(ref)
        return np.where(fin, np.abs(out - ref) <= tol, (np.isnan(out) & np.isnan(ref)) | (out == ref))


def bsdf_rows_ok(c, bsdf, pdf, incoming, outgoing, normal, front, flip=(), ratios=None):
    """bool per row: bsdf rgb and pdf (binary32, from a probe) equal bsdf_reference_f64 at the same directions.  Discrete: pdf zero or
    not, finite or not.  Continuous: within K * (the row's derived relative rounding) * |value|.  A row whose denominator lies within
    rounding of zero (`degenerate`: wi.z, wo.z, o.h, w or the length of the half-vector before it is normalised) has no binary64 value
    to be near, since the binary32 quotient is rounding noise over rounding noise; such a row is counted and reported, and what holds it
    is the bit-for-bit comparison of the device with the oracle."""
    rb, rp, rel_b, rel_p, abs_p, degenerate, dec = bsdf_reference_f64(c, incoming, outgoing, normal, front, flip)
    bsdf, pdf = np.asarray(bsdf, np.float64), np.asarray(pdf, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tol_b = K_BSDF * rel_b * np.abs(rb) + 1e-37
        tol_p = K_PDF * rel_p * np.abs(rp) + abs_p
        ok_b = _close(bsdf, rb, np.where(np.isfinite(tol_b), tol_b, np.inf)).all(1)
        ok_p = _close(pdf, rp, np.where(np.isfinite(tol_p), tol_p, np.inf))
        zero = ((pdf == 0.0) == (rp == 0.0)) | (np.abs(rp) <= np.where(np.isfinite(tol_p), tol_p, np.inf))
        if ratios is not None:
            fin = np.isfinite(bsdf).all(1) & np.isfinite(rb).all(1) & np.isfinite(pdf) & np.isfinite(rp) & ~degenerate & (rp != 0.0)
            fin &= ~np.logical_or.reduce([np.broadcast_to(v, fin.shape) for v in dec.near.values()] + [np.zeros(fin.shape, bool)])
            ratios.append((np.where(fin[:, None], np.abs(bsdf - rb) / tol_b, 0.0).max(initial=0.0),
                           np.where(fin, np.abs(pdf - rp) / tol_p, 0.0).max(initial=0.0)))
    return (ok_b & ok_p & zero) | degenerate, dec, degenerate


def check_bsdf_eval(out4, material, incoming, outgoing, normal, front):
    """out4 (pt_bsdf_eval / pto_bsdf_eval rows) against bsdf_reference_f64; every row is checked, a row on a threshold against both
    branches.  Returns (rows, degenerate rows, rows whose derived relative tolerance exceeds 1 %) for the caller to report."""
    c = Constants(material)
    out4 = np.asarray(out4)
    args = [np.asarray(a) for a in (incoming, outgoing, normal, front)]
    info = {}

    def evaluate(rows, flip):
        ok, dec, deg = bsdf_rows_ok(c, out4[rows, 0:3], out4[rows, 3], *[a[rows] for a in args], flip=flip)
        if not flip:
            info["degenerate"] = int(deg.sum())
        return ok, dec
    bad = _either_branch(evaluate, len(out4))
    assert bad.size == 0, (f"kind {material.kind} roughness {material.roughness}: {bad.size} rows equal no branch of the binary64 statement; first "
                           f"{bad[0]}: out {out4[bad[0]]}, binary64 {[x[0] for x in bsdf_reference_f64(c, *[a[bad[:1]] for a in args])[:4]]}")
    return len(out4), info["degenerate"]


def check_material_eval(out9, material, incoming, normal, front, uniforms, ratios=None):
    """out9 (pt_material_eval / pto_material_eval rows: direction, bsdf rgb, pdf, weakening, draws) against the binary64 statement, fed
    the binary32 uniforms the stream produced (uniforms[:, 0:3]).

    Discrete, exactly: the number of draws; reflected or refracted and the side of the normal the direction leaves on (both through the
    direction: the two candidates lie far apart, and the side is compared wherever |dot(direction, normal)| exceeds the direction's
    tolerance); pdf zero or not; every output finite or not.
    Continuous: the direction within material_reference_f64's per-row tolerance (the spread of each sqrt(1 - x^2) over the rounding of
    its argument: 1 - cos^2 in refract, 1 - r^2 and 1 - p1^2 - p2^2 in the samplers; the frame's azimuth over |v_.xy|); bsdf and pdf
    against get_bsdf_pdf in binary64 AT THE DIRECTION RETURNED (so that the sampler's rounding is not counted twice) within
    bsdf_reference_f64's per-row relative rounding (GGX::d over the rounding of 1 - cos^2, 1 / (4 |o.h|), 1 / |wi.z wo.z| and the w * w
    of the refraction Jacobian); the weakening |dot(direction, normal)| (1 for the delta materials) within 8 eps.
    Each tolerance is multiplied by its K_* above.  A row with a decision within binary32 rounding of its threshold (the critical
    angle, u < F, u2 < a_, v.z > 0.99999, dot > 0 and the sign tests inside get_bsdf_pdf) has to equal one of the branches' binary64
    results; no row is skipped."""
    c = Constants(material)
    out9 = np.asarray(out9)
    incoming, normal, front, uniforms = np.asarray(incoming), np.asarray(normal), np.asarray(front), np.asarray(uniforms)
    delta = material.kind in (SPECULAR, DIELECTRIC)

    def evaluate(rows, flip):
        o = out9[rows].astype(np.float64)
        d, tol, draws, _, dec = material_reference_f64(c, incoming[rows], normal[rows], front[rows], uniforms[rows], flip)
        ok = (o[:, 8] == draws) & _close(o[:, 0:3], d, K_DIRECTION * tol[:, None]).all(1)
        nrm = normal[rows].astype(np.float64)
        with np.errstate(invalid="ignore"):
            side_o, side_r = _dot(o[:, 0:3], nrm), _dot(d, nrm)
            ok &= (np.sign(side_o) == np.sign(side_r)) | (np.abs(side_r) <= K_DIRECTION * tol * 2.0) | np.isnan(side_r)
            weak = np.ones(len(rows)) if delta else np.abs(side_o)
            ok &= _close(o[:, 7], weak, K_WEAKENING * 8 * EPS)
        fl = tuple(f for f in flip if f.startswith("eval:"))
        ok_b, dec_b, _ = bsdf_rows_ok(c, o[:, 3:6], o[:, 6], incoming[rows], np.where(np.isfinite(o[:, 0:3]), o[:, 0:3], np.nan), nrm, front[rows],
                                      flip=[f[5:] for f in fl], ratios=ratios if not flip else None)
        for k, v in dec_b.near.items():
            dec.near["eval:" + k] = v
        if ratios is not None and not flip:
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(o[:, 0:3]).all(1) & np.isfinite(d).all(1)
                fin &= ~np.logical_or.reduce([np.broadcast_to(v, fin.shape) for k, v in dec.near.items() if not k.startswith("eval:")] + [np.zeros(fin.shape, bool)])
                ratios.append((np.where(fin, np.abs(o[:, 0:3] - d).max(1) / tol, 0.0).max(initial=0.0), np.abs(o[:, 7] - weak).max(initial=0.0) / (8 * EPS)))
        return ok & ok_b, dec
    bad = _either_branch(evaluate, len(out9))
    if bad.size:
        i = bad[:1]
        d, tol, draws, _, dec = material_reference_f64(c, incoming[i], normal[i], front[i], uniforms[i])
        raise AssertionError(f"kind {material.kind} roughness {material.roughness}: {bad.size} rows equal no branch of the binary64 statement; first {i[0]}: "
                             f"out {out9[i[0]]}, binary64 direction {d[0]} +- {tol[0]}, draws {draws[0]}, bsdf/pdf "
                             f"{[x[0] for x in bsdf_reference_f64(c, incoming[i], out9[i, 0:3], normal[i], front[i])[:4]]}, near "
                             f"{[k for k, v in dec.near.items() if np.any(v)]}")


# ------------------------------------------------------------------------------------------------------- the edge inputs
SEED = 0x5EED5EED
ROUGHNESS = (0.0, 0.03, 0.2, 0.4, 1.0)
PROBE_SIZES = (1, 255, 256, 257)          # around the probes' 256-thread blocks; the whole set follows


def materials():
    """the materials under test, by name"""
    from path_tracer_amd.scene_desc import Dielectric, GGX, Lambertian, Specular
    m = {"lambertian": Lambertian.new((0.7, 0.6, 0.5)), "specular": Specular.new((0.9, 0.9, 0.8)), "dielectric": Dielectric.new((0.95, 0.9, 0.85), 1.5, None)}
    for r in ROUGHNESS:
        m[f"metal_{r}"] = GGX.new_metal((0.9, 0.5, 0.2), r)
        m[f"glass_{r}"] = GGX.new_dielectric((0.95, 0.9, 0.85), r, 1.5, None)
    return m


def probe_scene(material):
    """a little scene that holds `material` (the probes look at a material only); returns the scene and the material's index"""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Emissive, Model, SceneDesc
    tri = scenes.cornell_box(8, 8).models[0]
    sc = SceneDesc.new([Model.new(tri.positions, tri.normals, Emissive.new((1, 1, 1))), Model.new(tri.positions + F(10), tri.normals, material)],
                       scenes.cornell_box(8, 8).camera)
    return sc, sc.materials().index(material)


def _normals():
    n = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-0.0, -0.0, 1.0], [-0.0, 0.0, -1.0],
         [1e-4, 0, -1], [-1e-4, 1e-4, -1], [1, 2, 3], [-0.3, 0.5, -0.81], [0.6, -0.64, 0.48], [0.7, 0.7, 1e-3]]
    n = np.array(n, np.float64)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def _angles(material):
    """incidence angles from exactly normal to grazing, and on both sides of each threshold the material has"""
    t = [0.0, 1e-4, 1e-2, 0.1, 0.5, 1.0, 1.3, np.pi / 2 - 1e-2, np.pi / 2 - 1e-4, np.pi / 2 - 1e-6]
    if material.kind in (DIELECTRIC, GGX_DIELECTRIC):
        crit = np.arcsin(1.0 / material.ior)                                 # back faces: total internal reflection beyond it
        t += [crit + k * 6e-8 for k in (-64, -4, -2, -1, 0, 1, 2, 4, 64)]
    if material.kind in (GGX_METAL, GGX_DIELECTRIC):
        a = Constants(material).alpha
        flip = np.arctan(np.sqrt(float(F(0.99999)) ** -2 - 1.0) / a)         # v.z = 1 / sqrt(1 + a^2 tan^2) crosses 0.99999 here (onb.rs:13)
        t += [flip * (1 + s) for s in (-1e-2, -1e-4, -1e-6, -1e-7, 0.0, 1e-7, 1e-6, 1e-4, 1e-2) if flip * (1 + s) < np.pi / 2]
        # v.z = 1 - (a tan)^2 / 2 moves little with the angle: a few binary32 steps per cent.  So also well clear of the flip, both sides
        t += [np.arctan(k * np.tan(flip)) for k in (0.5, 1.5, 2.5)]
    return np.array(t)


def _directions(normal, theta, phi):
    """the unit direction a ray travels in when it meets `normal` at incidence theta, azimuth phi (binary64, then rounded once)"""
    n = normal.astype(np.float64)
    c0, c1 = _onb(n)
    d = -(np.cos(theta)[:, None] * n + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * c0 + np.sin(phi)[:, None] * c1))
    return d.astype(F)


def edge_keys():
    return np.load(EDGE_KEYS)


def _tuples(material, azimuths):
    nrm, th = _normals(), _angles(material)
    ni, ti, pi, fi = np.meshgrid(np.arange(len(nrm)), np.arange(len(th)), np.arange(len(azimuths)), np.arange(2), indexing="ij")
    ni, ti, pi, fi = ni.ravel(), ti.ravel(), pi.ravel(), fi.ravel()
    inc = _directions(nrm[ni], th[ti], np.asarray(azimuths)[pi])
    extra_i, extra_n, extra_f = [], [], []
    if material.kind in (DIELECTRIC, GGX_DIELECTRIC):
        # the binary32 neighbours of the critical direction, one component at a time, on both sides
        at = np.flatnonzero(np.isclose(th[ti], np.arcsin(1.0 / material.ior), rtol=0, atol=1e-9))
        for k in range(3):
            for toward in (-np.inf, np.inf):
                d = inc[at].copy()
                d[:, k] = np.nextafter(d[:, k], F(toward))
                extra_i.append(d); extra_n.append(nrm[ni[at]]); extra_f.append(fi[at])
    if extra_i:
        return np.concatenate([inc] + extra_i), np.concatenate([nrm[ni]] + extra_n), np.concatenate([fi] + extra_f).astype(np.uint8)
    return inc, nrm[ni], fi.astype(np.uint8)


def edge_inputs(material, keys_per_tuple=5):
    """rows for pt_material_eval: every (normal, incidence, azimuth, side) of the material, each under keys_per_tuple stream keys with an
    extreme draw (the committed fixture, dealt round robin) and as many random ones.  Returns incoming, normal, front, pixel, sample."""
    inc, nrm, front = _tuples(material, (0.0, 0.7, 2.1, 3.9, 5.5))
    ek = edge_keys()
    n = len(inc)
    rng = np.random.default_rng(5)
    deal = (np.arange(n)[:, None] * keys_per_tuple + np.arange(keys_per_tuple)[None, :]) % len(ek["pixel"])
    px = np.concatenate([ek["pixel"][deal], rng.integers(0, 1 << 32, (n, keys_per_tuple), dtype=np.uint64).astype(np.uint32)], 1)
    sm = np.concatenate([ek["sample"][deal], rng.integers(0, 4096, (n, keys_per_tuple)).astype(np.uint32)], 1)
    k = px.shape[1]
    return np.repeat(inc, k, 0), np.repeat(nrm, k, 0), np.repeat(front, k), px.ravel(), sm.ravel()


def edge_uniforms(pixel, sample):
    return stream_f32(SEED, pixel, sample, DRAWS_CONSUMED, 3)


def _neighbours(d):
    """d and the vectors one binary32 step away in each of its first two components, both ways"""
    out = [d]
    for k in (0, 1):
        for toward in (-np.inf, np.inf):
            e = d.copy()
            e[:, k] = np.nextafter(e[:, k], F(toward))
            out.append(e)
    return out


def bsdf_inputs(material):
    """rows for pt_bsdf_eval: per (normal, incidence, azimuth, side) the outgoing directions next-event estimation can ask about: anywhere
    on the sphere; within 1e-6 of the surface plane on both sides and in it; the mirror direction and its binary32 neighbours; straight
    on, where wi + wo is nearly zero; and for the rough dielectric the directions that make eta * wi + wo nearly tangential, with z of
    either sign, for both values of eta.  Returns incoming, outgoing, normal, front."""
    inc, nrm, front = _tuples(material, (0.0, 2.1))
    n = len(inc)
    rng = np.random.default_rng(9)
    i64, n64 = inc.astype(np.float64), nrm.astype(np.float64)
    c0, c1 = _onb(n64)
    outs = []
    for _ in range(8):
        d = rng.normal(size=(n, 3))
        outs.append(_unit(d))
    for elev in (1e-6, -1e-6, 1e-7, -1e-7, 0.0):
        az = rng.uniform(0, 2 * np.pi, n)
        outs.append(np.cos(elev) * (np.cos(az)[:, None] * c0 + np.sin(az)[:, None] * c1) + np.sin(elev) * n64)
    outs += _neighbours(_reflect(i64, n64).astype(F))
    outs += _neighbours(inc.copy())[:3]
    if material.kind == GGX_DIELECTRIC:
        woz = -_dot(i64, n64)
        for eta in (float(F(material.ior)), float(F(1.0) / F(material.ior))):
            for s in (1.0 - 1e-6, 1.0, 1.0 + 1e-6, 1.0 + 1e-3):
                z = np.clip(-woz / eta * s, -1.0, 1.0)
                az = rng.uniform(0, 2 * np.pi, n)
                r = np.sqrt(1.0 - z * z)
                outs.append(r[:, None] * (np.cos(az)[:, None] * c0 + np.sin(az)[:, None] * c1) + z[:, None] * n64)
    k = len(outs)
    out = np.stack([np.asarray(o, np.float64).astype(F) for o in outs], 1).reshape(n * k, 3)
    return np.repeat(inc, k, 0), out, np.repeat(nrm, k, 0), np.repeat(front, k)


# ------------------------------------------------------------------------------- designed rays through the shading kernels
PLATE = 4.0
LIGHTS = ("overhead", "in_plane", "edge_on", "low", "far")
VARIANTS = ("lds", "global", "general", "volumes", "textured")
SAMPLES_PER_RAY = 8
EMITTED = (14.0, 12.0, 9.0)
# the materials whose paths can end with nothing gathered (a refracted or absorbed path, a NaN the finisher zeroes): their expected sets hold exact zeros
YIELDS_ZEROS = ("dielectric", "glass_0.0", "glass_0.03", "glass_0.2", "glass_0.4", "glass_1.0", "metal_0.4", "metal_1.0")
TARGETS = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 2.0], [PLATE, 0.0, PLATE], [1.0, 0.0, -2.0]])     # centre, on the shared diagonal, a vertex, inside one triangle


def _quad(p0, p1, p2, p3):
    p = np.array([[p0, p1, p2], [p0, p2, p3]], F)
    n = np.cross(p[0, 1].astype(np.float64) - p[0, 0], p[0, 2].astype(np.float64) - p[0, 0])
    return p, np.broadcast_to((n / np.linalg.norm(n)).astype(F), p.shape).copy()


def _light_quad(name):
    if name == "overhead":                                   # faces down onto the plate
        return _quad((-1, 5, -1), (1, 5, -1), (1, 5, 1), (-1, 5, 1))
    if name == "in_plane":                                   # in the plate's own plane: dot(dir, normal) and the light's cosine are 0 or rounding
        return _quad((6, 0, -1), (6, 0, 1), (8, 0, 1), (8, 0, -1))
    if name == "edge_on":                                    # its plane z = 0 holds the plate's centre: dot(dir, lnormal) = 0 from there
        return _quad((-1, 2, 0), (1, 2, 0), (1, 4, 0), (-1, 4, 0))
    if name == "low":                                        # 1e-3 above the plate's plane, beside it
        return _quad((4.5, 1e-3, -1), (6.5, 1e-3, -1), (6.5, 1e-3, 1), (4.5, 1e-3, 1))
    if name == "far":
        return _quad((-1e3, 1e6, -1e3), (1e3, 1e6, -1e3), (1e3, 1e6, 1e3), (-1e3, 1e6, 1e3))
    raise KeyError(name)


def plate_scene(material, light, variant="lds", width=16, height=16):
    """One two-triangle plate of `material` at y = 0 (normal +y), one emissive quad, a grazing camera.  variant "volumes" adds a distant glass
    ball with a medium (so the scene has volumes), "textured" binds an all-ones texture to the plate's material with every UV on texel
    corner (0, 0), where the bilinear weights are exactly 1, 0, 0, 0.  Returns (the scene for the library, the scene for the oracle,
    which knows no textures, and the renderer flags)."""
    from path_tracer_amd import scenes
    from path_tracer_amd.scene_desc import Camera, Dielectric, Emissive, Model, SceneDesc, Texture, Volume
    s = PLATE
    pp, pn = _quad((-s, 0, -s), (-s, 0, s), (s, 0, s), (s, 0, -s))
    lp, ln = _light_quad(light)
    cam = Camera.new((-7.0, 0.5, 0.5), (0.0, 0.0, 0.0), 60.0, width / height)
    extra = []
    if variant == "volumes":
        t, nr = scenes.sphere_mesh(0, (300.0, -200.0, 100.0), 5.0)
        extra = [Model.new(t.astype(F), nr.astype(F), Dielectric.new((1.0, 1.0, 1.0), 1.5, Volume.new((0.4, 0.1, 0.2), 0.3, 0.5, 0.2)), None, "ball")]
    light_m = Model.new(lp, ln, Emissive.new(EMITTED), None, "light")
    plain = SceneDesc.new([light_m, Model.new(pp, pn, material, None, "plate")] + extra, cam, f"plate, {light}")
    flags = {"global": 2, "general": 16}.get(variant, 0)
    if variant != "textured":
        return plain, plain, flags
    tex = material.textured(Texture.new(np.ones((2, 2, 3), F)))
    lib_scene = SceneDesc.new([light_m, Model.new(pp, pn, tex, None, "plate", uvs=np.zeros((2, 3, 2), F))], cam, f"plate, {light}, textured")
    return lib_scene, plain, flags


def designed_rays(material):
    """rays aimed at the plate's centre, shared diagonal, a vertex and the inside of one triangle, at the incidence angles of _angles
    (the thresholds' angles at the centre only), from above and from below (back faces); each ray SAMPLES_PER_RAY times.  Returns
    origins, directions, keys, samples."""
    base = _angles(material)[:10]
    o, d = [], []
    for ti, p in enumerate(TARGETS):
        th = _angles(material) if ti == 0 else base
        az = 0.3 + 1.1 * ti
        for side in (1.0, -1.0):
            v = np.stack([np.sin(th) * np.cos(az), side * np.cos(th), np.sin(th) * np.sin(az)], 1)
            o.append(p[None, :] + 3.0 * v)
            d.append(-v)
    o, d = np.concatenate(o).astype(F), np.concatenate(d).astype(F)
    n = len(o)
    key = np.repeat(np.arange(n, dtype=np.uint32) + np.uint32(7000), SAMPLES_PER_RAY)
    sample = np.tile(np.arange(SAMPLES_PER_RAY, dtype=np.uint32), n)
    return np.repeat(o, SAMPLES_PER_RAY, 0), np.repeat(d, SAMPLES_PER_RAY, 0), key, sample


_EXPECTED = {}


def oracle_rays(oracle_mod, name, light, variant, depth, nee):
    """Oracle.integrate over designed_rays of the plate scene: (radiance [n, 4], position [n, 4], id byte [n]), computed once per case.
    The oracle's scene differs between variants only by the distant ball."""
    key = (name, light, variant == "volumes", depth, nee)
    if key not in _EXPECTED:
        m = materials()[name]
        orc = oracle_mod.Oracle(plate_scene(m, light, "volumes" if variant == "volumes" else "lds")[1])
        o, d, k, s = designed_rays(m)
        rad = np.zeros((len(k), 4), F); pos = np.zeros((len(k), 4), F); idb = np.zeros(len(k), np.uint8)
        for i in range(len(k)):
            rad[i], pos[i], idb[i] = orc.integrate(o[i], d[i], int(k[i]), int(s[i]), 1, max_bounces=depth, enable_nee=int(nee))
        for a in (rad, pos, idb):
            a.setflags(write=False)
        _EXPECTED[key] = (rad, pos, idb)
    return _EXPECTED[key]


_OUT = {}


def oracle_edge_outputs(O, name):
    """pto_material_eval and pto_bsdf_eval over the whole edge set of one material, computed once and left unchanged"""
    if name not in _OUT:
        m = materials()[name]
        sc, mi = probe_scene(m)
        o = O.Oracle(sc)
        inc, nrm, front, px, sm = edge_inputs(m)
        out = np.stack([o.material_eval(mi, inc[i], nrm[i], front[i], int(px[i]), int(sm[i]), DRAWS_CONSUMED) for i in range(len(px))])
        bi = bsdf_inputs(m)
        out4 = o.bsdf_eval(mi, *bi)
        for a in (out, out4):
            a.setflags(write=False)
        _OUT[name] = dict(m=m, scene=sc, index=mi, inputs=(inc, nrm, front, px, sm), out=out, bsdf_inputs=bi, out4=out4, u=edge_uniforms(px, sm))
    return _OUT[name]


# ------------------------------------------------------------------------------------- a path that meets a NaN pdf after gathering light
def nan_pdf_scene():
    """A Lambertian plate at y = 0 under a wide smooth-dielectric sheet at y = 1 (normal +y) with a small upright light between them.  A ray
    that starts between the two gathers light on the plate by next-event estimation, bounces up and meets the sheet from behind: beyond
    the critical angle Dielectric::f is 1, and a draw of exactly 1.0 is not below it, so refract returns NaN and get_bsdf_pdf a NaN pdf
    (material.rs:501-507, utility.rs:28-31).  NaN < 0 is false: the reference walks on (integrator.rs:243), the NaN weight reaches the sum
    and the finisher returns zero in place of the light already gathered."""
    from path_tracer_amd.scene_desc import Camera, Dielectric, Emissive, Lambertian, Model, SceneDesc
    pp, pn = _quad((-PLATE, 0, -PLATE), (-PLATE, 0, PLATE), (PLATE, 0, PLATE), (PLATE, 0, -PLATE))
    sp, sn = _quad((-20, 1, -20), (-20, 1, 20), (20, 1, 20), (20, 1, -20))
    lp, ln = _quad((4.5, 0.1, -1), (4.5, 0.9, -1), (4.5, 0.9, 1), (4.5, 0.1, 1))
    return SceneDesc.new([Model.new(lp, ln, Emissive.new(EMITTED), None, "light"), Model.new(pp, pn, Lambertian.new((0.7, 0.6, 0.5)), None, "plate"),
                          Model.new(sp, sn, Dielectric.new((0.95, 0.9, 0.85), 1.5, None), None, "sheet")], Camera.new((-3.0, 0.5, 0.0), (0.0, 0.0, 0.0), 60.0, 1.0))


NAN_PDF_RAY = (np.array([0.0, 0.5, 0.0], F), (np.array([0.3, -1.0, 0.1]) / np.linalg.norm([0.3, -1.0, 0.1])).astype(F))
NAN_PDF_DRAW = 8          # draws before the sheet's: camera jitter 1, light choice 1, point on the light 2, bsdf-sampled estimate 2, bounce 2


def nan_pdf_rays():
    """NAN_PDF_RAY under the committed keys and, for contrast, under each key's neighbour: origins, directions, keys, samples"""
    px = edge_keys()["nan_pdf_pixel"]
    key = np.concatenate([px, px + np.uint32(1)]).astype(np.uint32)
    o, d = NAN_PDF_RAY
    return np.tile(o, (len(key), 1)), np.tile(d, (len(key), 1)), key, np.zeros(len(key), np.uint32)
