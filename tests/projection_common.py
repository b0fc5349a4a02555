"""The panoramic and orthographic camera rays of include/pt_api.h (pt_set_projection) restated in numpy binary32, one rounding per operation, with
the oracle's own stream draws, Sobol points, sin/cos (math_batch fn 0) and camera matrices.  tests/test_projection_host.py holds pt_primary_ray to
it bit for bit; tests/test_gpu_projection.py feeds its rays to the oracle's integrator for the expected radiance, as test_gpu_lens.py does."""
import numpy as np

F = np.float32
SEED = 0x5EED5EED
PERSPECTIVE, PANORAMA, ORTHOGRAPHIC = 0, 1, 2
DEG = F(0.017453292)


def _draw(O, state0, k):
    return int(O.lib().pto_wyrand(int(state0), int(k))) & 0xFFFFFFFF


def _unit(w):
    l = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    return (w / l[:, None]).astype(F)


def ndc(O, W, H, pixels, sample, n_sobol=512, seed=SEED):
    """nx, ny of the jittered position of `sample` inside the global pixels `pixels` (y * W + x): main.rs:193-197, camera.rs:96"""
    pixels = np.asarray(pixels, np.int64)
    L = O.lib()
    state0 = [L.pto_stream_state0(seed, int(p), int(sample)) for p in pixels]
    jit = np.array([O.ss_sobol(n_sobol, int(sample), _draw(O, s0, 0)) for s0 in state0], F).reshape(len(pixels), 2)
    gx, gy = (pixels % W).astype(F), (pixels // W).astype(F)
    u, v = (gx + (jit[:, 0] - F(0.5))) / F(W), (gy + (jit[:, 1] - F(0.5))) / F(H)
    nx, ny = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    assert nx.dtype == F and ny.dtype == F
    return nx, ny


def projection_rays(O, orc, W, H, pixels, sample, kind, span_x=0.0, span_y=0.0, ortho_height=0.0, aspect=None, n_sobol=512, seed=SEED):
    """origins [n, 3], directions [n, 3] and the stream draws consumed (1) of the camera rays of `sample` of `pixels` under the camera of the
    oracle `orc` and the projection; aspect: the aspect ratio the camera was set with (ORTHOGRAPHIC)"""
    n = len(pixels)
    m34 = orc.camera_matrices()[0]
    eye, c0, c1, c2 = (m34[:, k].astype(F) for k in (3, 0, 1, 2))
    nx, ny = ndc(O, W, H, pixels, sample, n_sobol, seed)
    if kind == PANORAMA:
        ax = (F(span_x if span_x else 360.0) * F(0.5)) * DEG
        ay = (F(span_y if span_y else 180.0) * F(0.5)) * DEG
        phi, theta = (ax * nx).astype(F), (ay * ny).astype(F)
        sp, cp = O.math_batch(0, phi)
        st, ct = O.math_batch(0, theta)
        dx, dy, dz = ct * sp, st, -(ct * cp)
        w = np.stack([(c0[k] * dx + c1[k] * dy) + c2[k] * dz for k in range(3)], 1)
        assert w.dtype == F
        return np.tile(eye, (n, 1)), _unit(w), 1
    assert kind == ORTHOGRAPHIC and aspect is not None
    hh = F(ortho_height) * F(0.5)
    hw = hh * F(aspect)
    a, b = (hw * nx).astype(F), (hh * ny).astype(F)
    o = np.stack([eye[k] + (c0[k] * a + c1[k] * b) for k in range(3)], 1)
    assert o.dtype == F
    d = _unit((-c2)[None, :])
    return o, np.tile(d, (n, 1)), 1
