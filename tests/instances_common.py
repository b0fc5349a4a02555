"""Shared by tests/test_instances_host.py and tests/test_gpu_instances.py: chains of instance moves on a scene description.

A chain is a list of steps; a step is a list of (model index, matrices [n, 3, 4]) handed to Renderer.set_instances before ONE rebuild.  apply()
gives the scene description a build from nothing would be given after the step: a moved scene IS a fresh scene with other matrices."""
import copy

import numpy as np

from path_tracer_amd import scenes
from path_tracer_amd.scene_desc import EMISSIVE, IDENTITY_3x4, SceneDesc, is_rigid

QUARTER_Y = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]], np.float32)
QUARTER_X = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0]], np.float32)


def shifted(m34, t):
    """the same rotations, translations moved by t: rigid whatever t is (model.rs:40-44 looks at the 3x3 only)"""
    m = np.array(m34, np.float32).reshape(-1, 3, 4).copy()
    m[:, :, 3] += np.asarray(t, np.float32)
    return m


def placed(rot34, t):
    m = np.array(rot34, np.float32).copy()
    m[:, 3] = np.asarray(t, np.float32)
    assert is_rigid(m)
    return m


def apply(desc, step):
    models = [copy.copy(m) for m in desc.models]
    for mi, mats in step:
        models[mi].matrices = np.ascontiguousarray(mats, np.float32).reshape(-1, 3, 4)
    return SceneDesc.new(models, desc.camera, desc.name)


def move(r, step):
    for mi, mats in step:
        r.set_instances(mi, mats)
    r.rebuild()


def chain(desc, seed, movable=None):
    """one model; all models; identity -> general -> identity; 1 -> 3 -> 0 -> 2 instances; the emissive model (lights TLAS)"""
    rng = np.random.default_rng(seed)
    n = len(desc.models)
    movable = list(range(n)) if movable is None else list(movable)
    light = next(i for i, m in enumerate(desc.models) if m.material.kind == EMISSIVE)
    solid = [i for i in movable if desc.models[i].material.kind != EMISSIVE]   # (the count chain empties a model: the scene keeps its lights)
    a, b = solid[-1], solid[0]
    origin = desc.models[a].matrices[0][:, 3] if len(desc.models[a].matrices) else np.zeros(3, np.float32)
    ident = placed(IDENTITY_3x4, (0.0, 0.0, 0.0))
    steps = [
        [(a, shifted(desc.models[a].matrices, (10.0, 0.0, -5.0)))],                                                        # one model
        [(i, shifted(desc.models[i].matrices, (float(i % 5) - 2.0, 1.0, 3.0 - float(i % 3)))) for i in range(n)],           # all models
        [(a, ident[None])],                                                                                                # (count may change)
        [(a, scenes.general_turn(rng)[None])],                                                                             # identity -> general
        [(a, ident[None])],                                                                                                # -> identity
        [(b, placed(QUARTER_Y, origin)[None])],                                                                            # 1 instance
        [(b, np.stack([placed(QUARTER_X, origin + np.float32(30.0)), scenes.general_turn(rng), placed(IDENTITY_3x4, (5.0, -7.0, 11.0))]))],  # 3
        [(b, np.zeros((0, 3, 4), np.float32))],                                                                            # 0: out of both TLASes
        [(b, np.stack([scenes.general_turn(rng), placed(QUARTER_Y, (-20.0, 4.0, 9.0))]))],                                 # 2
        [(light, shifted(desc.models[light].matrices, (0.0, -20.0, 0.0)))],                                                # the lights TLAS
        [(light, np.concatenate([shifted(desc.models[light].matrices, (0.0, -20.0, 0.0)), scenes.general_turn(rng, 20)[None] + np.float32(0.0)]))],
    ]
    return steps
