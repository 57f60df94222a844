"""The stand-alone passes of fspt_passes.hip, pinned byte for byte: ray generation under every camera model, the denoiser's
guides, the temporal G-buffer, Scene.intersect, the two test hooks and adaptive sampling's tile passes.

These kernels were moved out of fspt_kernels.hip and, where two copies existed (k_camera / k_camera_model, k_features /
k_features_model), unified.  tests/golden/passes_digests.json holds the SHA-256 of every case's output bytes as the library
of commit f008645 ("Move scene construction to fspt_scene.cpp, one install per scene part": the last one with the kernels
in their old place) produced them, built as an A/B library with tools/build_ab.sh and selected with FSPT_LIB; two runs of
that library agreed on every case.  The scenes are the suite's own (small_scene, rays.chain_scene); what this file adds to
them - rays, ray-buffer patterns, moves - is made of exactly representable numbers and elementwise float32 operations.

Shapes: 33 x 17 targets (odd, smaller than a 16 x 16 block in one direction, more than one block in the other; STEREO needs
an even height: 33 x 18), a 31 x 15 viewport, and next to the small scene the 64-leaf chain whose depth-63 tree needs 64
stack entries per lane = 64 KB of LDS per block, so that the launchers' opt-in to more than 48 KB runs."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from rays import chain_scene
from fspt_amd import PathTracer, Scene, _lib as L, sampler_eval, scene as S

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "passes_digests.json")
W, H, VW, VH = 33, 17, 31, 15
MODELS = ("pinhole", "ortho", "fisheye", "equirect", "stereo")
MODEL_KW = {"pinhole": {}, "ortho": {}, "fisheye": {"angle": 2.5}, "equirect": {}, "stereo": {"ipd": 0.125}}
CHAIN_LEAVES = 64
MATH_OPS = ("sin", "cos", "atan2", "asin", "exp2", "div", "sqrt", "rnd", "fract", "log2", "pow")  # fspt_math_eval's op 0 .. 10


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def height(model):
    return H + 1 if model == "stereo" else H


class Ctx:
    """The two scenes (arrays, a device scene, a camera), made once and never changed by a case."""

    def __init__(self, small_arrays):
        chain = chain_scene(CHAIN_LEAVES, small_arrays)
        self.arrays = {"small": small_arrays, "chain": chain}
        self.scene = {k: Scene(a) for k, a in self.arrays.items()}
        assert self.scene["chain"].depth + 1 > 48  # stack entries per lane: 4 waves x 64 lanes x 4 B each, more than 48 KB
        self.cam = {"small": dict(S.BUNNY_CAMERA),
                    "chain": dict(P=[CHAIN_LEAVES + 2.5, 0.0625, 0.125], I=[-1.0, -0.015625, -0.03125], fov_scale=0.5, env_theta=1.625,
                                  focal_depth=2.0, aperture=0.015625)}

    def tracer(self, name, w, h, scene=None, aperture=None, bounces=2):
        pt = PathTracer(scene if scene is not None else self.scene[name], w, h, num_bounces=bounces)
        cam = dict(self.cam[name])
        if aperture is not None:
            cam["aperture"] = aperture
        pt.set_camera(**cam)
        pt.seed(3)
        return pt


def rays_case(ctx, sampler, model, lens):
    h = height(model)
    pt = ctx.tracer("small", W, h, aperture=0.03125 if lens else 0.0)
    if sampler == "sobol":
        pt.set_sampler("sobol", 5)
    if model != "pinhole":
        pt.set_camera_model(model, **MODEL_KW[model])
    mark = (np.arange(W * h * 4, dtype=np.float32).reshape(h, W, 4) * 0.25) - 100.0  # what the edge pixels must keep
    pt.setRays(mark, mark * 2)
    pt.set_viewport(VW, VH)
    pt.drawCamera(1234.5)
    pos, d = pt.readRays()
    outside = np.ones((h, W), bool); outside[:VH, :VW] = False
    assert np.array_equal(pos[outside], mark[outside]) and np.array_equal(d[outside], (mark * 2)[outside])
    assert not np.array_equal(pos[~outside], mark[~outside])
    pt.close()
    return {"rays": digest(pos, d)}


def guides_case(ctx, name, model):
    pt = ctx.tracer(name, W, height(model))
    if model != "pinhole":
        pt.set_camera_model(model, **MODEL_KW[model])
    pt.features(samples=3, seed=1)
    f = pt.readFeatures()
    pt.close()
    return {"features": digest(f)}


def gbuffer_case(ctx, name):
    """first frame (no previous camera), a moved camera, and a frame after update_geometry between motion_begin and _end;
    on a scene of its own, because the last one moves it"""
    arrays = ctx.arrays[name]
    sc = Scene(arrays)
    pt = ctx.tracer(name, W, H, scene=sc)
    out = {}

    def frame(key):
        pt.clear()
        pt.seed(5)
        pt.render(1)
        pt.temporal_accumulate(read=False)
        g, m = pt.temporal_gbuffer()
        out[key] = digest(g, m)
        return g, m

    _, m = frame("first")
    assert (m == 0).all()
    cam = dict(ctx.cam[name])
    cam["P"] = [float(np.float32(p) + np.float32(o)) for p, o in zip(cam["P"], (0.125, 0.0625, -0.0625))]
    pt.set_camera(**cam)
    _, m = frame("moved")
    assert (m[..., 3] != 0).any()
    sc.motion_begin()
    tri = (arrays.tri.reshape(-1, 3) + np.array([0.03125, -0.015625, 0.0625], np.float32)).astype(np.float32).reshape(-1)
    pt.update_geometry(tri, arrays.norm)
    frame("motion")
    sc.motion_end()
    pt.close()
    sc.close()
    return out


def fixed_rays(arrays, n, along_x):
    """n rays of exactly representable numbers: origins in and around the scene's box, aimed at points inside it (not
    normalised); along_x: the first half starts beyond the +x end and looks down the whole length of the box"""
    rng = np.random.default_rng(11)
    v = arrays.tri.reshape(-1, 3)
    lo, ext = v.min(0).astype(np.float32), (v.max(0) - v.min(0)).astype(np.float32)
    u = (rng.integers(0, 257, (n, 3)).astype(np.float32) / np.float32(64) - np.float32(1.5))
    w = rng.integers(0, 65, (n, 3)).astype(np.float32) / np.float32(64)
    o, tgt = lo + ext * u, lo + ext * w
    if along_x:
        k = (n + 1) // 2
        o[:k, 0] = lo[0] + ext[0] + np.float32(2.0)
        tgt[:k, 0] = lo[0]
    d = tgt - o
    d[(d == 0).all(1)] = [1.0, 0.0, 0.0]
    return np.concatenate([o, d], 1).astype(np.float32)


def intersect_case(ctx, name, two_level, n):
    rays = fixed_rays(ctx.arrays[name], n, along_x=name == "chain")
    t, idx, steps, leaves = ctx.scene[name].intersect(rays, two_level=two_level)
    assert t.shape == (n,) and (idx >= 0).any()
    return {"t": digest(t), "index": digest(idx), "steps": digest(steps), "leaves": digest(leaves)}


def sampler_case(ctx):
    k = np.arange(257, dtype=np.uint32)
    return {"values": digest(sampler_eval(5, k * np.uint32(977), k % 7, k % 19))}


def math_case(ctx):
    rng = np.random.default_rng(13)
    a = (rng.integers(-4096, 4097, 513).astype(np.float32) / np.float32(512))
    b = (rng.integers(-4096, 4097, 513).astype(np.float32) / np.float32(256))
    out = {}
    for op, name in enumerate(MATH_OPS):
        r = np.zeros_like(a)
        L.check(L.lib().fspt_math_eval(0, op, L.fptr(a), L.fptr(b), a.size, L.fptr(r)))
        out[name] = digest(r.view(np.uint32))
    assert len(set(out.values())) == len(MATH_OPS)
    return out


def adaptive_case(ctx):
    """3 x 32769 pixels = 1 x 1025 tiles of 32 pixels: the first tile list is longer than one 1024-tile chunk of
    k_adaptive_select, in the smallest frame that has so many tiles"""
    w, h = 3, 32 * 1024 + 1
    pt = ctx.tracer("small", w, h)
    n = pt.render_adaptive(0.0625, max_ticks=8, min_ticks=4, round_ticks=2)
    counts, st = pt.sample_counts(), pt.adaptive_stats()
    pt.close()
    assert st["tile_ticks"].size == 1025 and 4 <= n <= 8 and counts.max() == n
    assert len(np.unique(st["tile_ticks"])) > 1  # tiles retire in different rounds: k_adaptive_select keeps some and drops others
    return {"counts": digest(counts), "tile_ticks": digest(st["tile_ticks"]), "tile_err": digest(st["tile_err"]),
            "totals": digest(np.array([st["rounds"], st["samples"]], np.uint64))}


CASES = {}
for _s in ("reference", "sobol"):
    for _m in MODELS:
        for _l in (False, True):
            CASES[f"rays-{_s}-{_m}-{'lens' if _l else 'nolens'}"] = (rays_case, (_s, _m, _l))
for _n in ("small", "chain"):
    for _m in MODELS:
        CASES[f"guides-{_n}-{_m}"] = (guides_case, (_n, _m))
    CASES[f"gbuffer-{_n}"] = (gbuffer_case, (_n,))
    for _t in (False, True):
        for _k in (1, 255, 256, 257):
            CASES[f"intersect-{_n}-{'quads' if _t else 'nodes'}-{_k}"] = (intersect_case, (_n, _t, _k))
CASES["sampler_eval"] = (sampler_case, ())
CASES["math_eval"] = (math_case, ())
CASES["render_adaptive"] = (adaptive_case, ())


def run_case(ctx, name):
    fn, args = CASES[name]
    return fn(ctx, *args)


@pytest.fixture(scope="module")
def ctx(small_scene):
    return Ctx(small_scene)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_lists_exactly_the_cases(table):
    assert table["recorded_from"].startswith("f008645") and sorted(table["digests"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pass_output_is_the_recorded_one(ctx, table, name):
    got = run_case(ctx, name)
    want = table["digests"][name]
    assert got == want, (name, [k for k in want if got.get(k) != want[k]])
