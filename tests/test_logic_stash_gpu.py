"""k_wf_logic's LDS stash (fspt_logic_set_stash): the lanes that own a shaded path park its state rows in LDS
beside the finishing paths' fetch, and the dense shading pass reads them from there - or from memory, for the listed paths
beyond the stash's capacity.  The same bits must reach the same arithmetic, so every frame here is == the frame of the same
call with the stash off (0), and one case per group is also == an independent reference: the CPU oracle, or - for the sampler
and the light mode the oracle does not have - the megakernel pipeline, which has no logic kernel.

The shapes are where the stash can go wrong, not the workload's: a small frame whose block iterations list a few hundred
shaded paths each (cap 1 and 64: both sources feed one shading pass; -1: everything parked), one launch large enough that a
thread owns more than one path per iteration, and every kernel variant whose rows mean something else."""
import numpy as np
import pytest

import lights_ref as R
import oracle as O
from fspt_amd import PathTracer, logic_set_stash
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu

W, H, TICKS, NB, SEED = 64, 48, 8, 8, 31
VARIANT_CAM = dict(P=[0.3, 1.2, 3.4], I=[-0.05, -0.3, -0.95], fov_scale=0.5, env_theta=1.66, focal_depth=2.0, aperture=0.02,
                   lens=[0.5, 0.02])


def many_sets_scene():
    """720 quads of distinct materials: more texture sets than WF_LDS_TABLE_MAX holds, so the logic kernel stages no tables and
    the stash starts at the bottom of the dynamic LDS (tests/test_parity_gpu.py: test_more_layers_than_the_lds_table_holds)"""
    rng = np.random.default_rng(12)
    props = []
    for i in range(720):
        c = [round(float(x), 3) for x in rng.uniform(0.05, 1.0, 3)]
        props.append({"path": "synthetic/quad.obj", "scale": 0.45, "rotate": [{"angle": float(rng.uniform(0, 6.28)), "axis": [1, 0.3, 0.2]}],
                      "translate": [float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-0.8, 0.8)), float(rng.uniform(-1.5, 0.5))],
                      "emittance": [0, 0, 0], "diffuse": c, "metallicRoughness": [round(i / 1000, 4), round(0.1 + i / 900, 4), 0],
                      "emission": [round(0.001 * i, 4), 0, 0], "normals": "flat"})
    env, w, h = S.synthetic_env(64, 32)
    arrays = S.build_scene(props, {"synthetic/quad.obj": S.QUAD_OBJ}, env=env, env_w=w, env_h=h)
    assert arrays.atlas_layers > 1024
    return arrays


@pytest.fixture(scope="module")
def scenes(small_scene, medium_scene, camera):
    """name -> (arrays, camera), built once"""
    from test_goldens import scene_from_golden
    return {"small": (small_scene, camera), "medium": (medium_scene, camera), "emissive": (R.scene_e3(), camera),
            "refractive": (scene_from_golden("variant"), VARIANT_CAM), "many_sets": (many_sets_scene(), camera)}


def frame(arrays, cam, stash, w=W, h=H, ticks=TICKS, pipeline="wavefront", sampler=None, lights=False, budget=None, pool=None):
    """(radiance, live-path fractions); every round goes through the trace / logic kernels (set_tail(0)), one batch"""
    pt = PathTracer(arrays, w, h, num_bounces=NB)
    pt.set_pipeline(pipeline, 0)
    pt.set_tail(0)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    if sampler:
        pt.set_sampler(sampler, 11)
    if lights:
        pt.set_lights("emitters", 0.5)
    if budget is not None:
        pt.set_trace_budget(budget)
    if pool is not None:
        pt.set_pool(pool)
    pt.seed(SEED)
    logic_set_stash(stash)
    try:
        pt.render(ticks)
        img = pt.readRadiance()
        live = pt.live_paths(4) if pipeline == "wavefront" else None
    finally:
        logic_set_stash(-1)
        pt.close()
    return img, live


def oracle_frame(arrays, cam, w=W, h=H, ticks=TICKS):
    want = np.zeros((h, w, 4), np.float32)
    O.render(arrays, w, h, cam["P"], cam["I"], cam["fov_scale"], cam["lens"], cam["env_theta"], NB, 0, ticks, SEED, want)
    return want


_off = {}


def stash_off(scenes, name, **kw):
    """the frame of the same call with the stash off, computed once per case"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _off:
        _off[key] = frame(*scenes[name], 0, **kw)
    return _off[key]


def differ(a, b):
    return f"{int((a != b).any(-1).sum())} of {a.shape[0] * a.shape[1]} pixels differ"


def test_setting_is_checked():
    from fspt_amd import _lib as L
    assert L.lib().fspt_logic_set_stash(-2) == -1 and b"fspt_logic_set_stash" in L.lib().fspt_last_error()
    for n in (0, 1, 1 << 20, -1):
        assert L.lib().fspt_logic_set_stash(n) == 0


def test_stash_off_is_the_oracle_and_lists_more_than_the_small_caps(scenes):
    """the yardstick of every comparison below is itself the oracle's frame, and the small frame's round-2 launch has
    48 block iterations of at most 512 paths, most of them shaded: more than cap 64 per iteration"""
    arrays, cam = scenes["small"]
    off, live = stash_off(scenes, "small")
    assert np.array_equal(off, oracle_frame(arrays, cam)), differ(off, oracle_frame(arrays, cam))
    assert live[1] > 0.5, live[1]  # > 256 of an iteration's 512 paths are listed in round 2


@pytest.mark.parametrize("stash", [1, 64, -1])
def test_small_frame_every_setting(scenes, stash):
    off, _ = stash_off(scenes, "small")
    got, _ = frame(*scenes["small"], stash)
    assert np.array_equal(got, off), differ(got, off)


@pytest.mark.parametrize("stash", [64, -1])
def test_more_than_one_path_per_thread(scenes, stash):
    """512 x 256 x 8 ticks: the round-2 launch has more live paths than 1 024 resident blocks x 512 threads, so a thread owns
    two paths per iteration (u_eff = 2): its second path's place in the list comes from the second pass's counts"""
    kw = dict(w=512, h=256)
    off, live = stash_off(scenes, "small", **kw)
    assert live[1] * 512 * 256 * TICKS > 1024 * 512, live[1]
    got, _ = frame(*scenes["small"], stash, **kw)
    assert np.array_equal(got, off), differ(got, off)


VARIANTS = {
    # name: (scene, frame() arguments, reference: "oracle" or the arguments of the megakernel frame)
    "sobol": ("small", dict(sampler="sobol"), "megakernel"),
    "emitter_nee": ("emissive", dict(lights=True), "megakernel"),
    "emissive": ("emissive", dict(), "oracle"),
    "refractive": ("refractive", dict(), "oracle"),
    "suspended": ("medium", dict(budget=3), "oracle"),
    "stream": ("medium", dict(pipeline="stream", pool=8192), "oracle"),
    "many_sets": ("many_sets", dict(), "oracle"),
}


@pytest.mark.parametrize("stash", [64, -1])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variants_whose_rows_differ(scenes, variant, stash):
    """Sobol: E.w carries the pixel and is always written; emitter NEE: WF_FLAG_LQ without a shadow ray, D.w = q / pb, P.w = the
    shadow bound; emissive: the colour row is non-zero before round 2; refractive: paths outlive the bounce budget; suspended:
    a trace budget of 3 steps, so carry blocks run in the logic launches and WF_HIT_PENDING paths are neither finished nor
    parked; stream: the stream scheduler's pool-sized launches; many_sets: no staged tables in front of the stash."""
    name, kw, ref = VARIANTS[variant]
    off, _ = stash_off(scenes, name, **kw)
    got, _ = frame(*scenes[name], stash, **kw)
    assert np.array_equal(got, off), differ(got, off)
    if stash == -1:  # one case per group against the independent reference
        if ref == "oracle":
            want = oracle_frame(*scenes[name])
        else:
            want, _ = frame(*scenes[name], 0, **dict(kw, pipeline="megakernel"))
        assert np.array_equal(got, want), differ(got, want)
