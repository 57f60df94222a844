"""Adaptive sampling on the device (fspt_render_adaptive): threshold 0 is render(max_ticks) bit for bit on every
pipeline; every tile retired after n ticks holds render(n)'s pixels bit for bit (rnd(), Sobol, emitter NEE, a viewport);
the device's schedule is adaptive_ref.py's on uniform frames of the same seed; the estimator is honest against a
converged frame; the sample counts; the state the call leaves; the JS host."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref as R
import lights_ref as LR
from fspt_amd import PathTracer
from fspt_amd import _lib as L
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
SMALL = dict(max_ticks=64, min_ticks=16, round_ticks=8)


def make_pt(arrays, W, H, pipeline="wavefront", sampler=None, lights=False, viewport=None, memory_limit=None):
    pt = PathTracer(arrays, W, H)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.seed(SEED)
    pt.set_pipeline(pipeline)
    if sampler:
        pt.set_sampler(sampler, 11)
    if lights:
        pt.set_lights("emitters", 0.5)
    if viewport:
        pt.set_viewport(*viewport)
    if memory_limit:
        pt.set_memory_limit(memory_limit)
    return pt


def uniform_frames(arrays, W, H, max_ticks, round_ticks, **kw):
    """frames[n] = render(n) of a fresh tracer, n = R, 2R, ..., max (one tracer, round_ticks at a time)."""
    pt = make_pt(arrays, W, H, **kw)
    out = {}
    for n in range(round_ticks, max_ticks + 1, round_ticks):
        pt.render(round_ticks)
        out[n] = pt.readRadiance()
    pt.close()
    return out


def adaptive(arrays, W, H, target, prm=SMALL, **kw):
    pt = make_pt(arrays, W, H, **kw)
    n = pt.render_adaptive(target, **prm)
    rad, counts, stats = pt.readRadiance(), pt.sample_counts(), pt.adaptive_stats()
    assert pt.pingpong == n == stats["rounds"] * prm["round_ticks"]
    pt.close()
    return rad, counts, stats, n


def mid_threshold(frames, prm, W, H, viewport=None):
    """A threshold that retires about half of the tiles at the first decision point."""
    rt, mn = prm["round_ticks"], prm["min_ticks"]
    m = rt
    for mm, n in R.decision_splits(mn, rt):
        if n == mn:
            m = mm
    vw, vh = viewport if viewport else (W, H)
    E = R.tile_means(R.rel_mse_terms(frames[mn][..., :3], frames[m][..., :3], m, mn), 32, vw, vh)
    E = E[np.isfinite(E)]
    return float(np.median(E)) * 1.0001


# ---- 1: threshold 0 = render(max_ticks) on every pipeline -----------------------------------------------------------
@pytest.mark.parametrize("form", ["megakernel", "wavefront", "stream", "fallback"])
def test_threshold_zero_is_render_max(small_scene, form):
    W, H = 160, 96
    kw = dict(pipeline="wavefront", memory_limit=4 << 20) if form == "fallback" else dict(pipeline=form)
    pt = make_pt(small_scene, W, H, **kw)
    pt.render(64)
    want = pt.readRadiance()
    pt.close()
    rad, counts, stats, n = adaptive(small_scene, W, H, 0.0, **kw)
    assert n == 64 and (counts == 64).all() and stats["samples"] == 64 * W * H
    assert np.array_equal(rad, want)


# ---- 2: a retired tile holds render(count)'s pixels -----------------------------------------------------------------
def check_tiles_match_render(arrays, W, H, viewport=None, **kw):
    frames = uniform_frames(arrays, W, H, SMALL["max_ticks"], SMALL["round_ticks"], viewport=viewport, **kw)
    target = mid_threshold(frames, SMALL, W, H, viewport)
    rad, counts, stats, _ = adaptive(arrays, W, H, target, viewport=viewport, **kw)
    vw, vh = viewport if viewport else (W, H)
    inside = counts[:vh, :vw]
    assert (inside > 0).all() and (counts[vh:] == 0).all() and (counts[:, vw:] == 0).all()
    ns = np.unique(inside)
    assert len(ns) >= 2 and (inside == SMALL["min_ticks"]).mean() > 0.1, ns  # a real share retired early
    for n in ns:
        sel = counts == n
        assert np.array_equal(rad[sel], frames[n][sel]), n
    assert (rad[counts == 0] == 0).all()  # (cleared, never traced)
    return frames, target, stats


@pytest.mark.parametrize("sampler", [None, "sobol"])
def test_retired_tiles_equal_render(small_scene, sampler):
    check_tiles_match_render(small_scene, 160, 96, sampler=sampler)


def test_retired_tiles_equal_render_viewport(small_scene):
    check_tiles_match_render(small_scene, 160, 96, viewport=(120, 70))


@pytest.fixture(scope="module")
def e3():
    return LR.scene_e3()


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_retired_tiles_equal_render_emitters(e3, pipeline):
    check_tiles_match_render(e3, 160, 96, lights=True, pipeline=pipeline)


# ---- 3: the device's schedule is the restatement's ---------------------------------------------------------------------
@pytest.mark.parametrize("viewport", [None, (120, 70)])
def test_schedule_matches_restatement(small_scene, viewport):
    W, H = 160, 96
    frames, target, stats = check_tiles_match_render(small_scene, W, H, viewport=viewport)
    c, e, tied, rounds = R.schedule(frames, target, tile=32, viewport=viewport, **SMALL)
    ok = ~tied
    assert ok.sum() >= c.size // 2
    assert np.array_equal(stats["tile_ticks"][ok], c[ok])
    got, want = stats["tile_err"][ok & (c > 0)], e[ok & (c > 0)]
    assert np.allclose(got, want, rtol=1e-5, atol=0), np.abs(got / want - 1).max()
    if not tied.any():
        assert stats["rounds"] == rounds
    vw, vh = viewport if viewport else (W, H)
    inside = R.expand(stats["tile_ticks"], W, H, viewport=viewport)
    assert stats["samples"] == int(inside.astype(np.uint64).sum())


# ---- 4: the estimator is honest -----------------------------------------------------------------------------------
def test_estimator_honest(medium_scene):
    W, H = 256, 160
    prm = dict(max_ticks=256, min_ticks=32, round_ticks=16)
    pt = make_pt(medium_scene, W, H)
    pt.seed(99)
    pt.render(4096)
    ref = pt.readRadiance()[..., :3].astype(np.float64)
    pt.close()
    frames = uniform_frames(medium_scene, W, H, prm["max_ticks"], prm["round_ticks"])
    target = mid_threshold(frames, prm, W, H) * 0.5
    rad, counts, stats, _ = adaptive(medium_scene, W, H, target, prm)
    r = (rad[..., :3].astype(np.float64) - ref) ** 2 / (rad[..., :3].astype(np.float64) ** 2 + 0.01)
    true = R.tile_means(r, 32, W, H)
    groups = 0
    for n in np.unique(stats["tile_ticks"]):
        sel = stats["tile_ticks"] == n
        if sel.sum() < 3:
            continue
        ratio = true[sel].mean() / stats["tile_err"][sel].mean()
        print("count %d: %d tiles, true / estimated relative MSE %.3f" % (n, sel.sum(), ratio))
        assert 0.5 <= ratio <= 2.0, (n, ratio)
        groups += 1
    assert groups >= 2


# ---- 5: sample counts ---------------------------------------------------------------------------------------------
def test_sample_counts_repeat(small_scene):
    W, H, vp = 150, 90, (131, 77)
    frames = uniform_frames(small_scene, W, H, SMALL["max_ticks"], SMALL["round_ticks"], viewport=vp)
    target = mid_threshold(frames, SMALL, W, H, vp)
    a = adaptive(small_scene, W, H, target, viewport=vp)
    b = adaptive(small_scene, W, H, target, viewport=vp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2]["tile_err"], b[2]["tile_err"]) and np.array_equal(a[2]["tile_ticks"], b[2]["tile_ticks"])
    assert np.array_equal(a[1], R.expand(a[2]["tile_ticks"], W, H, viewport=vp))
    assert (a[1][77:] == 0).all() and (a[1][:, 131:] == 0).all()


# ---- 6: the state the call leaves ------------------------------------------------------------------------------------
def test_state_after_adaptive(small_scene):
    W, H = 96, 64
    fresh = make_pt(small_scene, W, H)
    fresh.render(24)
    want = fresh.readRadiance()
    fresh.close()
    pt = make_pt(small_scene, W, H)
    n = pt.render_adaptive(1e-3, **SMALL)
    nxt = pt.next_rand_base()
    ref = make_pt(small_scene, W, H)
    ref.render(n)
    assert pt.pingpong == ref.pingpong == n and nxt == ref.next_rand_base()
    ref.close()
    pt.clear()
    pt.seed(SEED)
    pt.render(24)
    assert np.array_equal(pt.readRadiance(), want)
    pt.close()
    sh = make_pt(small_scene, W, H)
    sh.set_shard(0, 2)
    with pytest.raises(L.FsptError) as e:
        sh.render_adaptive(0.01, **SMALL)
    assert e.value.code == -6
    sh.close()


# ---- 7: the Node host -------------------------------------------------------------------------------------------------
def test_node_render_adaptive_matches_python(small_scene, tmp_path):
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, target = 96, 64, 2e-3
    rad, counts, _, n = adaptive(small_scene, W, H, target)
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "env", "bins"):
        getattr(small_scene, k).tofile(os.path.join(d, k + ".bin"))
    cam = S.BUNNY_CAMERA
    meta = dict(atlasRes=small_scene.atlas_res, atlasLayers=small_scene.atlas_layers, envW=small_scene.env_w, envH=small_scene.env_h,
                leafSize=small_scene.leaf_size, W=W, H=H, cam=cam, lens=S.lens_features(cam["focal_depth"], cam["aperture"]),
                seed=SEED, target=target, **{k: v for k, v in SMALL.items()})
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "adaptive_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d],
                          timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    got_counts = np.fromfile(os.path.join(d, "counts.bin"), np.uint32).reshape(H, W)
    assert json.load(open(os.path.join(d, "n.json"))) == n
    assert np.array_equal(got, rad) and np.array_equal(got_counts, counts)
