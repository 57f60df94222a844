"""Next-event estimation of emissive triangles (fspt_target_set_lights) on the MI355X.  Pinned three ways:
bit for bit where the mode must reduce to the reference (a scene without emitters; one bounce), against the numpy
restatement (tests/lights_ref.py: the light table, the emitter sample), and by statistics and equality across every
pipeline, scheduler and host entry (no bias, lower error, the same bits everywhere)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lights_ref as R
import oracle as O
from fspt_amd import PathTracer, Scene, light_alias_table
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = S.BUNNY_CAMERA


@pytest.fixture(scope="module")
def e1():
    return R.scene_e1()


@pytest.fixture(scope="module")
def e2():
    return R.scene_e2()


@pytest.fixture(scope="module")
def e3():
    return R.scene_e3()


def make_pt(arrays, W, H, nb=4, lights=True, sampler=None, fraction=0.5, seed=7):
    pt = PathTracer(arrays, W, H, num_bounces=nb)
    pt.set_camera(**CAM)
    pt.seed(seed)
    if sampler:
        pt.set_sampler(sampler, 11)
    if lights:
        pt.set_lights("emitters", fraction)
    return pt


def frame(arrays, W, H, n, pipeline="wavefront", **kw):
    pt = make_pt(arrays, W, H, **kw)
    pt.set_pipeline(pipeline)
    pt.render(n)
    img = pt.readRadiance()
    pt.close()
    return img


def oracle_frame(arrays, W, H, n, nb, seed=7):
    pt = make_pt(arrays, W, H, nb=nb, lights=False, seed=seed)
    want = np.zeros((H, W, 4), np.float32)
    O.render(arrays, W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, nb, 0, n, seed, want)
    pt.close()
    return want


# ---- 1, 2: where the mode must reduce to the reference -------------------------------------------------------------
@pytest.mark.parametrize("sampler", [None, "sobol"])
def test_no_emitters_is_bit_identical(medium_scene, sampler):
    W, H = 96, 64
    sc = Scene(medium_scene)
    assert sc.light_count() == 0
    sc.close()
    off = frame(medium_scene, W, H, 6, lights=False, sampler=sampler)
    for pipeline in ("wavefront", "megakernel", "stream"):
        assert np.array_equal(frame(medium_scene, W, H, 6, pipeline, sampler=sampler), off), pipeline
    if sampler is None:
        assert np.array_equal(off, oracle_frame(medium_scene, W, H, 6, 4))


@pytest.mark.parametrize("scene", ["e1", "e2"])
@pytest.mark.parametrize("sampler", [None, "sobol"])
def test_one_bounce_is_bit_identical(request, scene, sampler):
    arrays = request.getfixturevalue(scene)
    W, H = 96, 64
    off = frame(arrays, W, H, 6, nb=1, lights=False, sampler=sampler)
    for pipeline in ("wavefront", "megakernel", "stream"):
        assert np.array_equal(frame(arrays, W, H, 6, pipeline, nb=1, sampler=sampler), off), (pipeline, sampler)
    if sampler is None:
        assert np.array_equal(off, oracle_frame(arrays, W, H, 6, 1))


# ---- 3, 4: the light table and the emitter sample against the restatement ----------------------------------------------
def test_light_table_e1(e1):
    sc = Scene(e1)
    t = sc.light_table()
    w = R.flat_weights(e1)
    emit = np.nonzero(w > 0)[0]
    assert len(emit) == 2 and sc.light_count() == 2  # the lamp's two triangles
    assert np.array_equal(np.sort(t["tris"]), emit)
    assert np.allclose(t["weights"], w, rtol=1e-4, atol=0)
    real = R.realised(t["prob"], t["alias"]).astype(np.float32)
    tri_p = np.zeros(int(t["slot_tri"].max()) + 1, np.float32)  # (the last leaves read on into padding slots)
    tri_p[t["tris"]] = real
    assert np.array_equal(t["pick"], tri_p[t["slot_tri"]])
    assert np.allclose(real.astype(np.float64), w[t["tris"]] / w.sum(), rtol=1e-6)
    sc.close()


def test_light_table_e2(e2):
    sc = Scene(e2)
    t = sc.light_table()
    n = e2.atlas_res * e2.atlas_res * 4
    layers = np.clip(np.floor(e2.mat.reshape(-1, 12)[:, 1] + np.float32(0.5)), 0, e2.atlas_layers - 1).astype(np.int64)
    lit = np.array([e2.atlas[l * n:(l + 1) * n].reshape(-1, 4)[:, :3].any() for l in range(e2.atlas_layers)])
    emissive_quad = np.nonzero(lit[layers])[0]  # the triangles whose emission layer is not black
    assert len(emissive_quad) == 2
    assert sc.light_count() >= 1 and set(t["tris"]) <= set(emissive_quad.tolist())
    assert (t["weights"][t["tris"]] > 0).all() and (np.delete(t["weights"], t["tris"]) == 0).all()
    real = R.realised(t["prob"], t["alias"])
    assert np.allclose(real, t["weights"][t["tris"]] / t["weights"].sum(), rtol=1e-6)
    tri_p = np.zeros(int(t["slot_tri"].max()) + 1, np.float32)
    tri_p[t["tris"]] = real.astype(np.float32)
    assert np.array_equal(t["pick"], tri_p[t["slot_tri"]])
    sc.close()


def queries(n, seed):
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 10), np.float32)
    q[:, 0:3] = rng.uniform([-1.5, -0.7, -0.9], [1.5, 0.3, 1.0], (n, 3))
    nv = rng.normal(size=(n, 3)); q[:, 3:6] = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    q[:, 6:10] = rng.random((n, 4), dtype=np.float32)
    return q


def test_light_sample_eval_e1(e1):
    sc = Scene(e1)
    t = sc.light_table()
    q = queries(1 << 16, 3)
    tri, out = sc.light_sample_eval(q)
    rtri, x, pdf, le, cn = R.sample(e1, t, q)
    assert np.array_equal(tri, rtri)
    assert np.allclose(out[:, 0:3], x, rtol=1e-5, atol=1e-5)
    ok = pdf < 1e6  # (grazing views: the solid-angle pdf is ill-conditioned)
    assert np.allclose(out[ok, 3], pdf[ok], rtol=1e-4)
    assert np.allclose(out[:, 4:7], le, rtol=1e-6)
    assert np.allclose(out[:, 7], cn, atol=1e-5)
    sc.close()


def test_light_sample_eval_e2_entries(e2):
    sc = Scene(e2)
    t = sc.light_table()
    q = queries(1 << 14, 4)
    tri, out = sc.light_sample_eval(q)
    assert np.array_equal(tri, t["tris"][R.pick_entry(t["prob"], t["alias"], q[:, 7])])
    assert np.isfinite(out).all() and (out[:, 3] >= 0).all() and (out[:, 4:7] >= 0).all()
    sc.close()


# ---- 5: every form gives the same bits ----------------------------------------------------------------------------
FORMS = [
    ("megakernel", {}),
    ("wavefront", {"batch": 1}),
    ("wavefront", {"batch": 8}),
    ("wavefront", {"batch": 32, "tail": 2}),
    ("wavefront", {"batch": 32, "tail": 0}),
    ("stream", {}),
    ("stream", {"pool": 2 * 64 * 8}),
    ("wavefront", {"batch": 32, "memory_limit": 4 << 20}),
]


def render_form(arrays, W, H, pipeline, kw, sampler, n=12, count=0, nb=4):
    pt = make_pt(arrays, W, H, nb=nb, sampler=sampler)
    pt.set_pipeline(pipeline, kw.get("batch", 0))
    if "tail" in kw:
        pt.set_tail(kw["tail"])
    if "pool" in kw:
        pt.set_pool(kw["pool"])
    if "memory_limit" in kw:
        pt.set_memory_limit(kw["memory_limit"])
    if count:
        pt.enable_counters(count)
    pt.render(n)
    acc = pt.readRadiance()
    pt.close()
    return acc


@pytest.mark.parametrize("scene", ["e1", "e2"])
@pytest.mark.parametrize("sampler", [None, "sobol"])
def test_pipelines_and_schedulers_agree(request, scene, sampler):
    arrays = request.getfixturevalue(scene)
    W, H = 128, 96
    ref = render_form(arrays, W, H, "wavefront", {}, sampler)
    for pipeline, kw in FORMS:
        assert np.array_equal(render_form(arrays, W, H, pipeline, kw, sampler), ref), (pipeline, kw)
    for pipeline in ("megakernel", "wavefront", "stream"):
        for count in (1, 2):
            assert np.array_equal(render_form(arrays, W, H, pipeline, {}, sampler, count=count), ref), (pipeline, count)
    pt = make_pt(arrays, W, H, lights=False, sampler=sampler)
    pt.render(12)
    assert not np.array_equal(pt.readRadiance(), ref)  # the mode does change the samples
    pt.close()


@pytest.mark.parametrize("sampler", [None, "sobol"])
def test_deferred_present_shards_viewport(e1, sampler):
    W, H = 96, 64
    pt = make_pt(e1, W, H, sampler=sampler)
    pt.render(10)
    ref = pt.readRadiance()
    pt.clear()
    pt.seed(7)
    for _ in range(10):
        pt.tick()
    assert np.array_equal(pt.readRadiance(), ref)
    pt.clear()
    pt.seed(7)
    for _ in range(10):
        pt.tick()
        pt.present()
    pt.sync()
    assert np.array_equal(pt.readRadiance(), ref)
    pt.close()
    pt = make_pt(e1, W, H, sampler=sampler)
    pt.render(4)
    full = pt.readRadiance()
    pt.close()
    total = np.zeros_like(full)
    for s in range(3):
        pt = make_pt(e1, W, H, sampler=sampler)
        pt.set_shard(s, 3, 32)
        pt.render(4)
        total += pt.readRadiance()
        pt.close()
    assert np.array_equal(total[..., :3], full[..., :3])
    pt = make_pt(e1, W, H, sampler=sampler)
    pt.set_viewport(72, 40)
    pt.render(4)
    part = pt.readRadiance()
    pt.close()
    assert np.array_equal(part[:40, :72], full[:40, :72])
    assert not part[40:].any() and not part[:, 72:].any()


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel", "stream"])
def test_injected_rays(e2, pipeline):
    W, H = 96, 64
    pt = make_pt(e2, W, H)
    pt.drawCamera(1234.5)
    pos, d = pt.readRays()
    pt.clear()
    pt.setRays(pos, d)
    pt.drawTracer(0, 3.0)
    want = pt.readRadiance()
    pt.close()
    pt = make_pt(e2, W, H)
    pt.set_pipeline(pipeline)
    pt.clear()
    pt.setRays(pos, d)
    pt.drawTracer(0, 3.0)
    assert np.array_equal(pt.readRadiance(), want)
    pt.close()


def test_get_and_switch_back(e1):
    W, H = 64, 48
    pt = make_pt(e1, W, H, fraction=0.25)
    assert pt.get_lights() == ("emitters", 0.25)
    pt.render(3)
    pt.set_lights("off")
    assert pt.get_lights()[0] == "off"
    pt.clear()
    pt.seed(7)
    pt.render(5)
    assert np.array_equal(pt.readRadiance(), oracle_frame(e1, W, H, 5, 4))
    pt.close()


# ---- 6, 7: no bias, lower error ----------------------------------------------------------------------------------
def rel_mse(img, ref):
    e = img[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.mean(e * e / (ref[..., :3].astype(np.float64) ** 2 + 0.01)))


def converged(arrays, nb, spp, seed, **kw):
    pt = make_pt(arrays, 96, 64, nb=nb, seed=seed, **kw)
    pt.render(spp)
    img = pt.readRadiance()
    pt.close()
    return img


@pytest.mark.parametrize("scene,nb", [("e1", 4), ("e2", 8)])
def test_no_bias(request, scene, nb):
    arrays = request.getfixturevalue(scene)
    off_a = converged(arrays, nb, 4096, 100, lights=False)
    off_b = converged(arrays, nb, 4096, 200, lights=False)
    on = converged(arrays, nb, 4096, 300)
    m_off, m_on = off_a[..., :3].mean(), on[..., :3].mean()
    print("%s: mean off %.6f on %.6f; relMSE on %.3g off_b %.3g" % (scene, m_off, m_on, rel_mse(on, off_a), rel_mse(off_b, off_a)))
    assert abs(m_on / m_off - 1.0) <= 0.005, (m_on, m_off)
    assert rel_mse(on, off_a) <= 1.2 * rel_mse(off_b, off_a)
    if scene == "e2":
        for f in (0.25, 1.0):
            m = converged(arrays, nb, 4096, 400, fraction=f)[..., :3].mean()
            assert abs(m / m_off - 1.0) <= 0.005, (f, m, m_off)


@pytest.mark.xfail(strict=True, reason="finding (DESIGN 8.3): on E1 at 16 spp the mode's relative MSE is 0.76x (96x64) / "
                   "0.78x (1920x1080) the mode-off error - not below 0.5x")
def test_quality(e1):
    """Relative MSE at 16 spp with the mode on at most half the mode-off error (E1, 4 seeds, against a 4096-spp mode-off
    frame).  Measured on the MI355X: ratio 0.756 at 96x64, 0.78 at 1920x1080 (tools/lights_quality.py) - a gain, but not
    the issue's bound.  Kept as a strict expected failure at that bound, as DESIGN 8.2's test_quality is."""
    ref = converged(e1, 4, 4096, 100, lights=False)
    off = np.mean([rel_mse(converged(e1, 4, 16, s, lights=False), ref) for s in range(1, 5)])
    on = np.mean([rel_mse(converged(e1, 4, 16, s), ref) for s in range(1, 5)])
    print("E1 16 spp relMSE: off %.4g on %.4g ratio %.3f" % (off, on, on / off))
    assert on <= 0.5 * off, (on, off)


# ---- 8: the Node host ------------------------------------------------------------------------------------------
def test_node_set_lights_matches_python(e1, tmp_path):
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")):
        pytest.skip("node or the addon not available")
    W, H, n = 64, 48, 6
    want = frame(e1, W, H, n)
    d = str(tmp_path)
    for k in ("bvh", "tri", "mat", "norm", "uv", "atlas", "bins"):
        getattr(e1, k).tofile(os.path.join(d, k + ".bin"))
    meta = dict(atlasRes=e1.atlas_res, atlasLayers=e1.atlas_layers, leafSize=e1.leaf_size, W=W, H=H, n=n, cam=CAM,
                lens=S.lens_features(CAM["focal_depth"], CAM["aperture"]))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "lights_node_check.js"), os.path.join(ROOT, "fspt_amd", "js"), d],
                          timeout=300)
    got = np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(H, W, 4)
    assert np.array_equal(got, want)


# ---- 9: the hooks, bit for bit against the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["e1", "e2", "e3"])
def test_light_weights_match_oracle(request, scene):
    arrays = request.getfixturevalue(scene)
    sc = Scene(arrays)
    t = sc.light_table()
    sc.close()
    T = arrays.tri.size // 9
    in_leaf = np.zeros(T, bool)
    in_leaf[t["slot_tri"][t["slot_tri"] < T]] = True
    want = np.where(in_leaf, O.light_weights(arrays, np.arange(T)), np.float32(0))
    assert np.array_equal(t["weights"].view(np.uint32), want.view(np.uint32))
    prob, alias = light_alias_table(t["weights"][t["tris"]])
    assert np.array_equal(t["prob"], prob) and np.array_equal(t["alias"], alias)
    assert np.array_equal(R.device_table(t)["light_p"], O.realised_p(prob, alias))
    if scene == "e3":
        assert (t["alias"] != np.arange(t["tris"].size)).any()


def edge_queries(t, n, seed):
    """queries(): then edge values of u1 (0, k / n, prevfloat(1)), the alias coin exactly at prob, and u2 / u3 at 0 and
    prevfloat(1)."""
    q = queries(n, seed)
    m = t["tris"].size
    one = np.nextafter(np.float32(1), np.float32(0))
    k = np.arange(m, dtype=np.float32)
    edge_u1 = np.concatenate([[0.0, one], k / np.float32(m), (k + t["prob"]) / np.float32(m)]).astype(np.float32)
    rows = []
    for u1 in edge_u1:
        for u2 in (0.0, one, 0.5):
            for u3 in (0.0, one, 0.25):
                rows.append((u1, u2, u3))
    r = np.array(rows, np.float32)
    q[:len(r), 7:10] = r
    return q


@pytest.mark.parametrize("scene", ["e2", "e3"])
def test_light_sample_matches_oracle(request, scene):
    arrays = request.getfixturevalue(scene)
    sc = Scene(arrays)
    t = sc.light_table()
    q = edge_queries(t, 1 << 15, 6)
    tri, out = sc.light_sample_eval(q)
    sc.close()
    otri, oout = O.light_sample(arrays, R.device_table(t), q)
    assert np.array_equal(tri, otri)
    assert np.array_equal(out.view(np.uint32), oout.view(np.uint32))


# ---- 10: whole frames, bit for bit against the oracle --------------------------------------------------------------
def oracle_table(arrays, fraction):
    sc = Scene(arrays)
    t = R.device_table(sc.light_table())
    sc.close()
    return t, R.env_q(arrays, fraction)


@pytest.mark.parametrize("scene", ["e1", "e2", "e3"])
@pytest.mark.parametrize("nb", [2, 3, 4, 8, 70])
def test_frames_match_oracle(request, scene, nb):
    """rnd(): per tick (tick 0) and accumulated (ticks 1..3 on top, first_tick 1), every fraction, three pipelines."""
    arrays = request.getfixturevalue(scene)
    W, H = 64, 48
    for fraction in (0.25, 0.5, 1.0):
        lights = oracle_table(arrays, fraction)
        for pipeline in ("megakernel", "wavefront", "stream"):
            pt = make_pt(arrays, W, H, nb=nb, fraction=fraction)
            pt.set_pipeline(pipeline)
            want = np.zeros((H, W, 4), np.float32)
            O.render(arrays, W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, nb, 0, 1, 7, want, lights=lights)
            pt.render(1)
            got = pt.readRadiance()
            assert np.array_equal(got, want), (scene, nb, fraction, pipeline, "tick 0", int((got != want).any(-1).sum()))
            state = pt._rng.value
            pt.render(3)
            O.render(arrays, W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, nb, 1, 3, state, want,
                     lights=lights)
            got = pt.readRadiance()
            pt.close()
            assert np.array_equal(got, want), (scene, nb, fraction, pipeline, "ticks 1-3", int((got != want).any(-1).sum()))


SOBOL_SEED = 11
SOBOL_DIMS = 4 + 12 * 64  # every dimension a path with emitter NEE can reach


@pytest.mark.parametrize("scene", ["e1", "e2", "e3"])
@pytest.mark.parametrize("nb", [2, 4, 70])
def test_sobol_frames_match_oracle(request, scene, nb):
    """Sobol: each tick equals path_replay fed the sampler's values (dims 4..4 + 12 x 64) with the oracle's light table."""
    import sobol_ref as SR
    arrays = request.getfixturevalue(scene)
    W, H = 64, 48
    pix = np.arange(W * H, dtype=np.uint64)[:, None]
    for fraction in (0.25, 1.0):
        lights = oracle_table(arrays, fraction)
        for pipeline in ("megakernel", "wavefront", "stream"):
            pt = make_pt(arrays, W, H, nb=nb, fraction=fraction, sampler="sobol")
            pt.set_pipeline(pipeline)
            for tick in (0, 5):
                pt.clear()
                pt.pingpong = tick
                pt.render(1)
                got = pt.readRadiance().reshape(-1, 4)[:, :3]
                cam = SR.value(SOBOL_SEED, pix, np.uint64(tick), np.arange(4, dtype=np.uint64)[None, :]).reshape(H, W, 4)
                pos, d = O.camera_probe(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, cam)
                rec = SR.value(SOBOL_SEED, pix, np.uint64(tick), np.arange(4, 4 + SOBOL_DIMS, dtype=np.uint64)[None, :])
                col, used, _, _, _ = O.path_replay(arrays, pos, d, rec, np.full(W * H, SOBOL_DIMS, np.uint32), 1.0,
                                                   pt.envTheta, nb, lights=lights)
                assert used.max() <= SOBOL_DIMS
                want = (col / np.float32(tick + 1)).astype(np.float32)
                assert np.array_equal(got, want), (scene, nb, fraction, pipeline, tick, int((got != want).any(-1).sum()))
            pt.close()


# ---- 11: no bias, block by block -----------------------------------------------------------------------------------
# spp per seed (16 seeds per mode): enough that a 3 % shift of one 8x8 block of median noise stands > 5 standard errors out
REGION_SPP = {"e1": 16384, "e2": 4096, "e3": 4096}
REGION_SEEDS = 16
REGION_Z = 5.0


def block_means(arrays, nb, spp, seeds, lights):
    W, H = 96, 64
    out = []
    for s in seeds:
        pt = make_pt(arrays, W, H, nb=nb, seed=s, lights=lights)
        pt.render(spp)
        img = pt.readRadiance()[..., :3].astype(np.float64)
        pt.close()
        out.append(img.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3)) @ R.LUMA)
    return np.array(out)  # [seeds, 8, 12]


def block_z(a, b):
    se = np.sqrt(a.var(0, ddof=1) / len(a) + b.var(0, ddof=1) / len(b))
    d = a.mean(0) - b.mean(0)
    return np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d == 0, 0.0, np.inf)), se


@pytest.mark.parametrize("scene", ["e1", "e2", "e3"])
@pytest.mark.parametrize("nb", [2, 4])
def test_no_bias_per_region(request, scene, nb):
    arrays = request.getfixturevalue(scene)
    spp = REGION_SPP[scene]
    n = REGION_SEEDS
    off = block_means(arrays, nb, spp, range(1, n + 1), False)
    off2 = block_means(arrays, nb, spp, range(101, n + 101), False)
    on = block_means(arrays, nb, spp, range(201, n + 201), True)
    z_on, se = block_z(on, off)
    z_off, _ = block_z(off2, off)
    m = off.mean(0)
    lit = m > 1e-3 * m.max()
    rel_se = se[lit] / m[lit]
    k = np.flatnonzero(lit.ravel())[np.argsort(rel_se)[len(rel_se) // 2]]  # the block of median relative noise
    shifted = on.copy()
    shifted.reshape(n, -1)[:, k] *= 1.03
    z_shift, _ = block_z(shifted, off)
    print("%s nb %d spp %d: max |z| on %.2f, off-off %.2f; 3%% on block %d -> z %.1f; median rel SE %.4f, 3%% detectable "
          "in %d of %d lit blocks" % (scene, nb, spp, np.abs(z_on).max(), np.abs(z_off).max(), k, z_shift.ravel()[k],
                                    np.median(rel_se), int((0.03 / rel_se > REGION_Z).sum()), lit.sum()))
    assert np.abs(z_off).max() < REGION_Z  # the statistic itself is calibrated
    assert abs(z_shift.ravel()[k]) >= REGION_Z  # ... and has the power to see 3 % in a typical block
    assert np.abs(z_on).max() < REGION_Z, np.unravel_index(np.abs(z_on).argmax(), z_on.shape)
