"""The Owen-scrambled Sobol sampler (fspt_target_set_sampler) on the MI355X: the device function equals the
numpy restatement bit for bit; camera rays and whole paths equal the oracle's camera_probe / path_replay fed with the
sampler's values in call order; every pipeline, scheduler and host entry gives the same bits; it does not move a frame's
mean; and what it does to the error at equal sample counts is recorded (test_quality)."""
import numpy as np
import pytest

import oracle as O
import sobol_ref as R
from fspt_amd import PathTracer, sampler_eval

pytestmark = pytest.mark.gpu
SIZES = {"small": (96, 64), "medium": (128, 96)}
SEED = 0x2545F491
DIMS = 4 + 8 * 64 + 4  # every dimension a path can reach (+ slack)


def make_pt(arrays, W, H, cam, sampler=True, seed=SEED, nb=4):
    pt = PathTracer(arrays, W, H, num_bounces=nb)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"], cam["aperture"])
    pt.seed(7)
    if sampler:
        pt.set_sampler("sobol", seed)
    return pt


def sobol_rec(W, H, tick, dims, seed=SEED):
    """value(seed, y*W + x, tick, dims) as [H*W, len(dims)] float32."""
    pix = np.arange(W * H, dtype=np.uint64)[:, None]
    return R.value(seed, pix, np.uint64(tick), np.asarray(dims, np.uint64)[None, :])


def oracle_tick(arrays, W, H, pt, tick, seed=SEED):
    """The sample of tick `tick` per pixel: (camera rays, clamped colour [H*W, 3], rnd() calls used)."""
    cam = sobol_rec(W, H, tick, range(4), seed).reshape(H, W, 4)
    pos, d = O.camera_probe(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, cam)
    rec = sobol_rec(W, H, tick, range(4, 4 + DIMS), seed)
    col, used, _, _, _ = O.path_replay(arrays, pos, d, rec, np.full(W * H, DIMS, np.uint32), 1.0, pt.envTheta,
                                       pt.num_bounces)
    return pos, d, col, used


def test_sampler_eval_matches_numpy():
    rng = np.random.default_rng(5)
    n = 1 << 20
    pix = rng.integers(0, 1 << 24, n, dtype=np.uint64)
    smp = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    smp[:4096] = np.arange(4096)
    smp[4096:4200] = 1 << 31
    smp[4200:4300] = (1 << 32) - 1
    dim = rng.integers(0, 521, n, dtype=np.uint64)
    dim[:520] = np.arange(520)
    for seed in (0, SEED):
        got = sampler_eval(seed, pix, smp, dim)
        want = R.value(seed, pix, smp, dim)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.min() >= 0.0 and got.max() < 1.0


def test_camera_rays_match_oracle(small_scene, camera):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    pt.clear()
    for tick in (0, 3):
        pt.drawCamera(1234.5)  # rand_base does not matter under the Sobol sampler
        pos, d = pt.readRays()
        cam = sobol_rec(W, H, tick, range(4)).reshape(H, W, 4)
        opos, od = O.camera_probe(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, cam)
        assert np.array_equal(pos, opos) and np.array_equal(d, od), tick
        pt.drawTracer(tick, 99.0)  # acc_ticks -> tick + 1 ... the next materialisation uses sample 1 + tick
        pt.sync()
        if tick == 0:
            pt.clear()
            pt.render(3)  # ticks 0..2: the next camera draw is sample 3
    pt.close()


@pytest.mark.parametrize("name", ["small", "medium"])
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_whole_path_matches_oracle(small_scene, medium_scene, camera, name, pipeline):
    arrays = small_scene if name == "small" else medium_scene
    W, H = SIZES[name]
    pt = make_pt(arrays, W, H, camera)
    pt.set_pipeline(pipeline)
    for t in (0, 1, 7, 127, 4096, 1 << 20):
        pt.clear()
        pt.pingpong = t
        pt.render(1)
        got = pt.readRadiance().reshape(-1, 4)[:, :3]
        _, _, col, used = oracle_tick(arrays, W, H, pt, t)
        assert used.max() <= DIMS
        want = (col.astype(np.float32) / np.float32(t + 1)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, pipeline, t)
    pt.close()


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


def render_form(arrays, W, H, camera, pipeline, kw, n=12, count=0):
    pt = make_pt(arrays, W, H, camera)
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
    cnt = pt.counters() if count else None
    pt.close()
    return acc, cnt


def test_pipelines_and_schedulers_agree(medium_scene, camera):
    W, H = SIZES["medium"]
    ref, _ = render_form(medium_scene, W, H, camera, "wavefront", {})
    for pipeline, kw in FORMS:
        acc, _ = render_form(medium_scene, W, H, camera, pipeline, kw)
        assert np.array_equal(acc, ref), (pipeline, kw)
    # the counting variants: same accumulator, and the same counts in every pipeline
    counts = []
    for pipeline in ("megakernel", "wavefront", "stream"):
        acc, cnt = render_form(medium_scene, W, H, camera, pipeline, {}, count=1)
        assert np.array_equal(acc, ref), pipeline
        counts.append(cnt)
    assert all(c == counts[0] for c in counts[1:]), counts
    # the result differs from the reference sampler's
    pt = make_pt(medium_scene, W, H, camera, sampler=False)
    pt.render(12)
    assert not np.array_equal(pt.readRadiance(), ref)
    pt.close()


def test_deferred_pairs_and_present_match_render(small_scene, camera):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    pt.render(10)
    ref = pt.readRadiance()
    pt.clear()
    for _ in range(10):
        pt.tick()  # fspt_camera + fspt_trace pairs, recorded and run in batches
    assert np.array_equal(pt.readRadiance(), ref)
    pt.clear()
    for _ in range(10):
        pt.tick()
        pt.present()
    pt.sync()
    assert np.array_equal(pt.readRadiance(), ref)
    pt.close()


def test_shards_sum_to_the_frame_and_viewport(medium_scene, camera):
    W, H = SIZES["medium"]
    pt = make_pt(medium_scene, W, H, camera)
    pt.render(4)
    full = pt.readRadiance()
    pt.close()
    total = np.zeros_like(full)
    for s in range(3):
        pt = make_pt(medium_scene, W, H, camera)
        pt.set_shard(s, 3, 32)
        pt.render(4)
        total += pt.readRadiance()
        pt.close()
    assert np.array_equal(total[..., :3], full[..., :3])
    # a viewport: the pixels inside equal the full frame's, those outside stay as they were (zero)
    pt = make_pt(medium_scene, W, H, camera)
    pt.set_viewport(72, 40)
    pt.render(4)
    part = pt.readRadiance()
    pt.close()
    assert np.array_equal(part[:40, :72], full[:40, :72])
    assert not part[40:].any() and not part[:, 72:].any()


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel", "stream"])
def test_injected_rays_start_at_dim_4(small_scene, camera, pipeline):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    pt.set_pipeline(pipeline)
    pos, d, _, _ = oracle_tick(small_scene, W, H, pt, 0)
    for t in (0, 5):
        pt.clear()
        pt.setRays(pos, d)
        pt.drawTracer(t, 3.0)
        got = pt.readRadiance().reshape(-1, 4)[:, :3]
        rec = sobol_rec(W, H, t, range(4, 4 + DIMS))
        col, _, _, _, _ = O.path_replay(small_scene, pos, d, rec, np.full(W * H, DIMS, np.uint32), 1.0, pt.envTheta,
                                        pt.num_bounces)
        want = (col / np.float32(t + 1)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (pipeline, t)
    pt.close()


def test_switching_back_gives_the_reference(small_scene, camera):
    W, H = SIZES["small"]
    pt = make_pt(small_scene, W, H, camera)
    assert pt.get_sampler() == ("sobol", SEED)
    pt.render(3)
    pt.set_sampler("reference")
    assert pt.get_sampler() == ("reference", 0)
    pt.clear()
    pt.seed(7)
    pt.render(5)
    orc = np.zeros((H, W, 4), np.float32)
    O.render(small_scene, W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, pt.num_bounces, 0, 5, 7, orc)
    assert np.array_equal(pt.readRadiance(), orc)
    pt.close()


def rel_mse(img, ref):
    e = img[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.mean(e * e / (ref[..., :3].astype(np.float64) ** 2 + 0.01)))


@pytest.fixture(scope="module")
def quality_frames(medium_scene, camera):
    W, H = 320, 240

    def frame(spp, sampler, seed):
        pt = make_pt(medium_scene, W, H, camera, sampler=sampler == "sobol", seed=seed, nb=8)
        if sampler != "sobol":
            pt.seed(seed + 1)
        pt.render(spp)
        img = pt.readRadiance()
        pt.close()
        return img

    ref = frame(4096, "reference", 100)
    out = {"ref": ref, "ref2": frame(4096, "reference", 200), "sobol4096": frame(4096, "sobol", 300)}
    for spp in (16, 64):
        for s in ("reference", "sobol"):
            out[(s, spp)] = float(np.mean([rel_mse(frame(spp, s, seed), ref) for seed in range(4)]))
    return out


@pytest.mark.xfail(strict=True, reason="finding (DESIGN 8.2): on the medium scene the Sobol sampler's relative MSE is "
                   "1.03x / 1.02x the reference sampler's at 16 / 64 spp - not below it")
def test_quality(quality_frames):
    """LD relative MSE below the reference sampler's at 16 and 64 spp (medium scene, 320x240, 4 seeds, against a
    4096-spp reference-sampler frame).  Measured on the MI355X: ratios 1.030 (16 spp) and 1.019 (64 spp) - the sampler
    does NOT lower the error of this scene.  Kept as a strict expected failure at the issue's bound: an
    improvement that makes it pass turns it into a failure that asks for this record to be updated."""
    q = quality_frames
    r16 = q[("sobol", 16)] / q[("reference", 16)]
    r64 = q[("sobol", 64)] / q[("reference", 64)]
    print("relMSE ratio sobol/reference: 16 spp %.3f, 64 spp %.3f" % (r16, r64))
    assert r16 < 1.0 and r64 < 1.0, (r16, r64)


def test_no_bias(quality_frames):
    q = quality_frames
    m_ref, m_ld = q["ref"][..., :3].mean(), q["sobol4096"][..., :3].mean()
    assert abs(m_ld / m_ref - 1.0) <= 0.005, (m_ld, m_ref)
    assert rel_mse(q["sobol4096"], q["ref"]) <= 2.0 * rel_mse(q["ref2"], q["ref"])
