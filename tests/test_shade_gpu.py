"""The shading vertex of every path kernel - shade_hit and its helpers, consume_rays, accumulate_sample as compiled into
k_trace, k_wf_primary, k_wf_logic, k_wf_tail and k_wf_resolve - on the material zoo of tests/shade_cases.py, through the
public API with injected rays: one sample at tick 0 equals the oracle's bit for bit in every pipeline, primary form, tail
setting, counter mode, stash size and ray order, under both samplers, with and without emitter sampling and through the
tile list; the one-bounce colour is within the float64 bound measured on the oracle (tests/test_shade_cpu.py, which also
shows which branches these cases reach); and the running mean equals the oracle's at ticks where float32 stops counting."""
import numpy as np
import pytest

import lights_ref as LR
import lookup_cases as LC
import oracle as O
import shade_cases as SC
import shade_ref as SR
import sobol_ref
from fspt_amd import PathTracer, Scene, logic_set_stash
from test_lookup_gpu import CONFIGS, configure, same_bits

pytestmark = pytest.mark.gpu

SOBOL_SEED = 0x2545F491
SOBOL_DIMS = 4 + 12 * 64          # every dimension a path with emitter NEE can reach
BOUNCES = (1, 2, 4)


@pytest.fixture(scope="module")
def scenes():
    out = {name: Scene(SC.scene(name)[0]) for name in ("zoo", "dim")}
    yield out
    logic_set_stash(-1)
    for sc in out.values():
        sc.close()


def ordered(name, permuted):
    """the scene's rays in their own order (quad after quad) or shuffled over the frame -> (rays, the order)"""
    rays = SC.scene(name)[2]
    order = SC.permutation(len(rays)) if permuted else np.arange(len(rays))
    return rays[order], order


_oracle = {}


def oracle(name, num_bounces, permuted=False, fraction=None, table=None):
    """the oracle's sample of the scene's rays at tick 0 (computed once) -> (radiance [n, 3], first hits)"""
    key = (name, num_bounces, permuted, fraction)
    if key not in _oracle:
        rays, _ = ordered(name, permuted)
        lights = None if fraction is None else (table, SC.env_q(fraction))
        _oracle[key] = SC.oracle_frame(SC.scene(name)[0], rays, num_bounces, lights)
    return _oracle[key]


def tracer(scene, name, num_bounces=4):
    n = len(SC.scene(name)[2])
    pt = PathTracer(scene, LC.FRAME_W, max(1, -(-n // LC.FRAME_W)), num_bounces=num_bounces)
    pt.envTheta = SC.ENV_THETA
    return pt


def sample(pt, rays, tick=0):
    """one sample of the injected rays -> radiance float32 [n, 3]"""
    pos, d = LC.frame(rays)
    assert (pos.shape[1], pos.shape[0]) == pt.resolution
    pt.envTheta = SC.ENV_THETA
    pt.setRays(pos, d)
    pt.clear()
    pt.drawTracer(tick, SC.RAND_BASE)
    return pt.readRadiance().reshape(-1, 4)[:len(rays), :3]


def variations(config):
    """(tail, counters, stash) settings of one pipeline: both tail settings and both stash sizes where a logic kernel runs"""
    pipeline, _ = CONFIGS[config]
    tails = (0, 2) if pipeline == "wavefront" else (-1,)
    stashes = (0, -1) if pipeline != "megakernel" else (-1,)
    return [(t, c, s) for t in tails for c in (0, 1) for s in stashes]


def differing(got, want):
    return int((got != want).any(-1).sum()) if got.shape == want.shape else -1


# ---- 1: every configuration equals the oracle, and so each other -----------------------------------------------------
@pytest.mark.parametrize("num_bounces", BOUNCES)
@pytest.mark.parametrize("name", ["zoo", "dim"])
def test_every_configuration_matches_oracle(scenes, name, num_bounces):
    outputs = {}
    for config in CONFIGS:
        pt = configure(tracer(scenes[name], name, num_bounces), config)
        for tail, count, stash in variations(config):
            pt.set_tail(tail)
            pt.enable_counters(count)
            logic_set_stash(stash)
            for permuted in (False, True):
                rays, order = ordered(name, permuted)
                got = sample(pt, rays)
                if permuted:                 # rnd() is seeded by the hit point alone: a ray's sample does not depend on its pixel
                    back = np.empty_like(got)
                    back[order] = got
                    outputs[(config, tail, count, stash, "permuted")] = back
                else:
                    outputs[(config, tail, count, stash, "in order")] = got
        logic_set_stash(-1)
        pt.close()
    want, fh = oracle(name, num_bounces)
    assert same_bits(oracle(name, num_bounces, True)[0], want[ordered(name, True)[1]])       # ... in the oracle too
    wrong = {k: differing(v, want) for k, v in outputs.items() if not same_bits(v, want)}
    first = next(iter(outputs.values()))
    apart = [k for k, v in outputs.items() if not same_bits(v, first)]
    # all of them wrong and none apart: the kernels share a defect; some apart: those kernels have one of their own
    assert not wrong and not apart, (name, num_bounces, f"{len(wrong)} of {len(outputs)} differ from the oracle", wrong, "apart from the first:", apart)
    assert (fh["index"] >= 0).sum() > 0.9 * len(want) and np.isfinite(want).all()


def test_first_hits_match_oracle(scenes):
    """The zoo's first hits through Scene.intersect, the traversal kernel of its own: the placement of the cases holds on
    the device.  The path kernels' own first hits of the injected rays are held by the radiance above, which is the oracle's
    bit for bit only where every ray found the oracle's hit; test_camera_first_hits_match_oracle reads them out for camera
    rays."""
    rays = SC.scene("zoo")[2]
    fh = oracle("zoo", 1)[1]
    t, index = scenes["zoo"].intersect(rays)[:2]
    assert np.array_equal(index, fh["index"]) and np.array_equal(t[index >= 0], fh["t"][index >= 0])


# ---- 2: the Sobol sampler --------------------------------------------------------------------------------------------
_sobol = {}


def sobol_values(n_pixels):
    """the sampler's values of tick 0 behind the camera's four, per pixel (computed once)"""
    if n_pixels not in _sobol:
        pix = np.arange(n_pixels, dtype=np.uint64)[:, None]
        _sobol[n_pixels] = sobol_ref.value(SOBOL_SEED, pix, np.uint64(0), np.arange(4, 4 + SOBOL_DIMS, dtype=np.uint64)[None, :])
    return _sobol[n_pixels]


_replay = {}


def replay(name, num_bounces, permuted, lights=None, key=None):
    """oracle.path_replay of the scene's frame fed the sampler's values of tick 0 -> clamped colour [n, 3]"""
    k = (name, num_bounces, permuted, key)
    if k not in _replay:
        rays, _ = ordered(name, permuted)
        pos, d = LC.frame(rays)
        n = pos.shape[0] * pos.shape[1]
        rec = sobol_values(n)
        col, used, _, _, _ = O.path_replay(SC.scene(name)[0], pos.reshape(-1, 4), d.reshape(-1, 4), rec, np.full(n, SOBOL_DIMS, np.uint32),
                                           1.0, SC.ENV_THETA, num_bounces, lights=lights)
        assert used.max() <= SOBOL_DIMS
        _replay[k] = col[:len(rays)]
    return _replay[k]


@pytest.mark.parametrize("num_bounces", BOUNCES)
def test_sobol_matches_path_replay(scenes, num_bounces):
    for config in CONFIGS:
        pt = configure(tracer(scenes["zoo"], "zoo", num_bounces), config)
        pt.set_sampler("sobol", SOBOL_SEED)
        for permuted in (False, True):       # the sampler's values belong to the pixel: a shuffled frame is another frame
            got = sample(pt, ordered("zoo", permuted)[0])
            want = replay("zoo", num_bounces, permuted)
            assert same_bits(got, want), (config, num_bounces, permuted, differing(got, want))
        pt.close()


# ---- 3: emitter sampling ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(scenes):
    """the device's light table as the oracle takes it; the table built without a device holds the same triangles"""
    t = LR.device_table(scenes["zoo"].light_table())
    host, _ = SC.host_light_table()
    assert set(t["tris"].tolist()) == set(host["tris"].tolist())
    by_tri = dict(zip(host["tris"].tolist(), host["light_p"].tolist()))
    assert np.array_equal(t["light_p"], np.array([by_tri[k] for k in t["tris"].tolist()], np.float32))
    return t


@pytest.mark.parametrize("sampler", ["reference", "sobol"])
@pytest.mark.parametrize("num_bounces", [2, 4])
@pytest.mark.parametrize("fraction", SC.EMITTER_FRACTIONS)
def test_lights_match_oracle(scenes, table, fraction, num_bounces, sampler):
    lights = (table, SC.env_q(fraction))
    off = oracle("zoo", num_bounces)[0]
    for config in CONFIGS:
        pt = configure(tracer(scenes["zoo"], "zoo", num_bounces), config)
        pt.set_lights("emitters", fraction)
        if sampler == "sobol":
            pt.set_sampler("sobol", SOBOL_SEED)
        for permuted in (False, True):
            got = sample(pt, ordered("zoo", permuted)[0])
            if sampler == "sobol":
                want = replay("zoo", num_bounces, permuted, lights, fraction)
            else:
                want = oracle("zoo", num_bounces, permuted, fraction, table)[0]
            assert same_bits(got, want), (config, fraction, num_bounces, sampler, permuted, differing(got, want))
            assert sampler == "sobol" or permuted or not same_bits(want, off)      # the mode does change the samples
        pt.close()


@pytest.mark.parametrize("sampler", ["reference", "sobol"])
def test_lights_at_one_bounce_are_lights_off(scenes, sampler):
    """num_bounces = 1: no extension ray's hit is shaded, q = 0 at every vertex - the reference's bits"""
    out = []
    for fraction in (None, 0.5):
        pt = tracer(scenes["zoo"], "zoo", 1)
        if sampler == "sobol":
            pt.set_sampler("sobol", SOBOL_SEED)
        if fraction:
            pt.set_lights("emitters", fraction)
        out.append(sample(pt, SC.scene("zoo")[2]))
        pt.close()
    assert same_bits(out[0], out[1])
    assert same_bits(out[0], oracle("zoo", 1)[0] if sampler == "reference" else replay("zoo", 1, False))


# ---- 4: the tile list ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel", "stream"])
def test_tile_list_shades_the_zoo(scenes, pipeline):
    """render_adaptive at threshold 0 is render(max_ticks): the LIST = true instantiations of k_wf_primary and k_wf_tail
    shade the zoo through a camera that sees both of its parts, and give the plain render's bits - the oracle's"""
    W, H = SC.CAMERA_FRAME
    c, n = SC.CAMERA, 8
    frames = []
    for adaptive in (False, True):
        pt = PathTracer(scenes["zoo"], W, H, num_bounces=4)
        pt.set_pipeline(pipeline)
        pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])
        pt.seed(5)
        if adaptive:
            assert pt.render_adaptive(0.0, max_ticks=n, min_ticks=n, round_ticks=n // 2) == n
        else:
            pt.render(n)
        frames.append(pt.readRadiance())
        lens = pt.lensFeatures
        pt.close()
    assert np.array_equal(frames[0], frames[1])
    want = np.zeros((H, W, 4), np.float32)
    O.render(SC.scene("zoo")[0], W, H, c["P"], c["I"], c["fov_scale"], lens, c["env_theta"], 4, 0, n, 5, want)
    assert np.array_equal(frames[0], want) and frames[0][..., :3].max() > 0


def test_camera_first_hits_match_oracle(scenes):
    """features(1, seed) of the zoo from straight above: the diffuse texel, the macro normal and the depth of the first hits
    as a path kernel's own first vertex reads them (test_lookup_gpu.test_guides on the lookup scenes), against the oracle's
    first-hit records - both parts of the zoo, slabs and razor quads in view, about eighty of its quads"""
    from fspt_amd import scene as S
    W, H = SC.OVERHEAD_FRAME
    c, seed = SC.OVERHEAD, 7
    pos, d = O.camera(W, H, c["P"], c["I"], c["fov_scale"], S.lens_features(c["focal_depth"], c["aperture"]), O.rand_base_stream(seed, 1)[0])
    acc = np.zeros((H, W, 4), np.float32)
    fh = O.trace(SC.scene("zoo")[0], W, H, pos, d, 0, SC.RAND_BASE, c["env_theta"], 4, acc, first_hits=True).reshape(H, W)
    pt = PathTracer(scenes["zoo"], W, H, num_bounces=4)
    pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])
    pt.features(1, seed)
    got = pt.readFeatures()
    pt.close()
    hit = fh["index"] >= 0
    assert 2000 < hit.sum() < W * H and len(set((fh["index"][hit] // 2).tolist())) >= 80
    assert np.array_equal(got[..., 7], hit.astype(np.float32))
    assert np.array_equal(got[..., 0:3][hit], fh["diffuse"][hit])
    assert np.array_equal(got[..., 4:7][hit], fh["macro_normal"][hit])
    assert np.array_equal(got[..., 3][hit], fh["t"][hit])


# ---- 5: the float64 bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["megakernel", "wavefront_form1"])
@pytest.mark.parametrize("name", ["zoo", "dim"])
def test_one_bounce_colour_within_float64_bound(scenes, name, config):
    """the GPU's own one-bounce colour against emission + NEE + BSDF miss assembled by shade_ref, at the bound measured on
    the oracle: the same bound on the CPU and on the GPU"""
    V = SC.vertices(name)
    pt = configure(tracer(scenes[name], name, 1), config)
    got = sample(pt, SC.scene(name)[2])
    pt.close()
    one = ~V.any_exempt() & (~V.refracted | V.extension_missed)          # a refracted ray that hits shades on: not one vertex
    dev = SC.deviation(got[V.hit][one], V.ref_colour[one])
    assert dev.max() <= SC.BOUND["colour"], (name, config, int(dev.argmax()), dev.max())
    dev = SC.deviation(got[~V.hit], V.miss_colour)
    assert len(dev) == 0 or dev.max() <= SC.BOUND["colour"]
    assert one.sum() > 0.75 * len(one)


# ---- 6: the running mean at large ticks --------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline,tail", [("megakernel", -1), ("wavefront", 0), ("wavefront", 2), ("stream", -1)])
def test_running_mean_at_large_ticks(pipeline, tail):
    """accumulate_sample in k_trace, k_wf_tail and k_wf_resolve on a preloaded accumulator, at ticks where (float)tick is
    no longer exact and where ft + 1 rounds back to ft: the oracle's bits, NaN, +inf, negative and over-range samples
    included, and within the measured bound of the exact running mean"""
    import torch
    rays, colour, kind = SC.acc_frame()
    pos, d = SC.acc_frame_arrays()
    W, H = SC.ACC_FRAME
    arrays = SC.acc_scene()
    compared = np.array([k != "nan" for k in kind])           # what the clamp makes of NaN the oracle says; float64 does not
    assert {"nan", "inf", "negative", "above", "ordinary", "miss_dim", "miss_bright"} == set(kind)
    sc = Scene(arrays)
    pt = PathTracer(sc, W, H, num_bounces=1)
    pt.set_pipeline(pipeline)
    pt.set_tail(tail)
    pt.envTheta = SC.ENV_THETA
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device=f"cuda:{sc.device}")
    pt.bind_accumulator(acc.data_ptr(), keep=acc)
    pt.setRays(pos, d)
    for tick in SC.ACC_TICKS:
        want = SC.acc_preload()
        O.trace(arrays, W, H, pos, d, tick, SC.RAND_BASE, SC.ENV_THETA, 1, want)
        pt.sync()
        acc.copy_(torch.from_numpy(SC.acc_preload()))
        torch.cuda.synchronize()
        pt.drawTracer(tick, SC.RAND_BASE)
        pt.sync()
        got = acc.cpu().numpy()
        assert same_bits(got, want), (pipeline, tail, tick, differing(got, want))
        ref = SR.running_mean(SC.acc_preload().reshape(-1, 4)[:, :3], colour, tick)
        dev = SC.deviation(got.reshape(-1, 4)[compared, :3], ref[compared])
        assert dev.max() <= SC.BOUND["accumulate"], (pipeline, tail, tick, dev.max())
    pt.close()
    sc.close()
