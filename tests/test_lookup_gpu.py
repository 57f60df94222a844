"""The lookups of the HIP path tracer, each isolated through the public API and held to the oracle bit for bit AND to
the float64 reference (tests/lookup_ref.py) within the tolerances measured on the oracle (tests/lookup_cases.py):

  environment   setRays + drawTracer at num_bounces = 0: a ray that misses leaves clamp(env_sample(rd), 0, 1024) in the
                accumulator at tick 0 - env_taps and the tiling of tile_environment / k_ap_env_tile;
  emission      num_bounces = 1 on a scene without an environment: 30 * texEmissive * texDiffuse of the first vertex -
                material<> in every storage form, hit_geom's barycentrics and uvs;
  guides        features(1, seed): texDiffuse, macro_normal and depth of the camera's first hits - the diffuse and normal
                layers, the tangent frame.

The bit-equality catches what the kernels do differently from the oracle, the float64 bound what the two share."""
import numpy as np
import pytest

import hitref
import lookup_cases as LC
import lookup_ref as LR
import oracle as O
from fspt_amd import PathTracer, Scene, set_texture_interleave_budget
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu

RAND_BASE = 0.5
DEFAULT_BUDGET = 8 << 30
CONFIGS = {"megakernel": ("megakernel", 0), "wavefront_form1": ("wavefront", 1), "wavefront_form2": ("wavefront", 2),
           "stream": ("stream", 0)}


def configure(pt, config):
    pipeline, form = CONFIGS[config]
    pt.set_pipeline(pipeline)
    if form:
        pt.set_primary_form(form)
    return pt


def probe(pt, rays, env_theta=0.0):
    """one sample of the injected rays at tick 0 -> radiance float32 [n, 3]"""
    pos, d = LC.frame(rays)
    assert (pos.shape[1], pos.shape[0]) == pt.resolution
    pt.envTheta = float(env_theta)
    pt.setRays(pos, d)
    pt.clear()
    pt.drawTracer(0, RAND_BASE)
    return pt.readRadiance().reshape(-1, 4)[:len(rays), :3]


def oracle_probe(arrays, rays, env_theta, num_bounces):
    pos, d = LC.frame(rays)
    acc = np.zeros(pos.shape, np.float32)
    fh = O.trace(arrays, pos.shape[1], pos.shape[0], pos, d, 0, RAND_BASE, env_theta, num_bounces, acc, first_hits=True)
    return acc.reshape(-1, 4)[:len(rays), :3], fh[:len(rays)]


def same_bits(got, want):
    """equal as the suite's parity tests compare (==, up to the sign of zero), NaN equal to NaN"""
    return np.array_equal(got, want, equal_nan=True)


# ---- 1, 2: the environment lookup ------------------------------------------------------------------------------------
_env_expected = {}


def env_expected(small_scene, name):
    """rays of map `name` (the finite directions, then those beyond the definition) and per env_theta the oracle's radiance
    and - finite thetas - the float64 reference of the finite directions; computed once per map"""
    if name not in _env_expected:
        w, h, env = LC.env_map(name)
        dirs, _, beyond = LC.env_dirs(w, h)
        arrays = LC.env_scene(small_scene, name)
        rays = LC.away_rays(arrays, np.concatenate([dirs, beyond]))
        want = {}
        for theta in LC.ENV_THETAS + LC.ENV_THETAS_HUGE:
            rgb, fh = oracle_probe(arrays, rays, theta, 0)
            assert (fh["index"] == -1).all()
            want[theta] = (rgb, LR.env_lookup(env, w, h, dirs, theta) if theta in LC.ENV_THETAS else None)
        _env_expected[name] = (rays, len(dirs), want)
    return _env_expected[name]


def check_environment(pt, small_scene, name):
    rays, n_finite, want = env_expected(small_scene, name)
    for theta, (bits, ref) in want.items():
        got = probe(pt, rays, theta)
        assert same_bits(got, bits), (name, theta, int((got != bits).any(-1).sum()))
        if ref is not None:
            dev = LC.deviation(got[:n_finite], ref)
            assert dev.max() <= LC.BOUND["env"], (name, theta, rays[dev.argmax(), 3:], dev.max())


def frame_height(n_rays):
    return max(1, -(-n_rays // LC.FRAME_W))


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(LC.ENV_MAPS))
def test_environment_lookup(small_scene, camera, name, config):
    arrays = LC.env_scene(small_scene, name)
    rays = env_expected(small_scene, name)[0]
    W, H = LC.FRAME_W, frame_height(len(rays))
    sc = Scene(arrays)
    pt = configure(PathTracer(sc, W, H, num_bounces=0), config)
    check_environment(pt, small_scene, name)
    # every frame above was an all-miss frame: the tracer is left usable - its next render is a fresh tracer's
    frames = []
    fresh = configure(PathTracer(sc, W, H, num_bounces=0), config)
    for t in (pt, fresh):
        t.num_bounces = 4
        t.set_camera(camera["P"], camera["I"], camera["fov_scale"], camera["env_theta"], camera["focal_depth"], camera["aperture"])
        t.clear()
        t.seed(5)
        t.render(2)
        frames.append(t.readRadiance())
    assert np.array_equal(frames[0], frames[1]) and frames[0][..., :3].max() > 0
    pt.close(); fresh.close(); sc.close()


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", ["13x5", "15x7"])
def test_environment_lookup_after_live_update(small_scene, name, source):
    """one size below and one above the tile grid, tiled by k_ap_env_tile (fspt_scene_update_environment) and, `device`,
    from a tensor on the device with the bins built there (fspt_scene_update_environment_device; the probe itself takes
    milliseconds - the first test of a session that touches torch also pays for its start)"""
    w, h, env = LC.env_map(name)
    rays = env_expected(small_scene, name)[0]
    pt = PathTracer(small_scene, LC.FRAME_W, frame_height(len(rays)), num_bounces=0)
    probe(pt, rays)                                  # the scene's own 64 x 32 map is in use before the update
    if source == "host":
        pt.update_environment(env, w, h, np.array([0, 0, w, h], np.uint32))
    else:
        import torch
        pt.update_environment(torch.from_numpy(env.copy()).to(f"cuda:{pt.scene.device}"), w, h)
    check_environment(pt, small_scene, name)
    pt.close()


# ---- 3: the emission probe -------------------------------------------------------------------------------------------
_material_expected = {}


def material_expected(res):
    """per emission quad: its rays, the oracle's radiance at num_bounces = 1 and the float64 30 * E * D"""
    if res not in _material_expected:
        arrays = LC.material_scene(res)
        out = {}
        for q in LC.EMISSION_QUADS:
            rays = LC.material_rays(res, LC.QUAD_NAMES.index(q))
            bits, fh = oracle_probe(arrays, rays, 0.0, 1)
            # a scene without an environment: the shadow and extension terms are exact zeros and the oracle's value is
            # finite on every ray (tests/test_lookup_cpu.py test_emission_oracle_matches_float64 holds it to that)
            assert np.isfinite(bits).all() and (fh["index"] // 2 == LC.QUAD_NAMES.index(q)).all()
            ref = LR.hit_surface(arrays, rays, fh["t"], fh["index"])
            out[q] = (rays, bits, 30.0 * ref["emissive"] * ref["diffuse"])
        _material_expected[res] = (arrays, out)
    return _material_expected[res]


def material_tracer(arrays, res, n_interleaved, W, H, num_bounces, pipeline="wavefront"):
    set_texture_interleave_budget(LC.budget(res, n_interleaved))
    try:
        pt = PathTracer(arrays, W, H, num_bounces=num_bounces)
    finally:
        set_texture_interleave_budget(DEFAULT_BUDGET)
    pt.set_pipeline(pipeline)
    return pt


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_emission_probe(res, pipeline):
    arrays, expected = material_expected(res)
    H = frame_height(len(expected["const"][0]))
    pt = material_tracer(arrays, res, 2, LC.FRAME_W, H, 1, pipeline)
    for q, (rays, bits, ref) in expected.items():
        got = probe(pt, rays)
        assert same_bits(got, bits), (q, int((got != bits).any(-1).sum()))
        dev = LC.deviation(got, ref)
        assert dev.max() <= LC.BOUND["emission"], (q, int(dev.argmax()), dev.max())
    pt.close()


def test_emission_probe_nonfinite_uvs():
    """vertex uvs of 3e9, NaN and +-inf in a QUAD and a SEPARATE set: the oracle's bits (texel (0, 0) of each layer)"""
    arrays, rays = LC.nonfinite_scene(), LC.nonfinite_rays()
    bits, fh = oracle_probe(arrays, rays, 0.0, 1)
    assert (fh["index"] >= 0).all()
    pt = material_tracer(arrays, LC.NONFINITE_RES, 2, LC.FRAME_W, frame_height(len(rays)), 1)
    assert same_bits(probe(pt, rays), bits)
    pt.close()


# ---- 4: the guides ---------------------------------------------------------------------------------------------------
_guides_expected = {}


def guides_expected(res):
    """the oracle's first-hit records of the camera's rays, hitref's decisive hits among them and the float64 surface there"""
    if res not in _guides_expected:
        arrays, (W, H), c = material_expected(res)[0], LC.CAMERA_FRAME, LC.CAMERA
        pos, d = O.camera(W, H, c["P"], c["I"], c["fov_scale"], S.lens_features(c["focal_depth"], c["aperture"]),
                          O.rand_base_stream(LC.CAMERA_SEED, 1)[0])
        acc = np.zeros((H, W, 4), np.float32)
        fh = O.trace(arrays, W, H, pos, d, 0, RAND_BASE, 0.0, 4, acc, first_hits=True)
        rays = np.concatenate([pos[..., :3], d[..., :3]], -1).reshape(-1, 6)
        cl = hitref.classify(arrays, rays)
        hit = np.flatnonzero(cl.kind == 1)
        first = [(cl.ties[i][0][0], cl.ties[i][1][0], cl.ties[i][2][0]) for i in hit]     # any triangle of the tie band: one surface
        index, t64, tau = (np.array(x) for x in zip(*first))
        assert set(index // 2) == set(range(len(LC.QUAD_NAMES))) and len(hit) > 200
        _guides_expected[res] = (fh.reshape(H, W), hit, t64, tau, LR.hit_surface(arrays, rays[hit], t64, index))
    return _guides_expected[res]


def read_guides(pt):
    c = LC.CAMERA
    pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])
    pt.features(1, LC.CAMERA_SEED)
    return pt.readFeatures()


@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_guides(res):
    arrays = material_expected(res)[0]
    fh, decisive, t64, tau, ref = guides_expected(res)
    W, H = LC.CAMERA_FRAME
    pt = material_tracer(arrays, res, 2, W, H, 4)
    got = read_guides(pt)
    hit = fh["index"] >= 0
    assert 0 < hit.sum() < W * H
    assert np.array_equal(got[..., 0:3][hit], fh["diffuse"][hit])
    assert np.array_equal(got[..., 4:7][hit], fh["macro_normal"][hit])
    assert np.array_equal(got[..., 3][hit], fh["t"][hit])
    assert np.array_equal(got[..., 7], hit.astype(np.float32))
    flat = got.reshape(-1, 8)[decisive]
    assert (flat[:, 7] == 1).all()
    assert LC.deviation(flat[:, 0:3], ref["diffuse"]).max() <= LC.BOUND["diffuse"]
    assert LC.deviation(flat[:, 4:7], ref["macro_normal"]).max() <= LC.BOUND["macro_normal"]
    assert (np.abs(flat[:, 3] - t64) <= tau).all()       # depth: hitref's own bound on a float32 distance
    pt.close()


# ---- 5: the interleaving budget --------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_interleave_budget_sweep(res):
    """none, one and all of the sets that can be interleaved stored as TEXSET_QUAD: the probes' output does not change by
    a bit (and is the oracle's)"""
    arrays, expected = material_expected(res)
    H = frame_height(len(expected["const"][0]))
    outputs = []
    for n in (0, 1, 3):
        pt = material_tracer(arrays, res, n, LC.FRAME_W, H, 1)
        out = [probe(pt, rays) for rays, _, _ in expected.values()]
        pt.close()
        pt = material_tracer(arrays, res, n, *LC.CAMERA_FRAME, 4)
        out.append(read_guides(pt))
        pt.close()
        outputs.append(out)
    for out in outputs[1:]:
        assert all(same_bits(a, b) for a, b in zip(out, outputs[0]))
    assert all(same_bits(a, bits) for a, (_, bits, _) in zip(outputs[0], expected.values()))
