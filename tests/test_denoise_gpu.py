"""The guided denoiser on the MI355X: the feature pass equals the oracle's first-hit records bit for bit (odd shapes, many
samples, a 63-deep tree, a GPU-built tree, the refractive scene), the a-trous kernel equals its float64 reference
(tests/atrous_ref.py) over a sweep of shapes, iteration counts and settings on inputs that reach every edge
(tests/atrous_inputs.py, through the fspt_denoise_eval hook), fspt_draw_denoised equals the oracle's draw.fs, the filter
earns its place on a real frame, and nothing it does touches the existing results."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import atrous_ref as R
from fspt_amd import PathTracer, _lib as L, scene as S
from fspt_amd.tracer import DENOISE_DEFAULTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNGUIDED = dict(sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf)


def make_pt(arrays, W, H, cam, aperture=None):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(cam["P"], cam["I"], cam["fov_scale"], cam["env_theta"], cam["focal_depth"],
                  cam["aperture"] if aperture is None else aperture)
    return pt


def oracle_first_hits(arrays, W, H, pt, rand_base):
    pos, d = O.camera(W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, rand_base)
    acc = np.zeros((H, W, 4), np.float32)
    return O.trace(arrays, W, H, pos, d, 0, 0.5, pt.envTheta, 4, acc, first_hits=True).reshape(H, W)


def feature_record(fh):
    """One sample's features from an oracle first-hit record (the miss values where index < 0)."""
    hit = fh["index"] >= 0
    f = np.zeros(fh.shape + (8,), np.float32)
    f[..., 0:3] = np.where(hit[..., None], fh["diffuse"], np.float32(1.0))
    f[..., 3] = np.where(hit, fh["t"], np.float32(100000.0))
    f[..., 4:7] = np.where(hit[..., None], fh["macro_normal"], np.float32(0.0))
    f[..., 7] = hit
    return f


def scenes(small):
    return {"small": small, "textured": S.textured_test_scene()}


@pytest.mark.parametrize("aperture", [None, 0.0])
@pytest.mark.parametrize("name", ["small", "textured"])
def test_features_one_sample_bitwise(small_scene, camera, name, aperture):
    arrays = scenes(small_scene)[name]
    W, H, seed = 96, 64, 11
    pt = make_pt(arrays, W, H, camera, aperture)
    pt.features(1, seed)
    got = pt.readFeatures()
    fh = oracle_first_hits(arrays, W, H, pt, O.rand_base_stream(seed, 1)[0])
    hit = fh["index"] >= 0
    assert 0 < hit.sum() < W * H  # hits and misses both present
    assert np.array_equal(got[..., 0:3][hit], fh["diffuse"][hit])
    assert np.array_equal(got[..., 4:7][hit], fh["macro_normal"][hit])
    assert np.array_equal(got[..., 3][hit], fh["t"][hit])
    assert np.array_equal(got[..., 7], hit.astype(np.float32))
    assert (got[~hit] == np.array([1, 1, 1, 100000, 0, 0, 0, 0], np.float32)).all()


@pytest.mark.parametrize("name", ["small", "textured"])
def test_features_eight_samples(small_scene, camera, name):
    """The float32 sums in sample order / 8 of the oracle's records: bit-exact (IEEE division, correctly rounded on
    both sides)."""
    arrays = scenes(small_scene)[name]
    W, H, seed, n = 80, 56, 5, 8
    pt = make_pt(arrays, W, H, camera)
    pt.features(n, seed)
    got = pt.readFeatures()
    acc = np.zeros((H, W, 8), np.float32)
    for rb in O.rand_base_stream(seed, n):
        acc = acc + feature_record(oracle_first_hits(arrays, W, H, pt, rb))
    want = acc / np.float32(n)
    assert np.array_equal(got, want)
    assert ((got[..., 7] > 0) & (got[..., 7] < 1)).any()  # some pixels have hit and missed samples (DoF, silhouettes)


def check_close(got, ref):
    big = np.abs(ref) > 1e-3
    rel = np.abs(got[big] - ref[big]) / np.abs(ref[big])
    assert rel.max() <= 1e-4, rel.max()
    assert np.abs(got[~big] - ref[~big]).max(initial=0.0) <= 1e-6


SETTINGS = [dict(), dict(iterations=1), dict(iterations=3), dict(iterations=5), dict(iterations=5, **UNGUIDED),
            dict(iterations=0)]


def test_filter_matches_reference(small_scene, camera):
    W, H = 120, 80
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(3)
    pt.render(16)
    pt.features(8, 9)
    acc, feat = pt.readRadiance(), pt.readFeatures()
    for kw in SETTINGS:
        got = pt.denoise(**kw)
        ref = R.atrous(acc, feat, **{**DENOISE_DEFAULTS, **kw})
        check_close(got, ref)
    assert np.array_equal(pt.denoise(iterations=0), acc)


def test_filter_on_bound_accumulator(small_scene, camera):
    import torch
    W, H = 100, 70
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt = make_pt(small_scene, W, H, camera)
    pt.bind_accumulator(t.data_ptr(), keep=t)
    pt.seed(4)
    pt.render(16)  # recorded into the tensor; fspt_denoise flushes first
    pt.features(8, 2)
    got = pt.denoise()
    acc = t.cpu().numpy()
    check_close(got, R.atrous(acc, pt.readFeatures(), **DENOISE_DEFAULTS))
    assert acc[..., :3].max() > 0


def test_draw_denoised_is_draw_of_the_denoised_frame(small_scene, camera):
    W, H = 96, 64
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(2)
    pt.render(8)
    pt.features(4, 3)
    den = pt.denoise(iterations=3)
    for ex, sat in ((1.0, 1.0), (2.5, 0.7)):
        assert np.array_equal(pt.drawDenoised(ex, sat), O.draw(den, ex, sat))


def test_existing_results_untouched_and_call_order(small_scene, camera):
    W, H = 96, 64
    pt = make_pt(small_scene, W, H, camera)
    # call order first: no features, no denoised frame yet
    lib = L.lib()
    buf = np.zeros((H, W, 8), np.float32)
    assert lib.fspt_read_features(pt._t, L.fptr(buf)) == -6
    assert lib.fspt_denoise(pt._t, None, None) == -6
    assert lib.fspt_draw_denoised(pt._t, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -6
    cp = L.CameraParams()
    assert lib.fspt_features(pt._t, C.byref(cp), 0, 1) == -1  # samples >= 1
    pt.seed(5)
    pt.render(6)
    before, drawn = pt.readRadiance(), pt.draw(1.3, 0.9, True, 2.0)
    pt.features(2, 7)
    for bad in (L.DenoiseParams(17, 1, 128, 0.1), L.DenoiseParams(5, -1, 128, 0.1), L.DenoiseParams(5, 1, -1, 0.1),
                L.DenoiseParams(5, 1, 128, 0.0), L.DenoiseParams(5, 1, np.inf, 0.1)):
        assert lib.fspt_denoise(pt._t, C.byref(bad), None) == -1
    assert lib.fspt_draw_denoised(pt._t, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -6
    assert lib.fspt_denoise(pt._t, None, None) == 0  # result kept on the device
    pt.drawDenoised()
    pt.denoise()
    assert pt.readRadiance().tobytes() == before.tobytes()
    assert pt.draw(1.3, 0.9, True, 2.0).tobytes() == drawn.tobytes()


# ---- quality -------------------------------------------------------------------------------------------------------
def rel_mse(x, gt, mask=None):
    e = (x[..., :3].astype(np.float64) - gt[..., :3]) ** 2 / (gt[..., :3].astype(np.float64) ** 2 + 1e-2)
    return float(e[mask].mean() if mask is not None else e.mean())


def silhouettes(depth):
    """Pixels whose 3x3 neighbourhood has a relative depth jump > 10 %."""
    H, W = depth.shape
    z = np.pad(depth, 1, mode="edge")
    jump = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            q = z[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            jump |= np.abs(q - depth) > 0.1 * depth
    return jump


def quality(arrays, cam, params, W=320, H=240, gt_spp=4096, spp=16, feature_samples=8):
    pt = make_pt(arrays, W, H, cam)
    pt.seed(101)
    pt.render(gt_spp)
    gt = pt.readRadiance()
    pt.features(feature_samples, 1)
    mask = silhouettes(pt.readFeatures()[..., 3])
    pt.clear()
    pt.seed(7)
    pt.render(spp)
    raw = pt.readRadiance()
    out = {"raw": rel_mse(raw, gt), "edge_pixels": int(mask.sum())}
    for name, kw in params.items():
        den = pt.denoise(**kw)
        out[name] = rel_mse(den, gt)
        out[name + "_edge"] = rel_mse(den, gt, mask)
    pt.close()
    return out


def test_quality(medium_scene, camera):
    """320 x 240 of the medium scene, 16 spp against 4096 spp, relative MSE (error^2 / (reference^2 + 0.01)).  Measured on
    the MI355X with the shipped defaults (K 4, sigma_color 4, sigma_normal 32, sigma_depth 0.05): denoised / raw = 0.0077
    (raw 0.147); on the 965 silhouette pixels guided / unguided blur (K 4) = 0.060.  The thresholds keep a margin of 3-6x."""
    q = quality(medium_scene, camera, {"guided": dict(), "unguided": dict(iterations=4, **UNGUIDED)})
    print("quality", q)
    assert q["edge_pixels"] > 100
    assert q["guided"] <= 0.05 * q["raw"], q
    assert q["guided_edge"] <= 0.2 * q["unguided_edge"], q


# ---- the Node host ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "fspt_amd", "js", "fspt_napi.node")),
                    reason="node or the built addon is missing")
def test_node_host_matches_python_host(small_scene, camera, tmp_path):
    """fspt.js features / denoise / drawDenoised give the Python host's bytes; while a renderAsync job is in flight the
    three throw Error('render in flight')."""
    import base64
    import json
    W, H, seed, ticks, samples, fseed = 96, 64, 13, 6, 4, 3
    env, ew, eh = S.synthetic_env(64, 32)
    job = {"props": S.bunny_props(), "objs": {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ},
           "env": {"rgbe_b64": base64.b64encode(env.tobytes()).decode(), "width": ew, "height": eh},
           "W": W, "H": H, "bounces": 4, "seed": seed, "ticks": ticks, "samples": samples, "feature_seed": fseed,
           "cam": dict(P=camera["P"], I=camera["I"], fov_scale=camera["fov_scale"], env_theta=camera["env_theta"], lens=camera["lens"])}
    jp, op = tmp_path / "job.json", tmp_path / "out.json"
    jp.write_text(json.dumps(job))
    subprocess.check_call(["node", os.path.join(ROOT, "tests", "denoise_node_check.js"), str(jp), str(op)], timeout=300)
    out = json.loads(op.read_text())
    dec = lambda k: base64.b64decode(out[k])
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(seed)
    pt.render(ticks)
    pt.features(samples, fseed)
    assert dec("denoised") == pt.denoise().tobytes()
    assert dec("denoised_k2") == pt.denoise(iterations=2, sigma_color=2.0).tobytes()
    assert dec("drawn") == pt.drawDenoised(1.5, 0.8).tobytes()
    assert out["during"] == {"features": "render in flight", "denoise": "render in flight", "drawDenoised": "render in flight"}
    assert out["after"] is None


# ---- k_atrous through fspt_denoise_eval against the float64 reference, on inputs that reach every edge -------------------
import atrous_inputs as I  # noqa: E402
from fspt_amd import denoise_eval  # noqa: E402

SHAPES = [(1, 1), (1, 37), (53, 1), (15, 17), (16, 16), (17, 16), (255, 3), (120, 80)]  # (W, H)
ITERATIONS = [0, 1, 2, 4, 7, 10, 16]
U32 = 2.0 ** -24  # float32 unit roundoff
TINY = float(np.finfo(np.float32).smallest_subnormal)


def check_bound(got, ref, rtol=1e-4):
    """check_close's bound (1e-4 relative where |ref| > 1e-3, 1e-6 absolute elsewhere), widened by rtol - 1e-4 relative
    when rtol is wider; and the kernel's output finite."""
    assert np.isfinite(got).all(), f"{(~np.isfinite(got)).sum()} non-finite values"
    big = np.abs(ref) > 1e-3
    rel = np.abs(got[big] - ref[big]) / np.abs(ref[big])
    assert rel.max(initial=0.0) <= rtol, (rel.max(), rtol)
    small = np.abs(got[~big] - ref[~big])
    assert (small <= 1e-6 + (rtol - 1e-4) * np.abs(ref[~big])).all(), small.max()


def sweep(acc, f, rtol=1e-4, **kw):
    got = denoise_eval(acc, f, **kw)
    ref = R.atrous(acc, f, **{**DENOISE_DEFAULTS, **kw})
    check_bound(got, ref, rtol)
    return got


@pytest.mark.parametrize("W,H", SHAPES)
def test_atrous_shapes_and_iterations(W, H):
    """Every shape (single pixels, single rows and columns, partial 16 x 16 blocks) at every iteration count: from K = 5 on
    (step 16 and more) the taps of most pixels, and at 1 x 1 all but the centre, fall outside the frame."""
    acc, f = I.synthetic(H, W)
    for k in ITERATIONS:
        got = sweep(acc, f, iterations=k)
        if k == 0:
            assert np.array_equal(got, acc)


WEIGHTS = {"colour only": dict(sigma_normal=0.0, sigma_depth=np.inf), "normal only": dict(sigma_color=np.inf, sigma_depth=np.inf),
           "depth only": dict(sigma_color=np.inf, sigma_normal=0.0), "plain B3": UNGUIDED}


@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_atrous_weights_one_at_a_time(weights):
    for W, H in ((120, 80), (17, 16)):
        acc, f = I.synthetic(H, W)
        for k in (1, 2, 4, 7):
            sweep(acc, f, iterations=k, **WEIGHTS[weights])


def check_in_hull(got, acc, f):
    """Per channel, out / albedo lies within the range of the demodulated accumulator (a normalised sum of non-negative
    weights); and the output is finite."""
    assert np.isfinite(got).all()
    a = f[..., 0:3].astype(np.float64)
    u0 = acc[..., :3] / np.maximum(a, 1e-3)
    lo, hi = u0.min((0, 1)), u0.max((0, 1))
    assert (got[..., :3] >= a * lo * (1 - 1e-5)).all() and (got[..., :3] <= a * hi * (1 + 1e-5)).all()
    assert (got[..., 3] == 1).all()


def check_sigma_color_zero(acc, f):
    """sigma_color = 0: wc = exp(-|L_p - L_q| / 1e-4).  The kernel's lumas are float32 values of float32 u = c / max(a,
    1e-3): the division, three products and two sums and the subtraction put |L_p - L_q| off by at most 6u (L_p + L_q)
    (u = 2^-24), and 1 / 1e-4 turns that into an exponent off by 6u (L_p + L_q) 1e4 - an ill-conditioned weight that no
    float32 kernel keeps within 1e-4 (6e-4 measured at L ~ 1).  With every pixel whose L(u0) exceeds 1 scaled down to 1,
    one iteration's weights are off by a factor of at most e^(12u 1e4) = 1 + d, and the output (a normalised sum of
    non-negative terms) by at most (1+d)^2 - 1 on top of the 1e-4; later iterations feed those errors back into the
    weights (no bound to derive): finite and inside the input's range."""
    a = np.maximum(f[..., 0:3].astype(np.float64), 1e-3)
    acc = acc.copy()
    scale = np.minimum(1.0, 0.999 / np.maximum(R.luma(acc[..., :3] / a), 1e-30))
    acc[..., :3] = (acc[..., :3] * scale[..., None]).astype(np.float32)
    assert R.luma(acc[..., :3] / a).max() <= 1
    sweep(acc, f, float(np.expm1(2 * 12 * U32 * 1e4)) + 1e-4, iterations=1, sigma_color=0.0)
    for k in (2, 4, 7):
        check_in_hull(denoise_eval(acc, f, iterations=k, sigma_color=0.0), acc, f)


def test_atrous_sigma_color_zero():
    for W, H in ((120, 80), (17, 16)):
        check_sigma_color_zero(*I.synthetic(H, W))


def sigma_normal_rtol(sn, k):
    """The bound for sigma_normal > 128.  k_atrous rounds the cosine c = n_p.n_q / (|n_p||n_q|) in float32: the dot
    product (two fma on one product) carries an absolute error <= 3u |n_p||n_q| (u = 2^-24), each length 2.5u relative
    (three terms, the square root), their product one more u, the division one more: |c_f32 - c| <= 10u.  Clamped to 1,
    an equal pair weighs exactly 1 on both sides; for c >= 1/2, ln(c_f32 / c) <= 20u and the weight c^sn is off by a
    factor of at most e^(20 u sn) = 1 + d; a pair with c < 1/2 weighs < 2^-128 on both sides, below float32's resolution
    of the centre tap's weight.  With sigma_color = +inf the weights do not depend on u, every u is >= 0 (the accumulator
    is), and a normalised sum of non-negative terms whose weights are off by factors in [1/(1+d), 1+d] is off by a factor
    within (1+d)^2 - so k iterations are off by at most (1+d)^(2k) - 1, on top of the 1e-4 the float32 arithmetic keeps
    at sigma_normal <= 128.  At sigma_normal = 4096 this is 5e-3 per weight; at 1e9 it is unbounded (inf)."""
    with np.errstate(over="ignore"):
        return float(np.expm1(2 * k * 20 * U32 * sn)) + 1e-4


@pytest.mark.parametrize("sigma_normal", [1.0, 32.0, 128.0, 4096.0, 1e9])
def test_atrous_sigma_normal(sigma_normal):
    """sigma_normal up to 128: every setting within 1e-4.  Above: sigma_color off and the bound sigma_normal_rtol derives;
    where that bound is unbounded the output must still be finite and, per channel, a convex combination of the
    demodulated inputs times the pixel's albedo.  Finite output at the defaults otherwise, for every sigma_normal."""
    acc, f = I.synthetic(80, 120)
    for k in (1, 2, 4, 16):
        if sigma_normal <= 128:
            sweep(acc, f, iterations=k, sigma_normal=sigma_normal)
            continue
        got = denoise_eval(acc, f, iterations=k, sigma_normal=sigma_normal)
        assert np.isfinite(got).all(), (k, (~np.isfinite(got)).sum())
        rtol = sigma_normal_rtol(sigma_normal, k)
        if np.isfinite(rtol):
            got = sweep(acc, f, rtol, iterations=k, sigma_normal=sigma_normal, sigma_color=np.inf)
        else:
            check_in_hull(denoise_eval(acc, f, iterations=k, sigma_normal=sigma_normal, sigma_color=np.inf), acc, f)


@pytest.mark.parametrize("sigma_depth", [1e-6, 0.05, 1e3, TINY])
def test_atrous_sigma_depth(sigma_depth):
    """Down to the smallest positive float32, whose scaled denominator sigma_depth 2^k max(z_p, 1e-3) underflows to 0 in
    float32: the centre tap (and every tap at the same depth) still weighs 1."""
    acc, f = I.synthetic(80, 120)
    for k in (1, 2, 4, 16):
        sweep(acc, f, iterations=k, sigma_depth=sigma_depth)
        sweep(acc, f, iterations=k, sigma_depth=sigma_depth, sigma_color=np.inf, sigma_normal=0.0)


def test_atrous_full_hd_defaults():
    """One 1920 x 1080 frame at the defaults.  K iterations reach 2 (2^K - 1) pixels (30 at K = 4), so the reference of a
    window grown by that much on every side that is not the frame's edge is exact on the window: five windows (the four
    corners and the centre) stand in for the whole frame, whose reference takes most of a minute in numpy."""
    H, W, k = 1080, 1920, DENOISE_DEFAULTS["iterations"]
    acc, f = I.synthetic(H, W)
    got = denoise_eval(acc, f)
    assert np.isfinite(got).all()
    r = 2 * (2 ** k - 1)
    for y0, x0 in ((0, 0), (0, W - 96), (H - 96, 0), (H - 96, W - 96), (H // 2 - 48, W // 2 - 48)):
        y1, x1 = y0 + 96, x0 + 96
        ey0, ex0, ey1, ex1 = max(0, y0 - r), max(0, x0 - r), min(H, y1 + r), min(W, x1 + r)
        ref = R.atrous(acc[ey0:ey1, ex0:ex1], f[ey0:ey1, ex0:ex1], **DENOISE_DEFAULTS)
        check_bound(got[y0:y1, x0:x1], ref[y0 - ey0:y1 - ey0, x0 - ex0:x1 - ex0])


def test_denoise_eval_is_fspt_denoise(small_scene, camera):
    """The hook runs the code that ships: on a target's own accumulator and features it gives fspt_denoise's bytes, and
    it refuses what fspt_denoise refuses, with the same code."""
    W, H = 61, 37
    pt = make_pt(small_scene, W, H, camera)
    pt.seed(6)
    pt.render(4)
    pt.features(3, 2)
    acc, feat = pt.readRadiance(), pt.readFeatures()
    for kw in (dict(), dict(iterations=0), dict(iterations=1), dict(iterations=16, sigma_normal=1e9, sigma_depth=TINY),
               dict(sigma_color=0.0), dict(iterations=3, **UNGUIDED)):
        assert np.array_equal(denoise_eval(acc, feat, **kw), pt.denoise(**kw)), kw
    lib = L.lib()
    out = np.zeros((H, W, 4), np.float32)
    for bad in (L.DenoiseParams(17, 1, 128, 0.1), L.DenoiseParams(5, -1, 128, 0.1), L.DenoiseParams(5, 1, -1, 0.1),
                L.DenoiseParams(5, 1, 128, 0.0), L.DenoiseParams(5, 1, np.inf, 0.1), L.DenoiseParams(5, np.nan, 1, 0.1),
                L.DenoiseParams(5, 1, np.nan, 0.1), L.DenoiseParams(5, 1, 1, np.nan)):
        assert lib.fspt_denoise_eval(0, L.fptr(acc), L.fptr(feat), W, H, C.byref(bad), L.fptr(out)) == -1
        assert lib.fspt_denoise(pt._t, C.byref(bad), None) == -1
    assert lib.fspt_denoise_eval(1 << 20, L.fptr(acc), L.fptr(feat), W, H, None, L.fptr(out)) == -1  # no such device
    assert lib.fspt_denoise_eval(0, L.fptr(acc), L.fptr(feat), 0, 5, None, L.fptr(out)) == 0  # an empty frame: nothing to do
    pt.close()


@pytest.mark.parametrize("name", ["medium", "textured"])
def test_atrous_sweep_on_real_scenes(medium_scene, camera, name):
    """The real features of the medium and textured scenes (seams, silhouettes, textures) through the same sweep."""
    arrays = medium_scene if name == "medium" else S.textured_test_scene()
    W, H = 120, 80
    pt = make_pt(arrays, W, H, camera)
    pt.seed(3)
    pt.render(8)
    pt.features(8, 9)
    acc, feat = pt.readRadiance(), pt.readFeatures()
    pt.close()
    assert ((feat[..., 7] > 0) & (feat[..., 7] < 1)).any() and (feat[..., 7] == 0).any()
    check_sigma_color_zero(acc, feat)
    for kw in (dict(), dict(iterations=16), dict(sigma_normal=128.0),
               dict(sigma_depth=TINY), dict(sigma_depth=1e3), dict(iterations=7, **UNGUIDED)):
        sweep(acc, feat, **kw)
    for k in (1, 4):
        sweep(acc, feat, sigma_normal_rtol(4096.0, k), iterations=k, sigma_normal=4096.0, sigma_color=np.inf)
    assert np.isfinite(denoise_eval(acc, feat, sigma_normal=1e9)).all()


# ---- k_features on the traversal edge cases, bit-exact against the oracle ----------------------------------------------
def oracle_features(arrays, W, H, pt, seed, n):
    """The float32 sums in sample order / n of the oracle's first-hit records (n = 1: the record itself)."""
    acc = np.zeros((H, W, 8), np.float32)
    for rb in O.rand_base_stream(seed, n):
        acc = acc + feature_record(oracle_first_hits(arrays, W, H, pt, rb))
    return acc / np.float32(n)


CHAIN_CAMERA = dict(P=[64 + 2.5, 0.05, 0.1], I=[-1.0, -0.01, -0.02], fov_scale=0.5, env_theta=1.66, focal_depth=2.0, aperture=0.02)
VARIANT_CAMERA = dict(P=[0.3, 1.2, 3.4], I=[-0.05, -0.3, -0.95], fov_scale=0.5, env_theta=1.66, focal_depth=2.0, aperture=0.02)


@pytest.mark.parametrize("W,H", SHAPES)
def test_features_odd_shapes(small_scene, camera, W, H):
    pt = make_pt(small_scene, W, H, camera)
    pt.features(3, 4)
    assert np.array_equal(pt.readFeatures(), oracle_features(small_scene, W, H, pt, 4, 3))
    if (W, H) in ((15, 17), (255, 3)):  # and drawDenoised on them
        pt.seed(2)
        pt.render(4)
        den = pt.denoise(iterations=3)
        for ex, sat in ((1.0, 1.0), (2.5, 0.7)):
            assert np.array_equal(pt.drawDenoised(ex, sat), O.draw(den, ex, sat))
    pt.close()


@pytest.mark.parametrize("case", ["64 samples", "chain depth 63", "gpu-built tree", "refractive"])
def test_features_edge_trees(small_scene, camera, case):
    """64 samples per pixel; the 63-deep chain (the LDS opt-in of launch_features: 8 waves x 64 stack entries); a tree
    built by the GPU builder; the refractive golden scene (features stop at the first hit: the glass's own albedo)."""
    from rays import chain_scene
    from test_goldens import scene_from_golden
    W, H, n, arrays, cam = 15, 17, 64, small_scene, camera
    if case == "chain depth 63":
        W, H, n, arrays, cam = 72, 40, 3, chain_scene(64, small_scene), CHAIN_CAMERA
    elif case == "gpu-built tree":
        W, H, n, arrays = 53, 29, 3, S.bunny_scene(n=8, env_size=(64, 32), bvh="gpu")
    elif case == "refractive":
        W, H, n, arrays, cam = 72, 40, 3, scene_from_golden("variant"), VARIANT_CAMERA
    pt = make_pt(arrays, W, H, cam)
    pt.features(n, 8)
    got = pt.readFeatures()
    assert np.array_equal(got, oracle_features(arrays, W, H, pt, 8, n))
    assert (got[..., 7] > 0).any()
    pt.close()
