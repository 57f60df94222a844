"""Emitter next-event estimation in the oracle, checked without a device: one q > 0 vertex against the float64
restatement of 8.3's formulas (tests/lights_ref.py), the MIS weights of the two strategies summing to one for the same
direction, the reductions to the mode-off bits, the oracle's light weights and emitter sample against the restatement,
and scene E3's light table and sample range."""
import numpy as np
import pytest

import lights_ref as R
import oracle as O
from fspt_amd import scene as S

CAM = S.BUNNY_CAMERA
LENS = S.lens_features(CAM["focal_depth"], CAM["aperture"])


@pytest.fixture(scope="module")
def e1():
    return R.scene_e1()


@pytest.fixture(scope="module")
def e3():
    return R.scene_e3()


def render(arrays, W, H, nb, n, seed, lights=None, first_tick=0, acc=None):
    acc = np.zeros((H, W, 4), np.float32) if acc is None else acc
    O.render(arrays, W, H, CAM["P"], CAM["I"], CAM["fov_scale"], LENS, CAM["env_theta"], nb, first_tick, n, seed, acc,
             lights=lights)
    return acc


def camera_hits(arrays, W, H, rand_base=321.5):
    pos, d = O.camera(W, H, CAM["P"], CAM["I"], CAM["fov_scale"], LENS, rand_base)
    rays = np.concatenate([pos.reshape(-1, 4)[:, :3], d.reshape(-1, 4)[:, :3]], 1)
    t, idx, _, _ = O.intersect(arrays, rays)
    ok = idx >= 0
    return rays[ok], t[ok], idx[ok]


# ---- the vertex against the float64 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["e1", "e3"])
@pytest.mark.parametrize("bounce,nb", [(0, 4), (2, 4), (3, 4), (0, 1)])
def test_vertex_matches_float64(request, scene, bounce, nb):
    arrays = request.getfixturevalue(scene)
    table = R.host_table(arrays)
    q = R.env_q(arrays, 0.5)
    rays, t, idx = camera_hits(arrays, 160, 120)
    rec = np.random.default_rng(bounce + 10 * nb).random((rays.shape[0], 12), dtype=np.float32)
    v = O.light_vertex_probe(arrays, (table, q), rays, t, idx, rec=rec, bounce=bounce, num_bounces=nb)
    want_q = R.q_rule(v, q, bounce, nb).astype(np.float32)
    assert np.array_equal(v["q"], want_q)
    live = v["q"] > 0
    if nb == 1 or bounce + 1 >= nb:
        assert not live.any()
        return
    assert live.sum() > 1000
    # the branch decisions: q = 0 draws nothing more; u0 picks the strategy; u0..u3 follow the vertex's own draws
    assert (v["strategy"][~live] == 0).all()
    assert np.array_equal(v["strategy"][live], np.where(v["u"][live, 0] < q, 2, 1))
    used = v["used"].astype(int)
    assert (used[live] == np.where(v["specular"][live] > 0, 10, 12)).all()
    rows = np.flatnonzero(live)
    assert np.array_equal(v["u"][live], rec[rows[:, None], used[live][:, None] - 4 + np.arange(4)])
    # the environment strategy: the reference's contribution / (1 - q), weight 1, unbounded shadow ray
    env = v["strategy"] == 1
    assert (v["wx"][env] == 1).all() and (v["lt"][env] == np.float32(1e5)).all()
    em = v["strategy"] == 2
    assert em.sum() > 500
    lq = np.where(v["bsdf_pdf"] > 0, q / v["bsdf_pdf"].astype(np.float64), 0)
    assert np.allclose(v["lq"][live], lq[live], rtol=1e-6)
    sel = {k: x[em] for k, x in v.items()}
    r = R.emitter_vertex(arrays, table, q, sel)
    assert np.array_equal(sel["entry"].astype(int), r["entry"])
    assert np.array_equal(sel["tri"].astype(int), r["tri"])
    assert np.allclose(sel["x"], r["x"], rtol=1e-5, atol=1e-6)
    # away from grazing views of the emitter or the surface the float32 path keeps 1e-4
    ok = (r["cos_l"] > 0.05) & (np.abs(r["cn"]) > 0.05)
    assert ok.sum() > 200
    for k in ("pdf_L", "pdf_B", "w_L", "lt"):
        assert np.allclose(sel[k][ok], r[k][ok], rtol=1e-4, atol=0), (k, np.abs(sel[k][ok] / r[k][ok] - 1).max())
    lit = ok & (r["cn"] > 0)
    assert np.allclose(sel["pend"][lit], r["contrib"][lit], rtol=1e-4, atol=1e-7)
    shadow = (r["cn"] > 0) & (r["pdf_L"] > 0)
    assert np.array_equal(sel["has_shadow"] > 0, shadow)


# ---- the tracer's own random numbers realise the table ----------------------------------------------------------------
def test_rnd_draws_realise_light_p(e3):
    """Emitter entries picked at E3's camera hits with the tracer's rnd() (no replayed values), over many rand_base values,
    against light_p: rnd() is as coarse as 2^-8, and an alias slot + coin read from one draw alone misses the table (the
    lamp 1-10 % too rarely, the faintest entries ~270x too often)."""
    table = R.host_table(e3)
    q = R.env_q(e3, 0.5)
    rays, t, idx = camera_hits(e3, 160, 120)
    n = table["tris"].size
    cnt = np.zeros(n)
    for rb in np.linspace(17.0, 9000.0, 128):
        v = O.light_vertex_probe(e3, (table, q), rays, t, idx, rec=None, rand_base=float(rb), bounce=0, num_bounces=4)
        cnt += np.bincount(v["entry"][v["strategy"] == 2].astype(int), minlength=n)
    N = cnt.sum()
    assert N > 2e5
    exp = table["light_p"].astype(np.float64) * N
    big = exp > 50
    chi2, dof = float((((cnt - exp) ** 2) / exp)[big].sum()), int(big.sum()) - 1
    print("E3 rnd() entries: %d samples, chi2 %.1f over %d dof; faint entries %d for %.1f expected" %
          (N, chi2, dof, cnt[~big].sum(), exp[~big].sum()))
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof)
    heavy = exp > 5000
    assert np.allclose(cnt[heavy], exp[heavy], rtol=0.06)
    assert cnt[~big].sum() <= 2.0 * exp[~big].sum() + 10


# ---- the two strategies' weights sum to one for the same direction -------------------------------------------------------
def identity_scene(metallic, rough, height):
    """A 4 x 4 floor of the given metallic / roughness under a 0.5 x 0.5 lamp at `height` (tilted 30 degrees)."""
    props = [
        {"path": "synthetic/quad.obj", "scale": 4, "rotate": [{"angle": 3.1415927, "axis": [1, 0, 0]}],  # (normal +y)
         "translate": [0, 0, 0], "emittance": [0, 0, 0],
         "diffuse": [0.7, 0.6, 0.5], "metallicRoughness": [metallic, rough, 0], "normals": "flat"},
        {"path": "synthetic/lamp.obj", "scale": 0.5, "rotate": [{"angle": 2.6179938, "axis": [1, 0, 0]}],
         "translate": [0.3, height, -0.2], "emittance": [1, 1, 1], "normals": "flat"},
    ]
    texts = {"synthetic/quad.obj": S.QUAD_OBJ, "synthetic/lamp.obj": R.LAMP_OBJ}
    return S.build_scene(props, texts, mtl_texts={"synthetic/lamp.mtl": R.LAMP_MTL})


@pytest.mark.parametrize("metallic,rough", [(0, 0.5), (1, 0.05), (1, 0.3), (1, 1.0)])
@pytest.mark.parametrize("height", [0.05, 0.4, 6.0])
def test_weights_sum_to_one(metallic, rough, height):
    arrays = identity_scene(metallic, rough, height)
    table = R.host_table(arrays)
    n = 1 << 14
    rng = np.random.default_rng(int(height * 100) + int(rough * 10))
    # rays from above onto the floor, at all angles
    tgt = np.stack([rng.uniform(-1.5, 1.5, n), np.zeros(n), rng.uniform(-1.5, 1.5, n)], 1)
    d = rng.normal(size=(n, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.05
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([tgt - d * 2.0, d], 1).astype(np.float32)
    t, idx, _, _ = O.intersect(arrays, rays)
    floor = (idx >= 0) & (table["light_p"].size > 0) & ~np.isin(idx, table["tris"])
    rays, t, idx = rays[floor], t[floor], idx[floor]
    rec = rng.random((rays.shape[0], 12), dtype=np.float32)
    v = O.light_vertex_probe(arrays, (table, 1.0), rays, t, idx, rec=rec, bounce=0, num_bounces=4)
    assert (v["inside"] == 0).all()
    # no environment map: q = 1 and every vertex with q > 0 (not on a non-metal's specular lobe) samples an emitter
    assert np.array_equal(v["strategy"] == 2, (v["specular"] == 0) | (metallic == 1))
    assert (v["specular"] > 0).all() if metallic == 1 else (v["specular"] == 0).mean() > 0.5
    # the BSDF ray along the sampled direction from the same origin
    ok = (v["has_shadow"] > 0) & (v["specular"] == (1 if metallic == 1 else 0)) & (v["pdf_B"] > 0)
    shadow = np.concatenate([v["ro"], v["dir"]], 1)[ok]
    st, sidx, _, _ = O.intersect(arrays, shadow)
    hit = sidx == v["tri"][ok].astype(np.int32)
    assert hit.mean() > 0.99  # (nothing occludes the lamp here)
    lq = (np.float32(1.0) / v["pdf_B"][ok]).astype(np.float32)
    emw = O.emission_weight_probe(arrays, (table, 1.0), lq[hit], v["dir"][ok][hit], st[hit], sidx[hit])
    w_L = v["w_L"][ok][hit]
    assert np.isfinite(emw).all() and (emw >= 0).all() and (emw <= 1).all()
    # away from edge-on views (the solid-angle pdf is ill-conditioned there)
    tri = v["tri"][ok][hit].astype(int)
    _, e1, e2 = R.tri_geometry(arrays)
    ng = np.cross(e1[tri], e2[tri])
    cos_l = np.abs((ng * v["dir"][ok][hit]).sum(1)) / np.linalg.norm(ng, axis=1)
    good = cos_l > 0.05
    assert good.sum() > 1000
    err = np.abs(w_L[good].astype(np.float64) + emw[good] - 1.0)
    assert err.max() <= 1e-5, err.max()
    # near the lamp both strategies matter (far from it, w_L -> 1: the emitter is a point to the BSDF)
    assert ((w_L > 0.05) & (w_L < 0.95)).any() or height > 1


# ---- reductions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["e1", "e3"])
def test_empty_table_and_one_bounce_are_mode_off(request, scene):
    arrays = request.getfixturevalue(scene)
    W, H = 64, 48
    empty = {"tris": np.zeros(0, np.uint32), "prob": np.zeros(0, np.float32), "alias": np.zeros(0, np.uint32)}
    for nb in (1, 4, 70):
        off = render(arrays, W, H, nb, 3, 7)
        assert np.array_equal(render(arrays, W, H, nb, 3, 7, lights=(empty, 0.5)), off), nb
        on = render(arrays, W, H, nb, 3, 7, lights=(R.host_table(arrays), R.env_q(arrays, 0.5)))
        assert np.array_equal(on, off) == (nb == 1), nb


def test_path_replay_lights_off_unchanged(e3):
    W, H = 32, 24
    pos, d = O.camera(W, H, CAM["P"], CAM["I"], CAM["fov_scale"], LENS, 77.0)
    rec = np.random.default_rng(3).random((W * H, 600), dtype=np.float32)
    cnt = np.full(W * H, 600, np.uint32)
    a = O.path_replay(e3, pos, d, rec, cnt, 1.0, CAM["env_theta"], 1)
    b = O.path_replay(e3, pos, d, rec, cnt, 1.0, CAM["env_theta"], 1, lights=(R.host_table(e3), 0.5))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = O.path_replay(e3, pos, d, rec, cnt, 1.0, CAM["env_theta"], 4, lights=(R.host_table(e3), 0.5))
    assert not np.array_equal(c[0], O.path_replay(e3, pos, d, rec, cnt, 1.0, CAM["env_theta"], 4)[0])


# ---- the oracle's table weights and emitter sample against the restatement -------------------------------------------------
@pytest.mark.parametrize("scene", ["e1", "e3"])
def test_light_weights_and_sample(request, scene):
    arrays = request.getfixturevalue(scene)
    T = arrays.tri.size // 9
    w = O.light_weights(arrays, np.arange(T))
    assert np.allclose(w, R.flat_weights(arrays), rtol=1e-5, atol=0)
    table = R.host_table(arrays)
    rng = np.random.default_rng(9)
    n = 1 << 14
    qs = np.zeros((n, 10), np.float32)
    qs[:, 0:3] = rng.uniform([-1.5, -0.7, -0.9], [1.5, 0.3, 1.0], (n, 3))
    nv = rng.normal(size=(n, 3)); qs[:, 3:6] = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    qs[:, 6:10] = rng.random((n, 4), dtype=np.float32)
    tri, out = O.light_sample(arrays, table, qs)
    rtri, x, pdf, le, cn = R.sample(arrays, table, qs)
    assert np.array_equal(tri, rtri)
    assert np.allclose(out[:, 0:3], x, rtol=1e-5, atol=1e-5)
    ok = pdf < 1e6
    assert np.allclose(out[ok, 3], pdf[ok], rtol=1e-4)
    assert np.allclose(out[:, 4:7], le, rtol=1e-6)
    assert np.allclose(out[:, 7], cn, atol=1e-5)


# ---- E3 ----------------------------------------------------------------------------------------------------------------
def test_e3_table_moves_mass(e3):
    table = R.host_table(e3)
    w = R.flat_weights(e3)[table["tris"]]
    n = table["tris"].size
    assert 36 <= n <= 44
    assert np.log10(w.max() / w.min()) >= 4.0
    assert (table["alias"] != np.arange(n)).sum() >= n // 2
    assert np.allclose(table["light_p"], w / w.sum(), rtol=1e-5)
    assert e3.env is not None and R.env_q(e3, 1.0) == 0.875


@pytest.mark.parametrize("nb", [2, 4, 8])
def test_e3_clamp_never_binds(e3, nb):
    """Le x albedo stays low enough that no sample reaches the 1024 clamp, with the mode on at every fraction."""
    W, H = 96, 64
    top = 0.0
    for f in (0.25, 0.5, 1.0):
        for tick in range(4):
            acc = render(e3, W, H, nb, 1, 1000 + tick, lights=(R.host_table(e3), R.env_q(e3, f)))
            top = max(top, float(acc[..., :3].max()))
    print("E3 nb %d: largest sample %.1f" % (nb, top))
    assert top < 512.0
