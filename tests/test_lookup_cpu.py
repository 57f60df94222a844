"""The oracle's lookups against the float64 reference (tests/lookup_ref.py) on the committed cases (tests/lookup_cases.py):
the environment fetch through oracle.trace at num_bounces = 0, the hit record and the four material layers through its
first-hit records, the emission product at num_bounces = 1.  The tolerances of lookup_cases are measured here, every
mutant of the reference is shown to be rejected by them, and the coverage the cases claim is asserted from the float64
footprint indices.  No GPU."""
import functools

import numpy as np
import pytest

import hitref
import lookup_cases as LC
import lookup_ref as LR
import oracle as O
from appearance_cases import TEXSET_CONST, TEXSET_QUAD, TEXSET_SEPARATE

SURFACE_KEYS = ("uv", "bary", "diffuse", "emissive", "mr", "tex_normal", "bary_normal", "macro_normal")


def oracle_trace(arrays, rays, env_theta, num_bounces, first_hits=False):
    pos, d = LC.frame(rays)
    H = pos.shape[0]
    acc = np.zeros((H, LC.FRAME_W, 4), np.float32)
    fh = O.trace(arrays, LC.FRAME_W, H, pos, d, 0, 0.5, env_theta, num_bounces, acc, first_hits=True)
    n = len(rays)
    assert (fh["index"][n:] == -1).all()          # the padding rays miss
    return acc.reshape(-1, 4)[:n, :3], fh[:n]


class Cases:
    """Every oracle result and reference value the tests below share, computed once."""

    def __init__(self, small_scene):
        self.small = small_scene

    @functools.lru_cache(None)
    def env(self, name):
        """-> w, h, bytes, finite dirs, their texel centres, {theta: oracle rgb of finite dirs}, {theta: oracle rgb of
        the dirs beyond the definition}"""
        w, h, env = LC.env_map(name)
        dirs, centre, beyond = LC.env_dirs(w, h)
        arrays = LC.env_scene(self.small, name)
        got, got_beyond = {}, {}
        for theta in LC.ENV_THETAS:
            rgb, fh = oracle_trace(arrays, LC.away_rays(arrays, np.concatenate([dirs, beyond])), theta, 0)
            assert (fh["index"] == -1).all()      # placement: every ray misses the scene
            got[theta], got_beyond[theta] = rgb[:len(dirs)], rgb[len(dirs):]
        return w, h, env, dirs, centre, beyond, got, got_beyond

    @functools.lru_cache(None)
    def scene(self, res):
        return LC.material_scene(res)

    @functools.lru_cache(None)
    def surface(self, res):
        """-> rays (the injected rays of every quad, then the camera's decisive hits), quad of each injected ray, the
        oracle's first-hit records, (t, index) the float64 reference is evaluated at"""
        arrays = self.scene(res)
        rays = np.concatenate([LC.material_rays(res, k) for k in range(len(LC.QUAD_NAMES))])
        quad = np.concatenate([np.full(len(LC.material_rays(res, k)), k) for k in range(len(LC.QUAD_NAMES))])
        fh = np.concatenate([oracle_trace(arrays, LC.material_rays(res, k), 0.0, 1)[1] for k in range(len(LC.QUAD_NAMES))])
        assert np.array_equal(fh["index"] // 2, quad)      # every injected ray hits its quad
        cam_rays, cam_fh, cam_t, cam_index = self.camera(res)
        return (np.concatenate([rays, cam_rays]), quad, np.concatenate([fh, cam_fh]),
                np.concatenate([fh["t"].astype(np.float64), cam_t]), np.concatenate([fh["index"], cam_index]))

    @functools.lru_cache(None)
    def camera(self, res):
        """the camera's rays whose closest hit hitref decides: rays, the oracle's records, hitref's (t, index)"""
        arrays, (W, H), c = self.scene(res), LC.CAMERA_FRAME, LC.CAMERA
        from fspt_amd import scene as S
        pos, d = O.camera(W, H, c["P"], c["I"], c["fov_scale"], S.lens_features(c["focal_depth"], c["aperture"]),
                          O.rand_base_stream(LC.CAMERA_SEED, 1)[0])
        acc = np.zeros((H, W, 4), np.float32)
        fh = O.trace(arrays, W, H, pos, d, 0, 0.5, 0.0, 1, acc, first_hits=True)
        rays = np.concatenate([pos[..., :3], d[..., :3]], -1).reshape(-1, 6)
        cl = hitref.classify(arrays, rays)
        assert cl.mismatches(fh["t"], fh["index"]) == []
        hit = np.flatnonzero(cl.kind == 1)
        assert set(fh["index"][hit] // 2) == set(range(len(LC.QUAD_NAMES))) and (cl.kind == 0).any()   # every quad seen, and misses
        pick = [int(np.flatnonzero(cl.ties[i][0] == fh["index"][i])[0]) for i in hit]
        t64 = np.array([cl.ties[i][1][p] for i, p in zip(hit, pick)])
        return rays[hit], fh[hit], t64, fh["index"][hit]

    @functools.lru_cache(None)
    def surface_ref(self, res, mutant=None):
        rays, _, _, t, index = self.surface(res)
        return LR.hit_surface(self.scene(res), rays, t, index, **({"mutant": mutant} if mutant else {}))

    @functools.lru_cache(None)
    def emission(self, res):
        """-> oracle radiance of the injected rays at num_bounces = 1 per emission quad, by name"""
        return {q: oracle_trace(self.scene(res), LC.material_rays(res, LC.QUAD_NAMES.index(q)), 0.0, 1)[0] for q in LC.EMISSION_QUADS}

    def emission_ref(self, res, q):
        k = LC.QUAD_NAMES.index(q)
        rays, quad, _, _, _ = self.surface(res)
        ref = self.surface_ref(res)
        m = np.flatnonzero(quad == k)
        return 30.0 * ref["emissive"][m] * ref["diffuse"][m]


@pytest.fixture(scope="module")
def cases(small_scene):
    return Cases(small_scene)


def measure(cases):
    m = dict.fromkeys(LC.MEASURED, 0.0)
    for name in LC.ENV_MAPS:
        w, h, env, dirs, _, _, got, _ = cases.env(name)
        for theta in LC.ENV_THETAS:
            m["env"] = max(m["env"], LC.deviation(got[theta], LR.env_lookup(env, w, h, dirs, theta)).max())
    for res in LC.ATLAS_SIZES:
        fh, ref = cases.surface(res)[2], cases.surface_ref(res)
        for k in SURFACE_KEYS:
            m[k] = max(m[k], LC.deviation(fh[k], ref[k]).max())
        for q, got in cases.emission(res).items():
            m["emission"] = max(m["emission"], LC.deviation(got, cases.emission_ref(res, q)).max())
    return m


def test_measured_tolerances_are_current(cases):
    """The figures of lookup_cases.MEASURED are what the oracle deviates from the reference by (printed with -s); each is
    far below a texel step (this is a lookup of 8-bit texels: 1 / 255 = 3.9e-3)."""
    m = measure(cases)
    print("\nMEASURED = {\n" + "".join(f'    "{k}": {float(f"{v:.3g}") + 10 ** (np.floor(np.log10(v)) - 2):.3g},\n' for k, v in m.items()) + "}")
    for k, v in m.items():
        assert v <= 1e-3, (k, v)
        assert v <= LC.MEASURED[k] <= 1.25 * v + 1e-12, (k, v, LC.MEASURED[k])


# ---- the environment lookup ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.ENV_MAPS))
def test_environment_oracle_matches_float64(cases, name):
    w, h, env, dirs, _, beyond, got, got_beyond = cases.env(name)
    for theta in LC.ENV_THETAS:
        dev = LC.deviation(got[theta], LR.env_lookup(env, w, h, dirs, theta))
        assert dev.max() <= LC.BOUND["env"], (theta, dirs[dev.argmax()], dev.max())
        # beyond the definition (|y| > 1; the zero direction): asin's documented clamp, atan2(0, 0) = 0
        dev = LC.deviation(got_beyond[theta], LR.env_lookup(env, w, h, beyond, theta))
        assert dev.max() <= LC.BOUND["env"], (theta, beyond[dev.argmax()], dev.max())


def test_environment_mutants_are_rejected(cases):
    """Each defect of the reference is told from the oracle by the same bound on the same cases; the first case that does
    is named (-s)."""
    for mutant in LR.ENV_MUTANTS:
        found = None
        for name in LC.ENV_MAPS:
            w, h, env, dirs, _, _, got, _ = cases.env(name)
            for theta in LC.ENV_THETAS:
                dev = LC.deviation(got[theta], LR.env_lookup(env, w, h, dirs, theta, mutant))
                if found is None and dev.max() > LC.BOUND["env"]:
                    found = (name, theta, dirs[dev.argmax()].tolist(), float(dev.max()), int((dev > LC.BOUND["env"]).sum()))
        assert found is not None, f"mutant {mutant} survives every environment case"
        print(f"\n{mutant}: rejected by map {found[0]} at env_theta {found[1]}, direction {found[2]}: off by {found[3]:.3g} ({found[4]} directions)")


def test_environment_exact_expectations(cases):
    # a constant map returns its decoded value bit for bit, whatever the footprint and the weights
    w, h, env, dirs, _, _, got, got_beyond = cases.env("const_15x7")
    r, g, b, e = (np.float32(x) / np.float32(255) for x in LC.CONST_TEXEL)
    sc = O.math_eval(4, np.array([np.float64(e) * 255 - 128], np.float32))[0]   # exp2(fma(e, 255, -128)): one rounding
    want = np.array([r * sc, g * sc, b * sc], np.float32)
    for theta in LC.ENV_THETAS:
        assert (got[theta] == want).all() and (got_beyond[theta] == want).all()
    # the (column, row) map at texel centres names that texel
    w, h, env, dirs, centre, _, got, _ = cases.env("colrow_22x10")
    at = centre[:, 0] >= 0
    assert at.sum() == w * h
    named = np.rint(got[0.0][at].astype(np.float64) * 255).astype(int)
    assert np.array_equal(named[:, :2], centre[at]) and np.array_equal(named[:, 2], 255 - centre[at][:, 0])
    shift = np.rint(got[1.0][at].astype(np.float64) * 255).astype(int)      # a whole turn of env_theta: the same texel
    assert np.array_equal(shift[:, :2], centre[at])


@pytest.mark.parametrize("name", list(LC.ENV_MAPS))
def test_environment_cases_cover_the_map(cases, name):
    w, h, _, dirs, _, _, _, _ = cases.env(name)
    seen, wrapped, clamped, below, tiles = set(), set(), set(), set(), set()
    for theta in LC.ENV_THETAS:
        cx, cy = LR.env_coords(dirs, theta)
        i0, j0, _, _, _ = LR.footprint(w, h, cx, cy, False)
        col, row = np.mod(i0, w), np.clip(j0, 0, h - 1)
        seen |= set(zip(col.tolist(), row.tolist()))
        wrapped |= set(row[col == w - 1].tolist())                   # last column: its neighbour is column 0
        clamped |= set(col[j0 == h - 1].tolist())                    # last row: its neighbour is itself
        below |= set(col[j0 < 0].tolist())
        tiles |= set(zip((col // 7).tolist(), (row // 3).tolist()))  # the overlapping tiles' pitch
    assert seen == {(i, j) for i in range(w) for j in range(h)}      # every texel is some lookup's t00
    assert wrapped == set(range(h)) and clamped == set(range(w)) and below == set(range(w))
    assert tiles == {(a, b) for a in range((w + 6) // 7) for b in range((h + 2) // 3)}


# ---- the hit record and the material layers --------------------------------------------------------------------------
@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_surface_oracle_matches_float64(cases, res):
    fh, ref = cases.surface(res)[2], cases.surface_ref(res)
    for k in SURFACE_KEYS:
        dev = LC.deviation(fh[k], ref[k])
        assert dev.max() <= LC.BOUND[k], (k, int(dev.argmax()), dev.max())


@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_emission_oracle_matches_float64(cases, res):
    """num_bounces = 1 on a scene without an environment: 30 * texEmissive * texDiffuse of the first vertex and nothing
    else - finite on every ray (the shadow and extension terms are exact zeros)."""
    for q, got in cases.emission(res).items():
        assert np.isfinite(got).all(), q
        dev = LC.deviation(got, cases.emission_ref(res, q))
        assert dev.max() <= LC.BOUND["emission"], (q, int(dev.argmax()), dev.max())


def test_surface_mutants_are_rejected(cases):
    for mutant in LR.SURFACE_MUTANTS:
        found = None
        for res in LC.ATLAS_SIZES:
            fh, ref = cases.surface(res)[2], cases.surface_ref(res, mutant)
            for k in SURFACE_KEYS:
                dev = LC.deviation(fh[k], ref[k])
                if found is None and dev.max() > LC.BOUND[k]:
                    i = int(dev.argmax())
                    found = (res, k, LC.QUAD_NAMES[fh["index"][i] // 2], fh["uv"][i].tolist(), float(dev.max()), int((dev > LC.BOUND[k]).sum()))
        assert found is not None, f"mutant {mutant} survives every material case"
        print(f"\n{mutant}: rejected at atlas size {found[0]} by {found[1]} on quad {found[2]} at uv {found[3]}: off by {found[4]:.3g} ({found[5]} rays)")


def test_every_mutant_is_tried():
    assert set(LR.ENV_MUTANTS) | set(LR.SURFACE_MUTANTS) == set(LR.MUTANTS)


@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_storage_forms(cases, res):
    """Each scene holds every storage form at its budget (a one-texel atlas: all constant), and the sweep's three budgets
    interleave none, one and all of the sets that can be."""
    arrays = cases.scene(res)
    for n, n_quad in ((2, 2), (0, 0), (1, 1), (3, 3)):
        kinds = LC.classify(arrays, LC.budget(res, n))
        want = LC.expected_forms(res, n)
        assert [int(k) for k in kinds[::2]] == [want[q] for q in LC.QUAD_NAMES], n
        if res > 1:
            assert (kinds[::2] == TEXSET_QUAD).sum() == n_quad
    if res > 1:
        assert set(LC.expected_forms(res).values()) == {TEXSET_CONST, TEXSET_SEPARATE, TEXSET_QUAD}


def test_const_set_is_the_unfiltered_texel(cases):
    for res in LC.ATLAS_SIZES:
        fh, quad = cases.surface(res)[2], cases.surface(res)[1]
        m = np.flatnonzero(quad == LC.QUAD_NAMES.index("const"))
        c1, c2 = (np.array(c, np.float32) / np.float32(255) for c in LC.CONST_COLOURS[1:])
        assert (fh["diffuse"][m] == c1[:3]).all() and (fh["emissive"][m] == c2[:3]).all() and (fh["mr"][m] == c2[:2]).all()
        want_n = np.array([(c1[0] - np.float32(0.5)) * 2, (c1[1] - np.float32(0.5)) * 2, c1[2]], np.float32)
        assert (fh["tex_normal"][m] == want_n).all()


@pytest.mark.parametrize("res", LC.ATLAS_SIZES)
def test_material_cases_cover_the_atlas(cases, res):
    """From the float64 footprints of the injected rays, per quad: every texel is some lookup's t00, the last column is
    read with its wrapped neighbour and the last row with its wrapped one, both column cases of tap_geom occur (paired:
    i1 = i0 + 1 inside an 8-wide tile; unpaired: i0 & 7 = 7 or a wrapped i1), and so every tile of both layouts is read."""
    _, quad, _, _, _ = cases.surface(res)
    ref = cases.surface_ref(res)
    for k in range(len(LC.QUAD_NAMES)):
        m = np.flatnonzero(quad == k)
        i0, j0, _, _, _ = LR.footprint(res, res, ref["uv"][m, 0], ref["uv"][m, 1], True)
        assert (i0 < 0).any() and (j0 < 0).any() and (i0 >= res).any() and (j0 >= res).any()   # REPEAT on both sides
        col, row = np.mod(i0, res), np.mod(j0, res)
        assert set(zip(col.tolist(), row.tolist())) == {(i, j) for i in range(res) for j in range(res)}
        assert set(row[col == res - 1].tolist()) == set(range(res)) and set(col[row == res - 1].tolist()) == set(range(res))
        unpaired = (np.mod(i0 + 1, res) != col + 1) | (col & 7 == 7)
        assert unpaired.any() and ((~unpaired).any() or res == 1)
        if res > 8:
            assert ((col & 7 == 7) & (np.mod(i0 + 1, res) == col + 1)).any()   # leaves the tile without wrapping
        assert set(zip((col >> 3).tolist(), (row >> 2).tolist())) == {(a, b) for a in range((res + 7) >> 3) for b in range((res + 3) >> 2)}
        assert set(zip((col >> 2).tolist(), (row >> 1).tolist())) == {(a, b) for a in range((res + 3) >> 2) for b in range((res + 1) >> 1)}


def test_nonfinite_uvs_follow_the_documented_rule():
    """Vertex uvs beyond the integer range, NaN and infinite: floor taken as 0 and weight 0, so every layer returns its
    texel (0, 0) - in the oracle, and in the reference's statement of that rule."""
    arrays = LC.nonfinite_scene()
    rays = LC.nonfinite_rays()
    _, fh = oracle_trace(arrays, rays, 0.0, 1, first_hits=True)
    assert (fh["index"] >= 0).all()
    ref = LR.hit_surface(arrays, rays, fh["t"], fh["index"])
    atlas = arrays.atlas.reshape(arrays.atlas_layers, -1, 4)
    mat = arrays.mat.reshape(-1, 12)
    want = atlas[mat[fh["index"], 0].astype(int), 0, :3].astype(np.float32) / np.float32(255)
    assert (fh["diffuse"] == want).all() and np.abs(ref["diffuse"] - want).max() < 1e-7
