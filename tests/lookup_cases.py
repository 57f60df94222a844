"""The committed inputs of the lookup tests (tests/test_lookup_cpu.py, tests/test_lookup_gpu.py): environment maps and
directions, material scenes and rays, and the measured tolerances.  Deterministic generators with fixed seeds, no files.

Environment: sizes one below, at and one above a multiple of the 7-column / 3-row pitch of the overlapping environment
tiles (fspt_kernels.hip env_taps), and the single texel; directions through the float64 inverse of the equirect mapping at
every texel centre, corner and edge midpoint - rounded to float32, which lands them on both sides of each floor boundary
- plus the poles, the seam, the axes, denormal components, unnormalised and random directions.

Materials: a few unit quads, one material texture set each, in every storage form (fspt_surface.hpp material<>), at
atlas sizes below, at and above the 8 x 4 and 4 x 2 tiles, with uvs that leave the unit square on both sides."""
import dataclasses

import numpy as np

import appearance_cases as AC

FRAME_W = 64

# ---- tolerances ------------------------------------------------------------------------------------------------------
# Largest deviation of the ORACLE (oracle/fspt_oracle.c, on the CPU) from the float64 reference (tests/lookup_ref.py) over
# every finite case below, |got - ref| / max(1, |ref|), per quantity.  Measured 2026-10-20 with
#     python -m pytest tests/test_lookup_cpu.py -k measured -s
# which prints this dict; test_measured_tolerances_are_current fails when a figure here is below what it measures.  Never
# measured on the HIP kernels.  The bound asserted - on the CPU and the GPU alike - is 4 x the measured value: the factor
# covers the one-ulp freedom a different but legitimate float32 evaluation order has in cx * w near a texel boundary,
# where the bilinear function is continuous but its two sides use different texel pairs.
MEASURED = {
    "env": 8.21e-05,
    "uv": 1.32e-06,
    "bary": 4.31e-07,
    "diffuse": 1.55e-05,
    "emissive": 1.22e-05,
    "mr": 9.62e-06,
    "tex_normal": 2.26e-05,
    "bary_normal": 2.17e-07,
    "macro_normal": 4.71e-05,
    "emission": 7.08e-05,
}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def deviation(got, ref):
    """|got - ref|, absolute below 1 and relative above; the largest over the last axis"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return d.reshape(len(d), -1).max(1) if d.ndim > 1 else d


# ---- frames ----------------------------------------------------------------------------------------------------------
MISS_RAY = np.array([0.0, 1.0e4, 0.0, 0.0, 1.0, 0.0], np.float32)   # far above everything, pointing up


def frame(rays):
    """rays float32 [n, 6] -> (pos, dir) float32 [H, 64, 4] for setRays, H as small as holds them; the pixels left
    over carry MISS_RAY.  Ray k is pixel k in row-major order."""
    rays = np.asarray(rays, np.float32).reshape(-1, 6)
    H = max(1, -(-len(rays) // FRAME_W))
    assert FRAME_W * H < 10000, len(rays)
    full = np.tile(MISS_RAY, (FRAME_W * H, 1))
    full[:len(rays)] = rays
    pos = np.ones((H, FRAME_W, 4), np.float32); d = np.ones((H, FRAME_W, 4), np.float32)
    pos[..., :3] = full[:, :3].reshape(H, FRAME_W, 3)
    d[..., :3] = full[:, 3:].reshape(H, FRAME_W, 3)
    return pos, d


# ---- environment maps ------------------------------------------------------------------------------------------------
ENV_SIZES = ((1, 1), (2, 3), (7, 3), (8, 4), (13, 5), (14, 6), (15, 7), (22, 10), (29, 17))
ENV_THETAS = (0.0, 0.25, -3.75, 1.0)
ENV_THETAS_HUGE = (1.0e6, -1.0e6)      # float32's own rounding of theta + atan2 / 2 pi dominates: bit-equality only
CONST_TEXEL = (200, 17, 255, 131)


def random_env(w, h):
    """random RGBE bytes (0 and 255 among them), exponent byte in 120..136: every value below the 1024 clamp"""
    rng = np.random.default_rng(1000 * w + h)
    env = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    env[..., 3] = rng.integers(120, 137, (h, w))
    env[0, 0, 0], env[-1, -1, 1] = 0, 255
    return env


def const_env(w, h):
    """every texel CONST_TEXEL: every lookup must return its decoded value exactly"""
    return np.tile(np.array(CONST_TEXEL, np.uint8), (h, w, 1))


def colrow_env(w, h):
    """each texel's bytes name its own (column, row), exponent 128 (scale 1): a wrong texel is a visible value"""
    env = np.zeros((h, w, 4), np.uint8)
    env[..., 0] = np.arange(w)[None, :]
    env[..., 1] = np.arange(h)[:, None]
    env[..., 2] = 255 - np.arange(w)[None, :]
    env[..., 3] = 128
    return env


ENV_MAPS = {f"{w}x{h}": (w, h, random_env) for w, h in ENV_SIZES}
ENV_MAPS["const_15x7"] = (15, 7, const_env)
ENV_MAPS["colrow_22x10"] = (22, 10, colrow_env)


def env_map(name):
    w, h, make = ENV_MAPS[name]
    return w, h, np.ascontiguousarray(make(w, h)).reshape(-1)


def texel_points(w, h):
    """texel-space points (x, y), texel (i, j) covering [i, i + 1) x [j, j + 1): every centre, corner and edge midpoint"""
    i, j = np.arange(w + 1), np.arange(h + 1)
    grid = lambda xs, ys: np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([grid(i[:-1] + 0.5, j[:-1] + 0.5), grid(i, j), grid(i[:-1] + 0.5, j), grid(i, j[:-1] + 0.5)]).astype(np.float64)


def env_direction(px, py, w, h):
    """float64 inverse of the mapping at env_theta 0: the unit direction whose lookup lands on texel-space (px, py)"""
    phi, lat = 2 * np.pi * px / w, np.pi * (py / h - 0.5)      # atan2(z, x), asin(-y)
    return np.stack([np.cos(lat) * np.cos(phi), -np.sin(lat), np.cos(lat) * np.sin(phi)], -1)


TINY = 1e-40  # a float32 denormal


def env_dirs(w, h):
    """-> (finite float32 [n, 3], texel-centre (column, row) int [n, 2] or -1, bit-equality-only float32 [m, 3])"""
    rng = np.random.default_rng(77 * w + h)
    pts = texel_points(w, h)
    centre = np.full((len(pts), 2), -1)
    centre[:w * h] = np.floor(pts[:w * h])
    # at the poles every column is the same direction: the first and last half rows (j0 < 0; the last row with its
    # clamped neighbour) are reached a quarter texel in, at every column and column boundary
    i = np.arange(2 * w) / 2.0
    caps = np.concatenate([np.stack([i, np.full_like(i, 0.25)], 1), np.stack([i, np.full_like(i, h - 0.25)], 1)])
    unit = rng.normal(size=(300, 3)); unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    flat = unit[np.abs(unit[:, 1]) < 0.5][:16]
    special = np.array([
        [0, 1, 0], [0, -1, 0],                                          # the poles
        [-1, 0, 0.0], [-1, 0, -0.0],                                    # the seam from both sides
        [1, 0, 0], [0, 0, 1], [0, 0, -1], [1, 0, -0.0],                 # the remaining axes
        [TINY, 0.6, 0.8], [0.6, TINY, 0.8], [0.6, 0.8, TINY], [-TINY, -0.6, 0.8], [0.6, -TINY, -0.8],
        [-1, 0, TINY], [-1, 0, -TINY], [-0.6, 0.8, -TINY]])
    dirs = np.concatenate([env_direction(pts[:, 0], pts[:, 1], w, h), env_direction(caps[:, 0], caps[:, 1], w, h),
                           special, 0.5 * flat[:8], 2.0 * flat[8:], unit]).astype(np.float32)
    centre = np.concatenate([centre, np.full((len(dirs) - len(centre), 2), -1)])
    beyond = np.array([[0.3, 1.5, 0.2], [0.0, -1.0000001, 0.0], [-2.0, 3.0, 1.0], [0.5, -1.25, -0.5],   # |y| > 1
                       [0.0, 0.0, 0.0]], np.float32)                                                     # the zero direction
    return dirs, centre, beyond


def scene_box(arrays):
    v = arrays.tri.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2


def away_rays(arrays, dirs):
    """rays with the given directions from origins 100 scene radii out along them (the zero direction: straight up), so
    that each points away from the scene and misses"""
    c, r = scene_box(arrays)
    d = np.asarray(dirs, np.float64)
    n = np.linalg.norm(d, axis=1, keepdims=True)
    out = np.where(n > 0, d / np.where(n > 0, n, 1), [0.0, 1.0, 0.0])
    return np.concatenate([(c + 100 * r * out).astype(np.float32), np.asarray(dirs, np.float32)], 1)


def env_scene(base, name):
    """`base` (the suite's small scene) under environment map `name`, one importance bin over the whole map"""
    w, h, env = env_map(name)
    return dataclasses.replace(base, env=env, env_w=w, env_h=h, bins=np.array([0, 0, w, h], np.uint32))


# ---- material scenes -------------------------------------------------------------------------------------------------
ATLAS_SIZES = (1, 3, 4, 5, 8, 9, 17)
UV_LO, UV_SPAN = -1.25, 3.5            # a quad's uvs run over [-1.25, 2.25] both ways: REPEAT on both sides, negative coordinates
N_CONST, N_LAYERS = 3, 12              # layers 0..2 hold one colour each, 3..11 are images
WHITE, C1, C2 = 0, 1, 2
CONST_COLOURS = ((255, 255, 255, 255), (0, 255, 77, 255), (255, 0, 200, 255))


def image(k):
    """the k-th image layer"""
    return N_CONST + k


# one material texture set per quad: (diffuse, emissive, mr, normal) layers.  An emissive layer of constant 255 lets the
# emission probe read the diffuse layer alone, a diffuse layer of constant 255 the emissive layer alone.
QUADS = {
    "quad_d": (image(0), WHITE, image(1), image(2)),   # TEXSET_QUAD (three image layers, inside the interleaving budget)
    "quad_e": (WHITE, image(3), image(1), image(2)),   # TEXSET_QUAD
    "sep4": (image(4), image(5), image(6), image(7)),      # four image layers beyond the budget: TEXSET_SEPARATE
    "sep1_d": (image(8), WHITE, C1, C2),       # TEXSET_SEPARATE: one image layer, three LAYER_CONST
    "sep1_e": (WHITE, image(0), C1, C2),       # ... the emissive one (a layer a QUAD set holds too)
    "sep1_n": (C1, C2, C1, image(2)),          # ... the normal map
    "const": (C1, C2, C2, C1),             # TEXSET_CONST
}
QUAD_NAMES = tuple(QUADS)
EMISSION_QUADS = ("quad_d", "quad_e", "sep4", "sep1_d", "sep1_e", "const")


def quad_tiles(res):
    return ((res + 3) // 4) * ((res + 1) // 2)


def budget(res, n_sets=2):
    """the interleaving budget (bytes) that holds exactly n_sets interleaved images of this atlas size"""
    return n_sets * quad_tiles(res) * 128


def expected_forms(res, n_interleaved=2):
    """the storage form of each quad's set, by name, at budget(res, n_interleaved)"""
    if res == 1:
        return {q: AC.TEXSET_CONST for q in QUADS}     # a one-texel layer is constant
    many = [q for q in QUAD_NAMES if len({l for l in QUADS[q] if l >= N_CONST}) >= 2]
    return {q: AC.TEXSET_QUAD if q in many[:n_interleaved] else
            AC.TEXSET_CONST if q == "const" else AC.TEXSET_SEPARATE for q in QUADS}


def material_atlas(res):
    a = AC.random_atlas(res, N_LAYERS, 4000 + res, const=range(N_CONST)).reshape(N_LAYERS, res, res, 4).copy()
    for l, c in enumerate(CONST_COLOURS):
        a[l] = c
    a[N_CONST:, 0, 0, 0], a[N_CONST:, -1, -1, 1] = 0, 255     # both ends of the byte range in every image
    return a.reshape(-1)


def quad_origin(k):
    return 2.0 * (k % 4), 2.0 * (k // 4)


def material_scene(res, quads=QUAD_NAMES, uvs=None):
    """Unit quads in the plane y = 0, two right-isosceles triangles each (their legs along x and z: Cramer's rule in
    hit_geom stays well conditioned, so its float32 error does not set the tolerance), quad k at quad_origin(k) with
    material texture set QUADS[quads[k]]; a chain BVH with one quad per leaf; no environment.  Per-vertex uvs
    UV_LO + UV_SPAN * (x, z), or the constant uvs[k] at every vertex where that is not None.  Vertex normals, tangents and
    bitangents are random tilts of (y, x, z) of differing lengths: not axis-aligned, not orthonormal."""
    from fspt_amd import scene as S
    rng = np.random.default_rng(9000 + res)
    n = len(quads)
    tri = np.zeros((n, 2, 3, 3), np.float32); uv = np.zeros((n, 2, 3, 2), np.float32)
    norm = np.zeros((n, 2, 3, 3, 3), np.float32); mat = np.zeros((n, 2, 12), np.float32)
    for k, name in enumerate(quads):
        x0, z0 = quad_origin(k)
        corner = {c: np.array([x0 + c[0], 0.0, z0 + c[1]]) for c in ((0, 0), (1, 0), (0, 1), (1, 1))}
        frame_ = {c: (np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]) + rng.uniform(-0.3, 0.3, (3, 3))) * [[1.0], [1.3], [0.8]] for c in corner}
        for half, cs in enumerate((((0, 0), (1, 0), (0, 1)), ((1, 1), (0, 1), (1, 0)))):
            for v, c in enumerate(cs):
                tri[k, half, v] = corner[c]
                norm[k, half, v] = frame_[c]
                uv[k, half, v] = UV_LO + UV_SPAN * np.array(c, np.float64) if uvs is None or uvs[k] is None else uvs[k]
        d, e, mr, nm = QUADS[name]
        mat[k, :, [AC.MAT_DIFFUSE, AC.MAT_EMISSIVE, AC.MAT_NORMAL, AC.MAT_MR]] = np.array([d, e, nm, mr], np.float32)[:, None]
        mat[k, :, AC.MAT_IOR], mat[k, :, AC.MAT_DIELECTRIC] = 1.4, -1.0
    lo, hi = tri.reshape(n, -1, 3).min(1), tri.reshape(n, -1, 3).max(1)
    bvh = np.zeros((2 * n - 1, 9), np.float32)
    iv = bvh.view(np.int32)
    idx = 0
    for k in range(n):                 # interior k (quads k..), then its left child, the leaf of quad k; the last leaf alone
        if k < n - 1:
            iv[idx, :3] = (idx + 1, idx + 2, -1)
            bvh[idx, 3:6], bvh[idx, 6:9] = lo[k:].min(0), hi[k:].max(0)
            idx += 1
        iv[idx, :3] = (0, 0, 2 * k)
        bvh[idx, 3:6], bvh[idx, 6:9] = lo[k], hi[k]
        idx += 1
    return S.SceneArrays(bvh=bvh.reshape(-1), tri=tri.reshape(-1), mat=mat.reshape(-1), norm=norm.reshape(-1), uv=uv.reshape(-1),
                         atlas=material_atlas(res), atlas_res=res, atlas_layers=N_LAYERS, env=None, env_w=0, env_h=0,
                         bins=np.array([0, 0, 1, 1], np.uint32), leaf_size=2)


def classify(arrays, budget_bytes):
    """the storage form of each triangle's material texture set, by appearance_cases.classify_ref"""
    layers = arrays.atlas.reshape(arrays.atlas_layers, -1, 4)
    is_const = [bool((l == l[0]).all()) for l in layers]
    first = [int(np.ascontiguousarray(l[0]).view(np.uint32)[0]) for l in layers]
    tri_set, tab = AC.classify_ref(arrays.mat, arrays.atlas_layers, arrays.atlas_res, is_const, first, budget_bytes)
    return tab[tri_set, 0]


UV_SHIFTS = ((0, 0), (-1, 1), (1, -1))


def material_uvs(res):
    """uv targets: every texel centre, corner and edge midpoint of the unit square, and the same one period off on either
    side (s down and t up; s up and t down)"""
    p = texel_points(res, res) / res
    return np.concatenate([p + np.array(sh, np.float64) for sh in UV_SHIFTS])


def down_rays(k, uv):
    """rays straight down from y = 1 onto the points of quad k whose uv is `uv` [n, 2] (t = 1, the hit point's x and z the
    origin's): rounding the origin to float32 puts the uv on either side of its target"""
    x0, z0 = quad_origin(k)
    local = (np.asarray(uv, np.float64) - UV_LO) / UV_SPAN
    assert (local > 0.01).all() and (local < 0.99).all()
    o = np.stack([x0 + local[:, 0], np.ones(len(local)), z0 + local[:, 1]], 1)
    return np.concatenate([o, np.tile([0.0, -1.0, 0.0], (len(o), 1))], 1).astype(np.float32)


def material_rays(res, k):
    return down_rays(k, material_uvs(res))


CAMERA = dict(P=[3.5, 5.0, 2.6], I=[0.0, -1.0, -0.2], fov_scale=0.45, env_theta=0.0, focal_depth=2.0, aperture=0.0)
CAMERA_FRAME = (64, 32)
CAMERA_SEED = 7

# bit-equality only: quads whose vertex uvs are beyond the integer range, NaN and infinite, in a QUAD and a SEPARATE set
NONFINITE_RES = 5
NONFINITE_UVS = (3.0e9, np.nan, np.inf, -np.inf)
NONFINITE_QUADS = tuple(q for _ in NONFINITE_UVS for q in ("quad_d", "sep1_d"))


def nonfinite_scene():
    uvs = [np.float32(u) for u in NONFINITE_UVS for _ in range(2)]
    return material_scene(NONFINITE_RES, NONFINITE_QUADS, uvs)


def nonfinite_rays():
    rng = np.random.default_rng(5)
    return np.concatenate([down_rays(k, UV_LO + UV_SPAN * rng.uniform(0.05, 0.95, (12, 2))) for k in range(len(NONFINITE_QUADS))])
