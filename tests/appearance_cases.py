"""Cases and host restatements for the in-place appearance update (fspt_scene_update_materials / _environment).

Shared by tests/test_appearance_gpu.py and tests/test_appearance_cpu.py.  A case is a pair of SceneArrays over ONE topology
(bvh, tri, norm, leaf_size): the scene is created from the first, updated to the second, and compared with a scene created
from the second.  The cases are chosen where the layout code can go wrong - atlas resolutions around the two tile shapes,
layers that turn constant, the set forms, layer_of's corners, the environment apron's stride corners - not for size."""
import dataclasses

import numpy as np

MAT_DIFFUSE, MAT_EMISSIVE, MAT_NORMAL, MAT_MR, MAT_IOR, MAT_DIELECTRIC = 0, 1, 2, 3, 9, 10
TEXSET_CONST, TEXSET_SEPARATE, TEXSET_QUAD = 0, 1, 2
LAYER_CONST = 0xFFFFFFFF
DEFAULT_BUDGET = 8 << 30


# ---- the host's statements -------------------------------------------------------------------------------------------
def layer_of_ref(ids, n_layers):
    """clamp(floor(id + 0.5), 0, n_layers - 1) in binary32, NaN -> 0 (include/fspt.h: how matTex's layer ids are resolved)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.floor(np.asarray(ids, np.float32) + np.float32(0.5))
        out = np.zeros(x.shape, np.uint32)
        ok = x >= 0  # (False for NaN)
        top = ok & (x >= np.float32(n_layers - 1))
        mid = ok & ~top
        out[top] = n_layers - 1
        out[mid] = x[mid].astype(np.uint32)
    return out


def classify_ref(mat, n_layers, res, is_const, first, budget=DEFAULT_BUDGET):
    """The set classification as DESIGN 3 / 8.13 state it: sets in first-appearance order of (diffuse, emissive, mr, normal)
    layer keys; a set with >= 2 distinct image layers is QUAD while the interleaving budget lasts, one with >= 1 is
    SEPARATE, else CONST; the image layers of SEPARATE sets are stored once each, in first-use order.
    -> tri_set uint32 [T], tab uint32 [n_sets, 12]"""
    m = np.asarray(mat, np.float32).reshape(-1, 12)
    keys = np.stack([layer_of_ref(m[:, c], n_layers) for c in (MAT_DIFFUSE, MAT_EMISSIVE, MAT_MR, MAT_NORMAL)], 1)
    ids, sets, tri_set = {}, [], np.zeros(len(m), np.uint32)
    for i, k in enumerate(map(tuple, keys.tolist())):
        if k not in ids:
            ids[k] = len(sets)
            sets.append(k)
        tri_set[i] = ids[k]
    quad_tiles = ((res + 3) // 4) * ((res + 1) // 2)
    layer_tiles = ((res + 7) // 8) * ((res + 3) // 4)
    kind, quad_bytes, n_quad = [], 0, 0
    for k in sets:
        n_img = len({l for l in k if not is_const[l]})
        if n_img >= 2 and quad_bytes + quad_tiles * 128 <= budget and (n_quad + 1) * quad_tiles < 0xFFFFFFFF:
            kind.append(TEXSET_QUAD); quad_bytes += quad_tiles * 128; n_quad += 1
        else:
            kind.append(TEXSET_SEPARATE if n_img >= 1 else TEXSET_CONST)
    base, tiles = {}, 0
    for k, kd in zip(sets, kind):
        if kd != TEXSET_SEPARATE:
            continue
        for l in k:
            if not is_const[l] and l not in base:
                base[l] = tiles
                tiles += layer_tiles
    tab = np.zeros((len(sets), 12), np.uint32)
    qi = 0
    for si, (k, kd) in enumerate(zip(sets, kind)):
        tab[si, 0] = kd
        for c, l in enumerate(k):
            tab[si, 4 + c] = first[l]
            tab[si, 8 + c] = base[l] if kd == TEXSET_SEPARATE and not is_const[l] else LAYER_CONST
        if kd == TEXSET_QUAD:
            tab[si, 1] = qi * quad_tiles
            qi += 1
    return tri_set, tab


# ---- building blocks -------------------------------------------------------------------------------------------------
def random_atlas(res, layers, seed, const=()):
    """random RGBA8 texels; the layers in `const` hold one colour"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (layers, res, res, 4), dtype=np.uint8)
    a[..., 3] = 255
    for l in const:
        a[l] = a[l, 0, 0]
    return a.reshape(-1)


def grouped_ids(n_tris, table):
    """float32 [n_tris, 4] layer ids (diffuse, emissive, normal, mr): triangle i takes row i * len(table) // n_tris"""
    t = np.asarray(table, np.float32).reshape(-1, 4)
    return t[(np.arange(n_tris) * len(t)) // n_tris]


def retex(a, res, layers, seed, const=(0,), table=None, new_uv=False):
    """`a` with a random atlas of the given shape and layer ids from `table` (default: 5 random rows)"""
    rng = np.random.default_rng(seed + 1000)
    if table is None:
        table = rng.integers(0, layers, (5, 4)).astype(np.float32)
    mat = a.mat.reshape(-1, 12).copy()
    mat[:, [MAT_DIFFUSE, MAT_EMISSIVE, MAT_NORMAL, MAT_MR]] = grouped_ids(a.n_tris, table)
    kw = dict(mat=mat.reshape(-1), atlas=random_atlas(res, layers, seed, const), atlas_res=res, atlas_layers=layers)
    if new_uv:
        kw["uv"] = rng.uniform(-0.5, 1.5, a.uv.size).astype(np.float32)
    return dataclasses.replace(a, **kw)


def with_env(a, w, h, seed, n_bins=None):
    """`a` with a random w x h RGBE environment (None: no map) and its bins (n_bins = 1: one bin over the whole map)"""
    from fspt_amd import scene as S
    if w is None:
        return dataclasses.replace(a, env=None, env_w=0, env_h=0, bins=np.array([0, 0, 1, 1], np.uint32))
    rng = np.random.default_rng(seed)
    env = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    env[..., 3] = rng.integers(124, 131, (h, w))
    env = env.reshape(-1)
    bins = np.array([0, 0, w, h], np.uint32) if n_bins == 1 else np.ascontiguousarray(S.env_bins(env, w, h), np.uint32).reshape(-1)
    return dataclasses.replace(a, env=env, env_w=w, env_h=h, bins=bins)


def with_dielectric(a, on):
    """every triangle that refracts switched off (dielectric -1), or the sphere-like last tenth of the triangles switched on"""
    mat = a.mat.reshape(-1, 12).copy()
    if on:
        mat[-max(a.n_tris // 10, 1):, MAT_DIELECTRIC] = 0.2
        mat[-max(a.n_tris // 10, 1):, MAT_IOR] = 1.4
    else:
        mat[:, MAT_DIELECTRIC] = -1.0
    return dataclasses.replace(a, mat=mat.reshape(-1))


ATLAS_RES = (1, 2, 3, 5, 8, 9, 16, 33)       # below one tile of either layout, exactly one, one texel over
ENV_SIZES = ((1, 1), (7, 3), (8, 4), (15, 7), (64, 32))  # the apron's stride corners
FULL_PRODUCT = ("res_9", "e3_dielectric_off")  # pipeline x sampler x lights; the rest: wavefront


def fuzz_leaf5():
    """a random soup (tests/rays.py fuzz_scene) built with leaf size 5 whose last leaf is partially filled: padding slots"""
    import rays as RY
    for seed in range(1, 200):
        arrays = RY.fuzz_scene(seed)[0]
        ts = arrays.bvh.view(np.int32).reshape(-1, 9)[:, 2]
        if arrays.leaf_size == 5 and ts.max() + 5 > arrays.n_tris:  # the last leaf reads into the "-1" padding
            return arrays
    raise AssertionError("no fuzz seed with leaf size 5")


def bases(small_scene):
    import lights_ref as LR
    from fspt_amd import scene as S
    return {"textured": S.textured_test_scene(16), "small": small_scene, "e3": LR.scene_e3(), "fuzz": fuzz_leaf5()}


def pairs(b):
    """name -> (arrays0, arrays1, options); options: budget (interleaving budget for both scenes), uv (pass the uvs: default True)"""
    t, small, e3, fuzz = b["textured"], b["small"], b["e3"], b["fuzz"]
    p = {}
    for r in ATLAS_RES:  # from the 16 x 16 base: 16 -> 9 among them
        p[f"res_{r}"] = (t, retex(t, r, 5, r, new_uv=True), {})
    p["res_1_to_16"] = (retex(t, 1, 4, 50), retex(t, 16, 4, 51), {})
    p["layers_shrink"] = (retex(t, 8, 6, 52), retex(t, 8, 2, 53), {})
    p["layers_grow"] = (retex(t, 8, 2, 54), retex(t, 8, 7, 55), {})
    # a layer turns from image to constant and back: the same ids, layer 1 flat or not
    tab = [[1, 0, 2, 1], [1, 1, 1, 1], [2, 1, 0, 0]]
    img, flat = retex(t, 9, 3, 56, const=(0,), table=tab), retex(t, 9, 3, 56, const=(0, 1), table=tab)
    p["image_to_const"] = (img, flat, {})
    p["const_to_image"] = (flat, img, {})
    p["all_const"] = (t, retex(t, 5, 4, 57, const=(0, 1, 2, 3)), {})
    # one image layer (SEPARATE) | two (QUAD) | the same layer in two key positions (one image: SEPARATE) | ... beside another (QUAD)
    forms = [[1, 0, 0, 0], [1, 2, 0, 0], [3, 3, 0, 0], [3, 3, 0, 1], [0, 0, 0, 0]]
    p["set_forms"] = (t, retex(t, 9, 4, 58, table=forms), {})
    p["budget_0"] = (t, retex(t, 9, 5, 9), {"budget": 0})
    # layer_of's corners on a few triangles each
    L = 4
    corners = [[-1, 0.49, 0.5, L - 1 + 0.6], [np.nan, np.inf, -np.inf, 1.5], [0.49, np.nan, L - 1 + 0.6, -1], [2.5, 2.4999, 3.5, 0]]
    p["id_corners"] = (t, retex(t, 5, L, 59, const=(), table=corners), {})
    # the emissive layer switches on for geometry that was dark, and off again
    dark = retex(t, 8, 3, 60, const=(0,), table=[[1, 0, 2, 1]])
    dark.atlas.reshape(3, -1, 4)[0] = (0, 0, 0, 255)
    lit = dataclasses.replace(dark, mat=dark.mat.copy())
    lit.mat.reshape(-1, 12)[: t.n_tris // 2, MAT_EMISSIVE] = 1
    p["emissive_on"] = (dark, lit, {})
    p["emissive_off"] = (lit, dark, {})
    p["e3_dielectric_off"] = (e3, with_dielectric(e3, False), {})
    p["e3_dielectric_on"] = (with_dielectric(e3, False), e3, {})
    p["uv_kept"] = (t, dataclasses.replace(retex(t, 16, 5, 61), uv=t.uv), {"uv": False})
    p["small_retex"] = (small, retex(small, 3, 3, 62, new_uv=True), {})
    p["fuzz_leaf5"] = (fuzz, with_env(retex(fuzz, 5, 4, 63, new_uv=True), 15, 7, 63), {})
    for w, h in ENV_SIZES:
        p[f"env_{w}x{h}"] = (small, with_env(small, w, h, w * 100 + h), {})
    p["env_none"] = (small, with_env(small, None, None, 0), {})
    p["env_back"] = (with_env(small, None, None, 0), small, {})
    p["env_one_bin"] = (small, with_env(small, 8, 4, 64, n_bins=1), {})
    return p
