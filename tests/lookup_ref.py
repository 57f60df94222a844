"""float64 numpy statement of the lookups a path makes: the equirect environment fetch (tracer.fs:410-419), the four
material layers at one uv (tracer.fs:453-456) and the hit record's barycentric, uv and tangent-frame arithmetic
(tracer.fs:339-353, 447-460).  The checker tests/test_lookup_cpu.py holds the oracle to and tests/test_lookup_gpu.py the
HIP kernels.

The kernels and the oracle were written from the same reading of the shader and agree bit for bit; that cannot reveal an
error they share.  This is written from the sampler state the shader asks for (atlas bilinear REPEAT,
environment bilinear on the RGBE bytes with S = REPEAT, T = CLAMP_TO_EDGE) on plain [h, w, 4] images: no tiles, no paired
loads, no storage forms.  Inputs (texel bytes, directions, uvs, vertices, t) are the float32 values taken exactly;
everything after that is float64.

`mutant` names one deliberate defect (MUTANTS); tests/test_lookup_cpu.py proves that the committed cases
(tests/lookup_cases.py) tell each from the lookup as defined.  None is the lookup itself.

Outside the shader's definition the project documents two rules, and this states them and nothing else; the finite cases
never reach either.  asin of an unnormalised direction with |y| > 1: fspt-math's asin clamps its input to [-1, 1]
(DESIGN.md 2).  A NaN or infinite uv, or a coordinate beyond the integer range (safe_floor_coord and the two weight
guards, fspt_surface.hpp): a floor that is not inside (-1e9, 1e9) is taken as 0, and a weight that is not inside [0, 1]
is taken as 0."""
import numpy as np

MAT_DIFFUSE, MAT_EMISSIVE, MAT_NORMAL, MAT_MR = 0, 1, 2, 3   # matTex's layer ids, in the scene's mat rows

MUTANTS = (
    "no_half",        # the -1/2 texel-centre offset dropped
    "clamp_s",        # CLAMP instead of REPEAT in s
    "repeat_t",       # REPEAT instead of CLAMP in t (environment only)
    "no_wrap_i1",     # the second column taken as i0 + 1 without wrapping (reads on into the next row)
    "swap_ab",        # the weights a and b swapped
    "exp_per_tap",    # the RGBE exponent decoded per tap instead of filtered (environment only)
    "swap_mr",        # metallic and rough swapped
    "blue_remap",     # the normal's blue channel remapped like red and green
    "swap_tb",        # tangent and bitangent swapped
)
ENV_MUTANTS = ("no_half", "clamp_s", "repeat_t", "no_wrap_i1", "swap_ab", "exp_per_tap")
SURFACE_MUTANTS = ("no_half", "clamp_s", "no_wrap_i1", "swap_ab", "swap_mr", "blue_remap", "swap_tb")


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def footprint(w, h, s, t, repeat_t, mutant=None):
    """The 2 x 2 footprint of a bilinear fetch at (s, t) on a w x h image: (i0, j0) the floors before wrapping, the flat
    texel indices (row * w + column) of t00, t10, t01, t11 and the weights a (columns) and b (rows)."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    half = 0.0 if mutant == "no_half" else 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = s * w - half, t * h - half
        fu, fv = np.floor(u), np.floor(v)
        fu = np.where((fu > -1e9) & (fu < 1e9), fu, 0.0)     # the documented rule; no finite case gets here
        fv = np.where((fv > -1e9) & (fv < 1e9), fv, 0.0)
        a, b = u - fu, v - fv
        a = np.where((a >= 0) & (a <= 1), a, 0.0)
        b = np.where((b >= 0) & (b <= 1), b, 0.0)
    i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
    if mutant == "swap_ab":
        a, b = b, a
    wrap_s = (lambda i: np.clip(i, 0, w - 1)) if mutant == "clamp_s" else (lambda i: np.mod(i, w))
    rep_t = (not repeat_t) if mutant == "repeat_t" else repeat_t
    wrap_t = (lambda j: np.mod(j, h)) if rep_t else (lambda j: np.clip(j, 0, h - 1))
    c0, c1, r0, r1 = wrap_s(i0), wrap_s(i0 + 1), wrap_t(j0), wrap_t(j0 + 1)
    if mutant == "no_wrap_i1":
        t10, t11 = (r0 * w + c0 + 1) % (w * h), (r1 * w + c0 + 1) % (w * h)
    else:
        t10, t11 = r0 * w + c1, r1 * w + c1
    return i0, j0, (r0 * w + c0, t10, r1 * w + c0, t11), a, b


def bilinear(img, s, t, repeat_t, mutant=None, decode=None):
    """img uint8 [h, w, 4] -> float64 [n, 4] in [0, 1] (decode: a per-texel function applied before the filter)"""
    h, w = img.shape[:2]
    tex = img.reshape(-1, 4).astype(np.float64) / 255.0
    if decode is not None:
        tex = decode(tex)
    _, _, (k00, k10, k01, k11), a, b = footprint(w, h, s, t, repeat_t, mutant)
    a, b = a[:, None], b[:, None]
    top = tex[k00] * (1 - a) + tex[k10] * a
    bot = tex[k01] * (1 - a) + tex[k11] * a
    return top * (1 - b) + bot * b


def env_coords(dirs, env_theta):
    """(cx, cy) of envSample: the direction is used as it is, not normalised (tracer.fs:416-419)"""
    d = _f64(dirs).reshape(-1, 3)
    theta = float(np.float32(env_theta))
    cx = theta + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi)
    cy = np.arcsin(np.clip(-d[:, 1], -1.0, 1.0)) / np.pi + 0.5   # |y| > 1: fspt-math's asin clamps its input
    return cx, cy


def _rgbe_decode(rgbe):
    return rgbe[:, :3] * np.exp2(255.0 * rgbe[:, 3:4] - 128.0)


def env_lookup(env_rgbe, w, h, dirs, env_theta, mutant=None):
    """clamp(envSample(dir), 0, 1024) -> float64 [n, 3]: what one sample of a ray that misses leaves in the accumulator.
    All four channels are filtered, the exponent byte included, and the result decoded (tracer.fs:410-414)."""
    assert mutant is None or mutant in MUTANTS, mutant
    img = np.asarray(env_rgbe, np.uint8).reshape(h, w, 4)
    cx, cy = env_coords(dirs, env_theta)
    if mutant == "exp_per_tap":
        rgb = bilinear(img, cx, cy, False, None, lambda x: np.concatenate([_rgbe_decode(x), x[:, 3:]], 1))[:, :3]
    else:
        rgb = _rgbe_decode(bilinear(img, cx, cy, False, mutant))
    return np.clip(rgb, 0.0, 1024.0)


def layer_of(ident, n_layers):
    """the atlas layer a material's layer id names: clamp(floor(id + 0.5), 0, n_layers - 1)"""
    return int(np.clip(np.floor(float(np.float32(ident)) + 0.5), 0, n_layers - 1))


def atlas_lookup(atlas, res, layer, s, t, mutant=None):
    """texture(texArray, vec3(s, t, layer)) -> float64 [n, 4]: bilinear, REPEAT both ways, on one res x res layer"""
    assert mutant is None or mutant in MUTANTS, mutant
    img = np.asarray(atlas, np.uint8).reshape(-1, res, res, 4)[layer]
    return bilinear(img, s, t, True, mutant)


def material_lookup(arrays, tri, s, t, mutant=None):
    """The four layers of triangle `tri`'s material at uv (s, t) as tracer.fs:453-456 decodes them: diffuse rgb, emissive
    rgb, (metallic, rough) - rough not squared - and the normal (2r - 1, 2g - 1, b).  tri, s, t: [n]."""
    tri = np.asarray(tri).reshape(-1)
    s, t = np.asarray(s, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    mat = np.asarray(arrays.mat, np.float32).reshape(-1, 12)
    out = {"diffuse": np.zeros((len(tri), 3)), "emissive": np.zeros((len(tri), 3)), "mr": np.zeros((len(tri), 2)),
           "tex_normal": np.zeros((len(tri), 3))}
    for k in np.unique(tri):
        m = tri == k
        fetch = lambda col: atlas_lookup(arrays.atlas, arrays.atlas_res, layer_of(mat[k, col], arrays.atlas_layers), s[m], t[m], mutant)
        out["diffuse"][m] = fetch(MAT_DIFFUSE)[:, :3]
        out["emissive"][m] = fetch(MAT_EMISSIVE)[:, :3]
        mr = fetch(MAT_MR)[:, :2]
        out["mr"][m] = mr[:, ::-1] if mutant == "swap_mr" else mr
        n = fetch(MAT_NORMAL)[:, :3]
        out["tex_normal"][m] = np.stack([2 * n[:, 0] - 1, 2 * n[:, 1] - 1, 2 * n[:, 2] - 1 if mutant == "blue_remap" else n[:, 2]], 1)
    return out


def hit_surface(arrays, rays, t, index, mutant=None):
    """The surface at hit (t, index) of rays [n, 6], from tri, norm and uv: the hit point, its barycentric weights in the
    triangle's plane, the interpolated uv, bary_normal (the interpolated vertex normal), the four material layers there
    and macro_normal (the texture normal in the interpolated tangent frame, normalised; before the `inside` flip)."""
    assert mutant is None or mutant in MUTANTS, mutant
    rays = _f64(rays).reshape(-1, 6)
    t = np.asarray(t, np.float64).reshape(-1)
    index = np.asarray(index).reshape(-1)
    tri = _f64(arrays.tri).reshape(-1, 3, 3)[index]
    nrm = _f64(arrays.norm).reshape(-1, 3, 3, 3)[index]     # [n, vertex, (normal, tangent, bitangent), xyz]
    uvs = _f64(arrays.uv).reshape(-1, 3, 2)[index]
    p = rays[:, :3] + rays[:, 3:] * t[:, None]
    e1, e2, q = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], p - tri[:, 0]
    dot = lambda x, y: (x * y).sum(-1)
    d00, d01, d11, d20, d21 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(q, e1), dot(q, e2)
    den = d00 * d11 - d01 * d01
    bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
    w = np.stack([1 - bv - bw, bv, bw], 1)
    with np.errstate(invalid="ignore"):                      # (0 * inf for a triangle with infinite uvs)
        uv = np.einsum("nk,nkj->nj", w, uvs)
    bary = lambda which: np.einsum("nk,nkj->nj", w, nrm[:, :, which])
    bn, bt, bb = bary(0), bary(1), bary(2)
    if mutant == "swap_tb":
        bt, bb = bb, bt
    out = material_lookup(arrays, index, uv[:, 0], uv[:, 1], mutant)
    tn = out["tex_normal"]
    m = tn[:, 0:1] * bt + tn[:, 1:2] * bb + tn[:, 2:3] * bn
    out.update(origin=p, bary=w, uv=uv, bary_normal=bn, macro_normal=m / np.sqrt(dot(m, m))[:, None])
    return out
