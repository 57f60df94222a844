"""The committed inputs of the shading-vertex tests (tests/test_shade_cpu.py, tests/test_shade_gpu.py): a material zoo, the
rays injected into it and the measured tolerances.  Deterministic generators with fixed seeds, no files.

The zoo is one scene of unit quads in the plane y = 0, one material texture set each, three cells apart so that a ray
meant for one cannot reach another, built as lookup_cases.material_scene builds its quads:

  opaque       metallic byte {0, 128, 255} x rough byte {0, 1, 8, 128, 255}; diffuse black / white / grey, normal-map texel
               flat / tilted / z byte 0 and a non-zero emissive layer dealt round-robin over them;
  dielectric   dielectric {0, 4, 100} x ior {1, 1.5} x rough byte {0, 128}, and one at metallic 128; 100 is large enough
               that 1 - (1 - d) t dielectric is negative over a slab's thickness;
  textured     one set with four image layers (stored interleaved, TEXSET_QUAD) and one with a single image layer
               (TEXSET_SEPARATE): material<true, true, true, true> is read through both fetch paths;
  slabs        six of the dielectric materials again as closed boxes 0.05 thick: a refracted ray's next vertex is an
               inside hit;
  razor        single dielectric quads whose ior is tuned to one ray each (TIR_RAZOR below): refract()'s kk < 0.

Every quad and slab stands twice: in part A (exact orthonormal vertex frames; an opaque catcher plane below at y = -2 and
a lid above half of its columns at y = 3, both glowing dimly, so extension and shadow rays hit something) and in part B (randomly tilted, non-orthonormal vertex
frames; nothing below or above, so they miss).  Emitters for the lights cases: E1 faces down under the lid, partly
hidden by an occluder; E2 is a strip in the plane y = 0 itself - edge-on (area x cosine exactly 0) from every vertex whose
origin stays in that plane; E3 has a non-zero emissive layer and a black diffuse one, so its table weight and pick are 0.
The environment is lookup_cases.random_env, its two pole rows one texel each (rays leave exactly along y), at a non-zero
env_theta.  A second scene, `dim`, is the same geometry under
65536 importance bins that each span a dim map: envPdf is 1 / (65536 x 2 pi^2 sin phi), on both sides of EPSILON."""
import dataclasses
import functools

import numpy as np

import appearance_cases as AC
import lookup_cases as LC

RAND_BASE = 0.5
ENV_THETA = 0.37
EPSILON = np.float32(0.000001)
ATLAS_RES = 5
ENV_SIZE = (13, 5)
DIM_ENV_SIZE, DIM_BINS, DIM_EXPONENT = (8, 4), 1 << 16, 108
PITCH = 3.0
GRID_W = 10
SLAB_THICKNESS = 0.05
EMITTER_FRACTIONS = (0.25, 0.5, 1.0)
RD_DOT_H_MIN, SIN_PHI_MIN = 1e-3, 1e-3            # the exemptions' thresholds (Vertices.exempt)

# ---- tolerances ------------------------------------------------------------------------------------------------------
# Largest deviation of the ORACLE (oracle/fspt_oracle.c, on the CPU) from the float64 reference (tests/shade_ref.py) over
# every non-exempt case below, lookup_cases.deviation, per field.  Measured 2026-10-21 with
#     python -m pytest tests/test_shade_cpu.py -k measured -s
# which prints this dict; test_measured_tolerances_are_current fails when a figure here is below what it measures.  Never
# measured on the HIP kernels.  The bound asserted - on the CPU and the GPU alike - is 4 x the measured value, the factor
# of lookup_cases.MEASURED and for its reason: a different but legitimate float32 evaluation order has a one-ulp freedom
# in each product that the measured evaluation order happened not to use.
# bsdf_pdf_sharp and lq_sharp are bsdf_pdf and lq of the specular lobes of width max(0.001, rough) = 0.001 (rough bytes 0, 1
# and 8): near-deltas whose density float32 does not resolve (gtr2's t cancels to 1e-6 .. 1e-4 from terms of size 1) - a
# property of the reference's formula, recorded in DESIGN 5; every other field of those vertices is held to the common bound.
MEASURED = {
    "micro_normal": 0.000211,
    "rd": 0.00033,
    "ro": 1.02e-07,
    "bsdf_pdf": 0.0017,
    "bsdf_pdf_sharp": 1.12,
    "env_pdf": 1.63e-05,
    "bsdf_throughput": 0.000786,
    "env_throughput": 0.000796,
    "weights": 0.00298,
    "emw": 0.000334,
    "lq": 2.48e-05,
    "lq_sharp": 0.0256,
    "pend": 2.19e-05,
    "sc": 0.00137,
    "colour": 0.00443,
    "accumulate": 9.57e-08,
}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}

# ---- the atlas -------------------------------------------------------------------------------------------------------
BLACK, WHITE, GREY, EMIT, GLOW = 0, 1, 2, 3, 4
CONST_TEXELS = [(0, 0, 0, 255), (255, 255, 255, 255), (128, 128, 128, 255), (200, 150, 100, 255), (3, 2, 1, 255)]
METALLIC_BYTES, ROUGH_BYTES = (0, 128, 255), (0, 1, 8, 128, 255)
MR0 = len(CONST_TEXELS)


def mr_layer(metallic, rough):
    return MR0 + METALLIC_BYTES.index(metallic) * len(ROUGH_BYTES) + ROUGH_BYTES.index(rough)


CONST_TEXELS += [(m, r, 0, 255) for m in METALLIC_BYTES for r in ROUGH_BYTES]
FLAT, TILT, Z0 = len(CONST_TEXELS), len(CONST_TEXELS) + 1, len(CONST_TEXELS) + 2
CONST_TEXELS += [(128, 128, 255, 255), (170, 100, 220, 255), (200, 90, 0, 255)]
IMG0 = len(CONST_TEXELS)
N_IMAGES = 5                     # diffuse, emissive, mr, normal of the interleaved set; the diffuse layer of the separate one
N_LAYERS = IMG0 + N_IMAGES


def atlas():
    rng = np.random.default_rng(31)
    a = np.zeros((N_LAYERS, ATLAS_RES, ATLAS_RES, 4), np.uint8)
    for l, c in enumerate(CONST_TEXELS):
        a[l] = c
    img = rng.integers(0, 256, (N_IMAGES, ATLAS_RES, ATLAS_RES, 4), dtype=np.uint8)
    img[..., 3] = 255
    img[1] //= 4                                     # a dim emission map
    img[3, ..., 2] = 128 + img[3, ..., 2] // 2       # the normal map keeps to the upper hemisphere
    a[IMG0:] = img
    return a.reshape(-1)


# ---- materials -------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Material:
    name: str
    diffuse: int
    emissive: int
    mr: int
    normal: int
    ior: float
    dielectric: float
    metallic: int = -1           # the bytes behind mr (-1: an image)
    rough: int = -1


# with diffuse (grey, white, black)[i % 3]: all nine pairs among the first ten.  A tangent-plane normal under a metallic 255
# mirror, or under a lobe of width 0.001, is nothing but the ill-conditioned grazing reflection: those keep to the other two
OPAQUE_NORMALS = (FLAT, TILT, TILT, TILT, Z0, FLAT, FLAT, FLAT, Z0, Z0, TILT, FLAT, TILT, FLAT, TILT)


def _materials():
    out = []
    for i, (m, r) in enumerate((m, r) for m in METALLIC_BYTES for r in ROUGH_BYTES):
        out.append(Material(f"opaque_m{m}_r{r}", (GREY, WHITE, BLACK)[i % 3], EMIT if i % 4 == 1 else BLACK, mr_layer(m, r),
                            OPAQUE_NORMALS[i], 1.5 if i % 2 else 1.0, -1.0, m, r))
    j = 0
    for d in (0.0, 4.0, 100.0):
        for ior in (1.0, 1.5):
            for r in (0, 128):
                out.append(Material(f"glass_d{d:g}_i{ior:g}_r{r}", (GREY, WHITE, BLACK)[j % 3], BLACK, mr_layer(0, r),
                                    TILT if j % 4 == 3 else FLAT, ior, d, 0, r))
                j += 1
    out.append(Material("glass_d4_i1.5_r8_m128", GREY, BLACK, mr_layer(128, 8), FLAT, 1.5, 4.0, 128, 8))
    out.append(Material("tex_quad", IMG0, IMG0 + 1, IMG0 + 2, IMG0 + 3, 1.5, -1.0))
    out.append(Material("tex_sep", IMG0 + 4, BLACK, mr_layer(128, 128), FLAT, 1.5, -1.0, 128, 128))
    return out


MATERIALS = _materials()
MATERIAL = {m.name: m for m in MATERIALS}
SLAB_MATERIALS = ("glass_d0_i1.5_r0", "glass_d4_i1.5_r128", "glass_d100_i1.5_r0", "glass_d100_i1_r128",
                  "glass_d4_i1.5_r8_m128", "glass_d100_i1.5_r128")
PLAIN = Material("plain", GREY, BLACK, mr_layer(0, 128), FLAT, 1.5, -1.0, 0, 128)          # the occluder
GLOWING = Material("glowing", GREY, GLOW, mr_layer(0, 128), FLAT, 1.5, -1.0, 0, 128)       # catcher and lid: a dim light of their own
LAMP = Material("lamp", WHITE, EMIT, mr_layer(0, 128), FLAT, 1.5, -1.0, 0, 128)            # E1, E2
DARK_LAMP = Material("dark_lamp", BLACK, EMIT, mr_layer(0, 128), FLAT, 1.5, -1.0, 0, 128)  # E3: Le = 0, pick 0
# (dielectric 0.5: over the ray's t = 1 the absorption leaves 0.75 - what the zero direction then finds stays visible)
RAZOR = Material("razor", GREY, BLACK, mr_layer(0, 0), FLAT, 3.0, 0.5, 0, 0)               # ior: TIR_RAZOR's, per quad

# refract()'s kk < 0 (tracer.fs:486 with "total internal reflection will go through the specular path" above it): schlick()
# tests n^2 (1 - c^2) > 1 with 1 - c^2 from one fma, refract() tests 1 - eta^2 (1 - c c) < 0 with c c rounded first, and the
# specular coin is lost against F = 0.9988 at the critical angle.  Found by search_tir_razor() below - one ray from
# behind per quad, whose sixth random number is above 0.9992, and the ior, a float32 ulp apart from its neighbours, at
# which the two roundings fall on either side of 1.  uint32 bit patterns: ior, then the ray's origin and direction.
TIR_RAZOR = (
    (0x40491b8a, 0x3f024abd, 0xbf7340f0, 0x41f385b2, 0xbe8d2d56, 0x3f7340f0, 0x3e14a48a),
    (0x4047f18e, 0x4051ad9f, 0xbf729b22, 0x41f37bdc, 0x3e2f681e, 0x3f729b22, 0x3e89eb14),
    (0x405e51b6, 0x40d4f049, 0xbf753f7b, 0x41f6a764, 0xbe7e514a, 0x3f753f7b, 0xbe12cfb4),
    (0x40359612, 0x411590cf, 0xbf6f090c, 0x41f708e7, 0x3e752381, 0x3f6f090c, 0xbe8844cc),
    (0x404cc43f, 0x4146585e, 0xbf732618, 0x41f37500, 0xbe319a9a, 0x3f732618, 0xbe85509d),
    (0x4078aa47, 0x41752185, 0xbf76f14d, 0x41f26049, 0x3e39daf7, 0x3f76f14d, 0xbe43d0b4),
    (0x4048348d, 0x419058c6, 0xbf721ce1, 0x41f5fa73, 0x3e3cf7a1, 0x3f721ce1, 0xbe88e722),
    (0x403325d5, 0x41aeb288, 0xbf6f89da, 0x41ef0d58, 0xbe326fdd, 0x3f6f89da, 0x3e9d1093),
    (0x4055294a, 0x41c6f524, 0xbf741e71, 0x41f571f9, 0xbe5cf58f, 0x3f741e71, 0xbe570de3),
    (0x404c9856, 0x41dd3bb3, 0xbf73429f, 0x41f1011e, 0x3e35b244, 0x3f73429f, 0x3e831ace),
    (0x40487722, 0x3f7fca53, 0xbf72fbe2, 0x42062957, 0xbe0243da, 0x3f72fbe2, 0x3e936f50),
    (0x4075b9ef, 0x406a181d, 0xbf76b9a8, 0x42062763, 0x3d9f4aab, 0x3f76b9a8, 0xbe82a1e1),
    (0x40205df7, 0x40bcb803, 0xbf6a5a59, 0x42066a42, 0x3eccde9e, 0x3f6a5a59, 0x3d309873),
    (0x40609c49, 0x411c5103, 0xbf757197, 0x4205e429, 0xbe70a264, 0x3f757197, 0xbe23aca4),
    (0x40326b02, 0x41463fae, 0xbf6e4482, 0x42082ca2, 0x3e969d0c, 0x3f6e4482, 0xbe5e799a),
    (0x40317adb, 0x4177694c, 0xbf6f372f, 0x42042c7d, 0xbe3d0238, 0x3f6f372f, 0x3e9bf013),
    (0x403b6eda, 0x41949bdb, 0xbf70c9c7, 0x420393fa, 0x3e03c8b6, 0x3f70c9c7, 0x3ea0e482),
    (0x4032f93a, 0x41ac1727, 0xbf6f5316, 0x4205739b, 0xbeb3f5d5, 0x3f6f5316, 0xbd4c7be7),
    (0x401ac186, 0x41c7e854, 0xbf69654c, 0x4206df27, 0xbecb7f4e, 0x3f69654c, 0xbdd51de4),
    (0x4059a244, 0x41ddd6cd, 0xbf74f7b9, 0x42076379, 0xbe935333, 0x3f74f7b9, 0x3d208a4a),
    (0x40248799, 0x3bd7ae69, 0xbf6b8a03, 0x4213854a, 0x3e28f044, 0x3f6b8a03, 0xbeb5eb12),
    (0x405059b6, 0x404b3c94, 0xbf73409c, 0x42124c35, 0x3e9de5c1, 0x3f73409c, 0x3d37640e),
    (0x4024d17e, 0x40d01341, 0xbf6b783b, 0x42129319, 0x3e8661ef, 0x3f6b783b, 0xbe955640),
    (0x4054376e, 0x411c440a, 0xbf742ab0, 0x4211c8ab, 0x3dfc1ca7, 0x3f742ab0, 0x3e8c5d07),
)


def cell_origin(c):
    return PITCH * (c % GRID_W), PITCH * (c // GRID_W)


N_SINGLE = len(MATERIALS)
CELLS_PER_PART = N_SINGLE + len(SLAB_MATERIALS)
PART_ROWS = -(-CELLS_PER_PART // GRID_W)
PART_B_CELL0 = (PART_ROWS + 1) * GRID_W                  # a free row between the parts
RAZOR_CELL0 = (2 * PART_ROWS + 2) * GRID_W
E2_CELL, E2_LENGTH = PART_ROWS * GRID_W, 14.0            # in the free row


@dataclasses.dataclass
class Item:
    """one quad (kind "quad": two triangles) or slab (kind "slab": six quads, the top one first)"""
    kind: str
    material: Material
    part: str
    cell: int
    first_quad: int


def _frame(normal, rng):
    n = np.asarray(normal, np.float64)
    t = np.array([1.0, 0, 0]) if abs(n[0]) < 0.5 else np.array([0.0, 0, 1.0])
    b = np.cross(n, t)
    f = np.stack([n, t, b])
    if rng is None:
        return [f] * 4
    return [(f + rng.uniform(-0.2, 0.2, (3, 3))) * [[1.0], [1.3], [0.8]] for _ in range(4)]


class Builder:
    def __init__(self):
        self.corners, self.frames, self.mats, self.iors = [], [], [], []

    def quad(self, p00, e0, e1, normal, mat, rng=None, ior=None):
        """corners p00, p00 + e0, p00 + e1, p00 + e0 + e1; vertex frames (normal, tangent, bitangent)"""
        p00, e0, e1 = (np.asarray(v, np.float64) for v in (p00, e0, e1))
        self.corners.append(np.stack([p00, p00 + e0, p00 + e1, p00 + e0 + e1]))
        self.frames.append(np.stack(_frame(normal, rng)))
        self.mats.append(mat)
        self.iors.append(mat.ior if ior is None else ior)
        return len(self.corners) - 1

    def slab(self, x0, z0, mat, rng):
        h = SLAB_THICKNESS
        first = self.quad([x0, 0, z0], [1, 0, 0], [0, 0, 1], [0, 1, 0], mat, rng)
        self.quad([x0, -h, z0], [1, 0, 0], [0, 0, 1], [0, -1, 0], mat, rng)
        self.quad([x0, -h, z0], [0, h, 0], [0, 0, 1], [-1, 0, 0], mat, rng)
        self.quad([x0 + 1, -h, z0], [0, h, 0], [0, 0, 1], [1, 0, 0], mat, rng)
        self.quad([x0, -h, z0], [1, 0, 0], [0, h, 0], [0, 0, -1], mat, rng)
        self.quad([x0, -h, z0 + 1], [1, 0, 0], [0, h, 0], [0, 0, 1], mat, rng)
        return first


def _bvh(lo, hi):
    """a median-split BVH over the quads in the reference layout (pre-order; an interior node's left child follows it),
    one quad per leaf"""
    nodes = []

    def build(ids):
        idx = len(nodes)
        nodes.append(None)
        blo, bhi = lo[ids].min(0), hi[ids].max(0)
        if len(ids) == 1:
            nodes[idx] = (0, 0, 2 * int(ids[0]), blo, bhi)
            return idx
        c = (lo[ids] + hi[ids]) / 2
        order = ids[np.argsort(c[:, np.argmax(c.max(0) - c.min(0))], kind="stable")]
        left = build(order[:len(ids) // 2])
        right = build(order[len(ids) // 2:])
        nodes[idx] = (left, right, -1, blo, bhi)
        return idx

    build(np.arange(len(lo)))
    bvh = np.zeros((len(nodes), 9), np.float32)
    for i, (a, b, c, blo, bhi) in enumerate(nodes):
        bvh.view(np.int32)[i, :3] = (a, b, c)
        bvh[i, 3:6], bvh[i, 6:9] = blo, bhi
    return bvh


TRI_CORNERS = ((0, 1, 2), (3, 2, 1))          # two right-isosceles triangles per quad, their legs along its edges


@functools.lru_cache(None)
def zoo(razor=TIR_RAZOR):
    """-> (SceneArrays, items): the zoo under the noise environment.  `razor`: the table of razor quads (TIR_RAZOR, or
    the candidates search_tir_razor is trying)"""
    from fspt_amd import scene as S
    b = Builder()
    items = []
    for part, cell0 in (("A", 0), ("B", PART_B_CELL0)):
        rng = None if part == "A" else np.random.default_rng(77)
        for k, mat in enumerate(MATERIALS):
            x0, z0 = cell_origin(cell0 + k)
            items.append(Item("quad", mat, part, cell0 + k, b.quad([x0, 0, z0], [1, 0, 0], [0, 0, 1], [0, 1, 0], mat, rng)))
        for k, name in enumerate(SLAB_MATERIALS):
            x0, z0 = cell_origin(cell0 + N_SINGLE + k)
            items.append(Item("slab", MATERIAL[name], part, cell0 + N_SINGLE + k, b.slab(x0, z0, MATERIAL[name], rng)))
    for k, row in enumerate(razor):
        x0, z0 = cell_origin(RAZOR_CELL0 + k)
        ior = float(np.array([row[0]], np.uint32).view(np.float32)[0])
        items.append(Item("razor", RAZOR, "R", RAZOR_CELL0 + k, b.quad([x0, 0, z0], [1, 0, 0], [0, 0, 1], [0, 1, 0], RAZOR, ior=ior)))
    xa, za = PITCH * GRID_W, PITCH * PART_ROWS
    b.quad([-1, -2, -1], [xa + 1, 0, 0], [0, 0, za + 1], [0, 1, 0], GLOWING)                    # the catcher under part A
    b.quad([-1, 3, -1], [xa / 2 + 0.5, 0, 0], [0, 0, za + 1], [0, -1, 0], GLOWING)              # the lid over its lower columns
    b.quad([13, 2.5, 4], [2, 0, 0], [0, 0, 2], [0, -1, 0], LAMP)                                # E1
    b.quad([13.5, 2.0, 4.5], [1, 0, 0], [0, 0, 1], [0, -1, 0], PLAIN)                           # its occluder
    x0, z0 = cell_origin(E2_CELL)
    b.quad([x0, 0, z0], [E2_LENGTH, 0, 0], [0, 0, 1], [0, 1, 0], LAMP)                          # E2, a strip in the plane y = 0
    b.quad([-4, 2.5, PITCH * (PART_ROWS + 2)], [1, 0, 0], [0, 0, 1], [0, -1, 0], DARK_LAMP)      # E3
    n = len(b.corners)
    corners = np.array(b.corners)
    tri = np.zeros((n, 2, 3, 3), np.float32); uv = np.zeros((n, 2, 3, 2), np.float32)
    norm = np.zeros((n, 2, 3, 3, 3), np.float32); mat = np.zeros((n, 2, 12), np.float32)
    corner_uv = LC.UV_LO + LC.UV_SPAN * np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float64)
    for q in range(n):
        for half, cs in enumerate(TRI_CORNERS):
            for v, c in enumerate(cs):
                tri[q, half, v], norm[q, half, v], uv[q, half, v] = corners[q, c], b.frames[q][c], corner_uv[c]
        m = b.mats[q]
        mat[q, :, [AC.MAT_DIFFUSE, AC.MAT_EMISSIVE, AC.MAT_NORMAL, AC.MAT_MR]] = np.array([m.diffuse, m.emissive, m.normal, m.mr], np.float32)[:, None]
        mat[q, :, AC.MAT_IOR], mat[q, :, AC.MAT_DIELECTRIC] = b.iors[q], m.dielectric
    w, h = ENV_SIZE
    env = LC.random_env(w, h)
    env[0], env[-1] = env[0, 0], env[-1, 0]          # at a pole the column is atan2 of two cancelled components: one texel there
    arrays = S.SceneArrays(bvh=_bvh(corners.min(1), corners.max(1)).reshape(-1), tri=tri.reshape(-1), mat=mat.reshape(-1),
                           norm=norm.reshape(-1), uv=uv.reshape(-1), atlas=atlas(), atlas_res=ATLAS_RES, atlas_layers=N_LAYERS,
                           env=np.ascontiguousarray(env).reshape(-1), env_w=w, env_h=h,
                           bins=np.array([0, 0, w, h], np.uint32), leaf_size=2)
    return arrays, tuple(items)


@functools.lru_cache(None)
def dim_zoo():
    """the zoo's geometry under DIM_BINS importance bins that each span a dim DIM_ENV_SIZE map: envPdf on both sides of
    EPSILON (sin phi above and below 0.77), the radiance small enough that colours stay below the clamp"""
    arrays, items = zoo()
    w, h = DIM_ENV_SIZE
    env = LC.random_env(w, h)
    env[..., 3] = DIM_EXPONENT
    return dataclasses.replace(arrays, env=np.ascontiguousarray(env).reshape(-1), env_w=w, env_h=h,
                               bins=np.tile(np.array([0, 0, w, h], np.uint32), DIM_BINS)), items


# ---- rays ------------------------------------------------------------------------------------------------------------
def _toward(points, dirs, t):
    """rays that reach `points` after distance t along `dirs` (unit)"""
    points, dirs = np.asarray(points, np.float64), np.asarray(dirs, np.float64)
    return np.concatenate([points - dirs * np.asarray(t, np.float64).reshape(-1, 1), dirs], 1)


def _polar(cos, phi, up=-1.0):
    """unit directions at cosine `cos` to the plane's normal and azimuth phi, heading down (up = -1) or up (+1)"""
    cos, phi = np.broadcast_arrays(np.asarray(cos, np.float64), np.asarray(phi, np.float64))
    s = np.sqrt(1 - cos * cos)
    return np.stack([s * np.cos(phi), up * cos, s * np.sin(phi)], -1)


SPECIAL_POINTS = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0.5, 0], [0, 0.5], [1, 0.5], [0.5, 1], [0.5, 0.5],
                           [1 / 3, 1 / 3], [2 / 3, 2 / 3]])       # corners, edge midpoints, the diagonal, the centroids
FAN_COS = (0.3, 0.15, 0.07, 0.02)


def item_rays(item):
    """the rays of one quad or slab, float64 [n, 6]"""
    rng = np.random.default_rng(500 + item.cell)
    x0, z0 = cell_origin(item.cell)
    at = lambda p: np.stack([x0 + p[:, 0], np.zeros(len(p)), z0 + p[:, 1]], 1)
    inner = lambda n: at(rng.uniform(0.06, 0.94, (n, 2)))
    down = np.array([0.0, -1.0, 0.0])
    long_t = (1e-3, 0.1, 1.0, 30.0, 300.0, 1e3) if item.part == "B" else (1e-3, 0.01, 0.1, 1.0, 2.0, 2.0)
    if item.kind == "razor":
        return np.zeros((0, 6))
    out = [_toward(inner(16), np.tile(down, (16, 1)), 1.0)]                                     # normal incidence, t = 1
    out.append(_toward(inner(6), _polar(np.sqrt(0.5), rng.uniform(0, 2 * np.pi, 6)), long_t))   # 45 degrees, t 1e-3 .. 1e3
    fan = np.repeat(FAN_COS, 8)
    out.append(_toward(inner(len(fan)), _polar(fan, rng.uniform(0, 2 * np.pi, len(fan))), 1.0)) # where Fresnel decides
    if item.kind == "quad":
        out.append(_toward(at(SPECIAL_POINTS), np.tile(down, (len(SPECIAL_POINTS), 1)), 1.0))
        out.append(_toward(inner(4), _polar([1e-3, 1e-3, 1e-6, 1e-6], rng.uniform(0, 2 * np.pi, 4)), [0.5, 1.0, 0.5, 1.0]))   # grazing
        out.append(_toward(inner(1), [[1.0, 0.0, 0.0]], 2.0))                                   # exactly tangent
        n = 6 if item.material.dielectric < 0 else 18               # from behind; inside a dielectric the distance is what absorbs
        out.append(_toward(inner(n), np.tile(-down, (n, 1)), np.resize([0.02, 0.05, 0.1, 0.2, 0.5, 1.0], n)))
        out.append(_toward(inner(3), _polar(np.sqrt(0.5), rng.uniform(0, 2 * np.pi, 3), 1.0), [0.01, 0.5, 1.0]))
    else:
        # from inside the slab, steep against the face they reach: beyond the critical angle of ior 1.5 (and of the micro
        # normals around it) on the bottom, the top and a side
        mid = inner(12) - [0.0, SLAB_THICKNESS / 2, 0.0]
        cos = np.array([0.9, 0.75, 0.6, 0.5, 0.35, 0.2] * 2)
        d = _polar(cos, rng.uniform(0, 2 * np.pi, 12), np.repeat([-1.0, 1.0], 6))
        out.append(np.concatenate([mid, d], 1))
    return np.concatenate(out)


@functools.lru_cache(None)
def zoo_rays():
    """-> (rays float32 [n, 6], item index of each ray): the zoo's rays, then TIR_RAZOR's"""
    _, items = zoo()
    rays = [item_rays(it).astype(np.float32) for it in items]
    which = [np.full(len(r), k) for k, r in enumerate(rays)]
    razor = np.array([row[1:] for row in TIR_RAZOR], np.uint32).reshape(-1, 6).view(np.float32)
    first = next((k for k, it in enumerate(items) if it.kind == "razor"), len(items))
    return np.concatenate(rays + [razor]), np.concatenate(which + [first + np.arange(len(razor))])


@functools.lru_cache(None)
def dim_rays():
    """every third of the normal-incidence and 45-degree rays of the opaque quads whose normal map leaves the tangent plane
    (a tangent-plane normal under normal incidence is the ill-conditioned grazing reflection): enough for both sides of
    envPdf <= EPSILON"""
    _, items = zoo()
    rays, which = zoo_rays()
    keep = np.zeros(len(rays), bool)
    for k, it in enumerate(items):
        if it.kind == "quad" and it.material.dielectric < 0 and it.material.metallic in (0, 128) and it.material.normal != Z0:
            keep[np.flatnonzero(which == k)[:22:3]] = True
    return rays[keep], which[keep]


def permutation(n):
    """a fixed shuffle of a frame's n rays: every wave then holds quads of every kind"""
    return np.random.default_rng(4242).permutation(n)


# a camera that sees both parts of the zoo (the tile-list instantiations shade camera rays)
CAMERA = dict(P=[14.0, 9.0, 33.0], I=[0.0, -0.45, -1.0], fov_scale=0.8, env_theta=ENV_THETA, focal_depth=2.0, aperture=0.0)
CAMERA_FRAME = (64, 48)
# ... and one straight above it, for the first hits alone: every quad that the lid does not hide
OVERHEAD = dict(P=[14.0, 45.0, 20.0], I=[0.0, -1.0, -0.05], fov_scale=0.5, env_theta=ENV_THETA, focal_depth=2.0, aperture=0.0)
OVERHEAD_FRAME = (128, 96)

# ---- the running mean ------------------------------------------------------------------------------------------------
ACC_TICKS = (0, 1, 2, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 31, 0xFFFFFFFF)
ACC_FRAME = (8, 8)


def search_tir_razor(want=24, n_candidates=60000, seed=9):
    """How TIR_RAZOR was found (seconds on a CPU; prints the table).  Candidate rays from behind onto a RAZOR quad at
    15..25 degrees to its normal; of those whose specular coin - the sixth rnd() of the vertex - is above 0.9992, the
    float32 iors around the critical 1 / sin(theta) of the ray's own micro normal are tried in the oracle until one
    gives refracted with rd = 0.  The table hangs on the sixth rnd() of each vertex, and so on the float32 sin() of the
    oracle's math: where that differs the census (test_shade_cpu.py) fails on "refract: kk < 0" - it cannot pass with the
    branch lost - and the table is to be regenerated with this function."""
    import oracle as O
    rng = np.random.default_rng(seed)
    found = []
    arrays, items = zoo(tuple((np.float32(3.0).view(np.uint32).item(),) + (0,) * 6 for _ in range(want)))
    arrays = dataclasses.replace(arrays, mat=arrays.mat.copy())        # the iors are tried on a copy: the cached zoo stays as built
    mat = arrays.mat.reshape(-1, 12)
    for it in (it for it in items if it.kind == "razor"):          # one ray per quad: the ior is the quad's
        x0, z0 = cell_origin(it.cell)
        n, quad, hit = n_candidates, it.first_quad, None
        while hit is None:
            p = np.stack([x0 + rng.uniform(0.1, 0.9, n), np.zeros(n), z0 + rng.uniform(0.1, 0.9, n)], 1)
            rays = _toward(p, _polar(np.cos(np.radians(rng.uniform(15, 25, n))), rng.uniform(0, 2 * np.pi, n), 1.0), 1.0).astype(np.float32)
            t, index, _, _ = O.intersect(arrays, rays)
            b = O.bounce_probe(arrays, rays, t, index, RAND_BASE, ENV_THETA)
            coin = O.rnd_sequence(b[:, 0], 6)[:, 5]
            for i in np.flatnonzero((index // 2 == quad) & (coin > 0.9992)):
                c = float(np.dot(b[i, 28:31].astype(np.float64), -rays[i, 3:].astype(np.float64)))
                cand = [np.float32(1.0 / np.sqrt(1.0 - c * c))]
                for _ in range(40):
                    cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(9))]
                for ior in cand:
                    mat[2 * quad:2 * quad + 2, AC.MAT_IOR] = ior
                    r = O.bounce_probe(arrays, rays[i:i + 1], t[i:i + 1], index[i:i + 1], RAND_BASE, ENV_THETA)[0]
                    if r[23] == 1 and not r[4:7].any():
                        hit = (np.float32(ior).view(np.uint32).item(),) + tuple(int(v) for v in rays[i].view(np.uint32))
                        break
                if hit is not None:
                    break
        found.append(hit)
    print("TIR_RAZOR = (\n" + "".join("    (%s),\n" % ", ".join("0x%08x" % v for v in row) for row in found) + ")")
    return found


# ---- the oracle's vertices and their float64 restatement, computed once ------------------------------------------------
@functools.lru_cache(None)
def scene(name):
    """-> (arrays, items, rays, item of each ray) of scene "zoo" or "dim" """
    return (zoo() + zoo_rays()) if name == "zoo" else (dim_zoo() + dim_rays())


def env_q(fraction):
    """q as the host sets it under an environment map: the emitter fraction capped at FSPT_LIGHTS_ENV_Q_MAX"""
    return float(min(np.float32(fraction), np.float32(0.875)))


@functools.lru_cache(None)
def host_light_table(name="zoo"):
    """The scene's light table built without a device: the triangles of positive weight (oracle.light_weights, what
    k_light_weights computes), their alias table (fspt_light_alias_table, a host function) and light_p as the host
    realises it -> (table for oracle.olights, pick per triangle)"""
    import oracle as O
    from fspt_amd import light_alias_table
    arrays = scene(name)[0]
    w = O.light_weights(arrays, np.arange(arrays.tri.size // 9))
    tris = np.flatnonzero(w > 0).astype(np.uint32)
    prob, alias = light_alias_table(w[tris])
    light_p = O.realised_p(prob, alias)
    pick = np.zeros(len(w), np.float32)
    pick[tris] = light_p
    return {"tris": tris, "prob": prob, "alias": alias, "light_p": light_p}, pick


def oracle_frame(arrays, rays, num_bounces, lights=None, tick=0, accum=None):
    """one oracle sample of the injected rays -> (radiance float32 [n, 3], first-hit records [n])"""
    import oracle as O
    pos, d = LC.frame(rays)
    acc = np.zeros(pos.shape, np.float32) if accum is None else accum
    fh = O.trace(arrays, pos.shape[1], pos.shape[0], pos, d, tick, RAND_BASE, ENV_THETA, num_bounces, acc, first_hits=True, lights=lights)
    return acc.reshape(-1, 4)[:len(rays), :3].copy(), fh[:len(rays)]


class Vertices:
    """The first vertex of every ray of a scene that hits: the oracle's bounce_probe record, the random numbers it drew, the
    results of its two rays, and shade_ref's float64 vertex under the oracle's decisions"""

    def __init__(self, name):
        import oracle as O
        import shade_ref as SR
        self.arrays, self.items, all_rays, all_which = scene(name)
        self.colour, fh = oracle_frame(self.arrays, all_rays, 1)
        self.hit = fh["index"] >= 0
        self.all_rays = all_rays
        self.rays, self.which, self.t, self.index = all_rays[self.hit], all_which[self.hit], fh["t"][self.hit], fh["index"][self.hit]
        b = O.bounce_probe(self.arrays, self.rays, self.t, self.index, RAND_BASE, ENV_THETA)
        self.rnd = O.rnd_sequence(b[:, 0], 12)
        self.inside, self.specular, self.refracted = b[:, 1] != 0, b[:, 2] != 0, b[:, 23] != 0
        self.tir = self.refracted & ~b[:, 4:7].any(1)
        self.got = dict(micro_normal=b[:, 28:31], rd=b[:, 4:7], ro=b[:, 8:11], bsdf_pdf=b[:, 3], env_pdf=b[:, 19],
                        bsdf_throughput=b[:, 12:15], env_throughput=b[:, 16:19], weights=b[:, [7, 11]])
        self.env_dir, self.cos_env, self.dielectric, self.normal = b[:, 20:23], b[:, 15], b[:, 35], b[:, 32:35]
        self.next_index, self.next_t = b[:, 39].astype(np.int32), b[:, 43]
        self.has_shadow = (self.dielectric < 0) & (self.cos_env > 0)
        self.shadow_missed = O.intersect(self.arrays, np.concatenate([b[:, 8:11], b[:, 20:23]], 1))[1] < 0
        self.extension_missed = self.next_index < 0
        self.material = np.array([self.items[k].material.name for k in self.which])
        self.ref = SR.vertex(self.arrays, self.rays, self.t, self.index, self.rnd, self.specular, self.inside, self.tir, ENV_THETA)
        self.ref_colour = SR.colour_one_bounce(self.arrays, self.ref, self.shadow_missed, self.extension_missed, ENV_THETA)
        self.miss_colour = SR.env_radiance(self.arrays, all_rays[~self.hit, 3:], ENV_THETA)
        self.sharp = self.specular & (self.ref["rough"] <= 0.001)

    def exempt(self):
        """Where the float64 value itself shows ill-conditioning - each condition by name -> bool [n]"""
        r = self.ref
        with np.errstate(invalid="ignore"):
            near = lambda x, at: np.abs(x - at) <= 2.0 ** -23 * abs(at)
            return {
                # gtr2's t = 1 + (a^2 - 1) ndh^2 has cancelled to within a thousandth of its floor a^2 = 1e-6: one float32
                # rounding of its terms, 6e-8, is 6 % of it
                "gtr2_t_cancelled": self.specular & (r["gtr2_t"] <= 1.001e-6),
                # gtr2Pdf divides by |dot(bsdfDir, h)| with h = normalize(bsdfDir + incident): a grazing reflection, where the
                # sum cancels before it is normalised
                "rd_dot_h_small": self.specular & (r["rd_dot_h"] < RD_DOT_H_MIN),
                # sampleEnv divides by sin phi: a direction at a pole of the map
                "sin_phi_small": np.abs(r["sin_phi"]) < SIN_PHI_MIN,
                # misWeights' EPSILON and the frame's |n.z| < 0.999, decided within one float32 ulp
                "decision_within_an_ulp": near(r["env_pdf"], EPSILON) | near(r["bsdf_pdf"], EPSILON) | near(np.abs(r["normal"][:, 2]), 0.999),
            }

    def any_exempt(self):
        return np.logical_or.reduce(list(self.exempt().values()))


@functools.lru_cache(None)
def vertices(name):
    return Vertices(name)


class LightVertices:
    """The zoo's first vertices as vertices of a path of four bounces at one emitter fraction: the oracle's
    light_vertex_probe and emission_weight_probe against shade_ref's emitter arm under the oracle's decisions"""

    def __init__(self, fraction):
        import oracle as O
        import shade_ref as SR
        V = self.V = vertices("zoo")
        self.table, self.pick = host_light_table()
        self.q = q = env_q(fraction)
        v = self.v = O.light_vertex_probe(V.arrays, (self.table, q), V.rays, V.t, V.index, rec=None, rand_base=RAND_BASE,
                                           env_theta=ENV_THETA, bounce=0, num_bounces=4)
        self.strategy = v["strategy"].astype(int)
        self.emitter, self.environment = self.strategy == 2, self.strategy == 1
        e = np.flatnonzero(self.emitter)
        sub = {k: a[e] for k, a in V.ref.items()}
        self.ref_emitter = SR.emitter_vertex(V.arrays, sub, self.table, q, v["entry"][e], v["u"][e])
        n = len(V.rays)
        self.ref_sc, self.ref_pend = np.zeros(n), np.zeros((n, 3))
        sc, pend = SR.environment_strategy(V.ref, q)
        self.ref_sc[self.environment], self.ref_pend[self.environment] = sc[self.environment], pend[self.environment]
        self.ref_sc[e], self.ref_pend[e] = self.ref_emitter["sc"], self.ref_emitter["pend"]
        self.ref_lq = np.where(self.strategy > 0, SR.lq(V.ref, q), 0.0)
        # the emission the extension ray finds, weighted against this vertex's emitter sampling
        self.ext = np.flatnonzero(~V.extension_missed)
        self.emw = O.emission_weight_probe(V.arrays, (self.table, q), v["lq"][self.ext], V.got["rd"][self.ext], V.next_t[self.ext], V.next_index[self.ext])
        self.ref_emw = SR.emission_weight(V.arrays, self.pick, self.ref_lq[self.ext], V.ref["rd"][self.ext], V.next_t[self.ext], V.next_index[self.ext])

    def exempt(self):
        """-> bool [n]: the vertex's own exemptions, and for an emitter sample those of its direction w"""
        out = self.V.any_exempt().copy()
        e = np.flatnonzero(self.emitter)
        r = self.ref_emitter
        sp = self.V.specular[e]
        out[e] |= (sp & (r["gtr2_t"] <= 1.001e-6)) | (sp & (r["w_dot_h"] < RD_DOT_H_MIN))
        return out


@functools.lru_cache(None)
def light_vertices(fraction):
    return LightVertices(fraction)


def deviation(got, ref):
    """lookup_cases.deviation per case over the cases where both are finite; where only one of them is, infinite; where
    neither is (the same overflow, the same 0 / 0), zero"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if len(got) == 0:
        return np.zeros(1)
    fg, fr = (np.isfinite(a).reshape(len(a), -1).all(1) for a in (got, ref))
    dev = np.where(fg != fr, np.inf, 0.0)
    both = fg & fr
    if both.any():
        dev[both] = LC.deviation(got[both], ref[both])
    return dev


# ---- the running mean: one 8 x 8 frame -----------------------------------------------------------------------------------
@functools.lru_cache(None)
def acc_scene():
    """The zoo's geometry under a map whose right half is bright beyond what float32 holds once a throughput above 2 multiplies it (exponent byte
    255: 2^127) and two importance bins - the map, and as many rows below it, where sin phi and with it envPdf are negative
    (the host takes the bins as they come): sample colours above 1024, infinite, NaN and negative occur."""
    arrays, items = zoo()
    w, h = 8, 4
    env = LC.random_env(w, h)
    env[:, w // 2:, 3] = 255
    return dataclasses.replace(arrays, env=np.ascontiguousarray(env).reshape(-1), env_w=w, env_h=h,
                               bins=np.array([0, 0, w, h, 0, h, w, 2 * h], np.uint32))


@functools.lru_cache(None)
def acc_frame():
    """-> (rays float32 [64, 6], the oracle's sample colour before the clamp [64, 3], class of each pixel): of the zoo's
    rays in acc_scene, the first (up to eight) whose one-vertex sample is NaN, +inf, negative and above 1024, ordinary ones
    up to forty in all, twelve that miss into the dim half of the map and twelve into the bright one"""
    import oracle as O
    arrays = acc_scene()
    rays = zoo_rays()[0]
    t, index, _, _ = O.intersect(arrays, rays)
    b = O.bounce_probe(arrays, rays, t, index, RAND_BASE, ENV_THETA)
    c = b[:, 36:39]
    one_vertex = (index >= 0) & ((b[:, 23] == 0) | (b[:, 39] < 0))          # a refracted ray that hits goes on
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(c).all(1)
        classes = {"nan": np.isnan(c).any(1), "inf": np.isposinf(c).any(1) & ~np.isnan(c).any(1), "negative": finite & (c < 0).any(1),
                   "above": finite & (c > 1024).any(1) & (c >= 0).all(1), "ordinary": finite & (c > 0).all(1) & (c < 1024).all(1)}
    pick, kind = [], []
    for k, m in classes.items():
        i = np.flatnonzero(m & one_vertex)[:8 if k != "ordinary" else 40 - len(pick)]
        assert len(i) >= 1, k
        pick += i.tolist(); kind += [k] * len(i)
    assert len(pick) == 40
    up = _polar(0.5, np.linspace(0.1, 6.2, 48), 1.0)
    miss = np.concatenate([np.tile(LC.MISS_RAY[:3], (len(up), 1)), up], 1).astype(np.float32)
    pos, d = LC.frame(miss)
    acc = np.zeros(pos.shape, np.float32)
    O.trace(arrays, 64, 1, pos, d, 0, RAND_BASE, ENV_THETA, 0, acc)
    seen = acc.reshape(-1, 4)[:len(miss), :3]
    dim, bright = np.flatnonzero((seen < 1024).all(1))[:12], np.flatnonzero((seen >= 1024).any(1))[:12]
    assert len(dim) == 12 and len(bright) == 12, (len(dim), len(bright))
    out = np.concatenate([rays[pick], miss[dim], miss[bright]])
    return out, np.concatenate([c[pick], seen[dim], seen[bright]]), tuple(kind + ["miss_dim"] * 12 + ["miss_bright"] * 12)


def acc_preload():
    """accumulator values across [0, 1024], one row of the frame per decade"""
    rng = np.random.default_rng(8)
    a = np.ones((8, 8, 4), np.float32)
    a[..., :3] = (rng.uniform(0.5, 1.0, (8, 8, 3)) * np.array([0.0, 1e-6, 1e-3, 0.1, 1.0, 10.0, 100.0, 1024.0])[:, None, None]).astype(np.float32)
    return a


def acc_frame_arrays():
    """(pos, dir) float32 [8, 8, 4] of acc_frame's rays"""
    rays = acc_frame()[0]
    pos = np.ones((8, 8, 4), np.float32); d = np.ones((8, 8, 4), np.float32)
    pos[..., :3], d[..., :3] = rays[:, :3].reshape(8, 8, 3), rays[:, 3:].reshape(8, 8, 3)
    return pos, d
