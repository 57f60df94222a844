"""numpy float64 restatement of the emitter light table and the emitter sample (fspt_target_set_lights) for
scenes whose emissive and diffuse layers are flat colours, and the test scenes of tests/test_lights_*.py."""
import numpy as np

LUMA = np.array([0.2126, 0.7152, 0.0722])

# a quad in the y = 0 plane whose group uses an MTL material (`kem`: the flat emissive colour of the emitter)
LAMP_OBJ = "\n".join(["mtllib lamp.mtl", "v 0.5 0.0 0.5", "v 0.5 0.0 -0.5", "v -0.5 0.0 -0.5", "v -0.5 0.0 0.5", "",
                      "vt 0.0 0.0", "vt 0.0 1.0", "vt 1.0 1.0", "vt 1.0 0.0", "", "usemtl lamp",
                      "f 1/1 3/3 2/2", "f 3/3 1/1 4/4", ""])
LAMP_MTL = "newmtl lamp\nkd 1 1 1\nkem 0.6 0.55 0.45\n"


def scene_e1():
    """E1: floor, back wall, a small flat-colour emitter under the ceiling whose back edge touches the wall, a dielectric
    sphere (the refraction branch) and no environment map."""
    from fspt_amd import scene as S
    props = [
        {"path": "synthetic/quad.obj", "scale": 4, "rotate": [], "translate": [0, -0.75, 0], "emittance": [0, 0, 0],
         "diffuse": [0.6, 0.6, 0.6], "metallicRoughness": [0, 0.5, 0], "normals": "flat"},
        {"path": "synthetic/quad.obj", "scale": 4, "rotate": [{"angle": -1.5707964, "axis": [1, 0, 0]}],
         "translate": [0, 0.25, -1], "emittance": [0, 0, 0], "diffuse": [0.5, 0.55, 0.6],
         "metallicRoughness": [0, 0.4, 0], "normals": "flat"},
        {"path": "synthetic/lamp.obj", "scale": 0.5, "rotate": [], "translate": [0.0, 0.45, -0.75], "emittance": [1, 1, 1],
         "normals": "flat"},
        {"path": "synthetic/cube_sphere.obj", "scale": 0.25, "rotate": [], "translate": [0.35, -0.5, -0.2],
         "diffuse": [0.95, 0.95, 0.95], "emittance": [0, 0, 0], "metallicRoughness": [0, 0.1, 0], "normals": "smooth",
         "ior": 1.4, "dielectric": 0.2},
    ]
    texts = {"synthetic/quad.obj": S.QUAD_OBJ, "synthetic/lamp.obj": LAMP_OBJ, "synthetic/cube_sphere.obj": S.cube_sphere_obj(5)}
    s = S.build_scene(props, texts, mtl_texts={"synthetic/lamp.mtl": LAMP_MTL})
    s.meta = dict(kind="E1")
    return s


def scene_e2():
    """E2: textured_test_scene - its emission map lights part of one quad; it has an environment map (q < 1)."""
    from fspt_amd import scene as S
    return S.textured_test_scene()


def flat_texel(arrays, layer_id):
    """The RGB of a flat-colour atlas layer (any texel), as unorm8 / 255 in float64."""
    L = int(np.clip(np.floor(np.float32(layer_id) + np.float32(0.5)), 0, arrays.atlas_layers - 1))
    n = arrays.atlas_res * arrays.atlas_res * 4
    return arrays.atlas[L * n: L * n + 3].astype(np.float64) / 255.0


def tri_geometry(arrays):
    t = arrays.tri.reshape(-1, 3, 3).astype(np.float64)  # v1, v2, v3
    return t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]


def flat_le(arrays):
    """Le = 30 * emissive * diffuse per triangle (flat-colour layers)."""
    mat = arrays.mat.reshape(-1, 12)
    return np.array([30.0 * flat_texel(arrays, m[1]) * flat_texel(arrays, m[0]) for m in mat])


def flat_weights(arrays):
    """w_i = A_i * luma(Le_i): the mean over the 16 points of a flat-colour triangle is its one value."""
    _, e1, e2 = tri_geometry(arrays)
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    return area * (flat_le(arrays) @ LUMA)


def realised(prob, alias):
    """Probability of each entry under the stored float32 table, in float64: (prob_i + sum_{alias_j = i} (1 - prob_j)) / n."""
    prob = prob.astype(np.float64)
    n = prob.size
    r = prob.copy()
    moved = np.arange(n) != alias
    np.add.at(r, alias[moved], 1.0 - prob[moved])
    return r / n


def pick_entry(prob, alias, u1):
    """The device's alias lookup, in float32."""
    n = prob.size
    fn = np.float32(u1) * np.float32(n)
    i = np.minimum(fn.astype(np.int64), n - 1)
    coin = fn - i.astype(np.float32)
    return np.where(coin < prob[i], i, alias[i])


def sample(arrays, table, q):
    """The emitter sample for queries q [n, 10] (ro, n, u0..u3) of a flat-colour scene: (tri, point, pdf_L, Le, n . w)."""
    e = pick_entry(table["prob"], table["alias"], q[:, 7])
    tri = table["tris"][e].astype(np.int64)
    v1, e1, e2 = tri_geometry(arrays)
    u2, u3 = q[:, 8].astype(np.float64), q[:, 9].astype(np.float64)
    su = np.sqrt(u2)
    b1, b2 = u3 * su, su - u3 * su
    x = v1[tri] + e1[tri] * b1[:, None] + e2[tri] * b2[:, None]
    d = x - q[:, 0:3].astype(np.float64)
    d2 = (d * d).sum(1)
    w = d / np.sqrt(d2)[:, None]
    cr = np.cross(e1[tri], e2[tri])
    pdf = realised(table["prob"], table["alias"])[e] * d2 * 2.0 / np.abs((cr * w).sum(1))
    return tri, x, pdf, flat_le(arrays)[tri], (q[:, 3:6].astype(np.float64) * w).sum(1)
