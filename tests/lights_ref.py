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


def alias_v(u0, u1, q):
    """The alias draw of an emitter sample, v = fract(u1 + (u0 / q) 2^-8), in float32: given u0 < q, u0 / q is uniform
    and fills in the bits below rnd()'s resolution."""
    f = np.float32
    x = np.asarray(u1, f) + (np.asarray(u0, f) / f(q)) * f(2.0 ** -8)  # (the product is exact: one rounding, as the fma)
    return (x - np.floor(x)).astype(f)


def pick_entry(prob, alias, u1):
    """The device's alias lookup for the alias draw u1 (slot floor(u1 n), coin its fraction), in float32."""
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


# ---- E3: flat colours, an environment map, a light table that moves mass ------------------------------------------------
def _emitter_obj(name):
    """LAMP_OBJ's quad with material `name` from e3.mtl."""
    return LAMP_OBJ.replace("mtllib lamp.mtl", "mtllib e3.mtl").replace("usemtl lamp", "usemtl " + name)


def _e3_strip():
    """16 small emitters along the back wall: (scale, kem) spanning more than four decades of A * luma(Le)."""
    out = []
    for k in range(16):
        s = 0.04 + 0.014 * k                     # area 0.0016 .. 0.06
        lvl = [1, 2, 4, 9, 20, 40, 90, 160, 255][k % 9] / 255.0  # emission 1/255 .. 1
        kem = [lvl, lvl * (0.5 + 0.03 * k), lvl * 0.3] if k % 3 else [lvl * 0.4, lvl * 0.7, lvl]
        out.append((s, kem))
    return out


def scene_e3():
    """E3: a flat-colour scene with an environment map (both NEE strategies run): a Lambert floor, a metallic = 1 floor
    patch at low roughness, a metallic = 0.5 back wall, the ceiling lamp with an occluder below it, an emitter standing
    perpendicular to the floor, two emitters facing each other, 16 small emitters on the wall whose weights span more than
    four decades (40 emitter triangles; the alias table moves mass) and the dielectric sphere."""
    from fspt_amd import scene as S
    h = 1.5707964
    quad = lambda **kw: dict({"path": "synthetic/quad.obj", "rotate": [], "emittance": [0, 0, 0], "normals": "flat"}, **kw)
    props = [
        quad(scale=4, translate=[0, -0.75, 0], diffuse=[0.6, 0.6, 0.6], metallicRoughness=[0, 0.5, 0]),
        quad(scale=4, rotate=[{"angle": -h, "axis": [1, 0, 0]}], translate=[0, 0.25, -1], diffuse=[0.5, 0.55, 0.6],
             metallicRoughness=[0.5, 0.4, 0]),
        quad(scale=0.8, translate=[-0.45, -0.745, -0.25], diffuse=[0.9, 0.8, 0.6], metallicRoughness=[1, 0.25, 0]),
        quad(scale=0.35, translate=[0.0, 0.2, -0.7], diffuse=[0.4, 0.4, 0.4], metallicRoughness=[0, 0.7, 0]),  # occluder
        {"path": "synthetic/lamp.obj", "scale": 0.5, "rotate": [], "translate": [0.0, 0.45, -0.75], "emittance": [1, 1, 1],
         "normals": "flat"},
        {"path": "synthetic/e3_side.obj", "scale": 0.3, "rotate": [{"angle": h, "axis": [0, 0, 1]}],
         "translate": [0.75, -0.58, -0.35], "emittance": [1, 1, 1], "normals": "flat"},  # perpendicular to the floor
        {"path": "synthetic/e3_pair.obj", "scale": 0.2, "rotate": [{"angle": h, "axis": [0, 0, 1]}],
         "translate": [-0.95, -0.35, -0.55], "emittance": [1, 1, 1], "normals": "flat"},
        {"path": "synthetic/e3_pair.obj", "scale": 0.2, "rotate": [{"angle": h, "axis": [0, 0, 1]}],
         "translate": [-0.65, -0.35, -0.55], "emittance": [1, 1, 1], "normals": "flat"},  # the two see each other
        {"path": "synthetic/cube_sphere.obj", "scale": 0.25, "rotate": [], "translate": [0.35, -0.5, -0.2],
         "diffuse": [0.95, 0.95, 0.95], "emittance": [0, 0, 0], "metallicRoughness": [0, 0.1, 0], "normals": "smooth",
         "ior": 1.4, "dielectric": 0.2},
    ]
    mtl = ["newmtl side", "kd 1 1 1", "kem 0.35 0.5 0.6", "newmtl pair", "kd 1 1 1", "kem 0.5 0.3 0.2"]
    texts = {"synthetic/quad.obj": S.QUAD_OBJ, "synthetic/lamp.obj": LAMP_OBJ, "synthetic/cube_sphere.obj": S.cube_sphere_obj(5),
             "synthetic/e3_side.obj": _emitter_obj("side"), "synthetic/e3_pair.obj": _emitter_obj("pair")}
    wall_rot = [{"angle": -h, "axis": [1, 0, 0]}]
    for k, (s, kem) in enumerate(_e3_strip()):
        mtl += ["newmtl s%d" % k, "kd 1 1 1", "kem %r %r %r" % tuple(kem)]
        texts["synthetic/e3_s%d.obj" % k] = _emitter_obj("s%d" % k)
        props.append({"path": "synthetic/e3_s%d.obj" % k, "scale": s, "rotate": wall_rot,
                      "translate": [-1.1 + 0.14 * k, -0.1 + 0.1 * (k % 4), -0.99], "emittance": [1, 1, 1], "normals": "flat"})
    env, w, h_ = S.synthetic_env(64, 32, sun_deg=6.0, sun_gain=6.0)
    s = S.build_scene(props, texts, env=env, env_w=w, env_h=h_, mtl_texts={"synthetic/e3.mtl": "\n".join(mtl) + "\n",
                                                                               "synthetic/lamp.mtl": LAMP_MTL})
    s.meta = dict(kind="E3")
    return s


def host_table(arrays):
    """The light table of a flat-colour scene built without a device: entries = triangles with flat_weights > 0, the alias
    table of their float32 weights (fspt_light_alias_table), light_p as the host realises it."""
    from fspt_amd import light_alias_table
    import oracle as O
    w = flat_weights(arrays)
    tris = np.nonzero(w > 0)[0].astype(np.uint32)
    prob, alias = light_alias_table(w[tris].astype(np.float32))
    return {"tris": tris, "prob": prob, "alias": alias, "light_p": O.realised_p(prob, alias)}


def device_table(t):
    """Scene.light_table() as the oracle takes it: light_p[e] = the pick of entry e's triangle (per leaf slot on the device)."""
    T = t["weights"].size
    tri_pick = np.zeros(T, np.float32)
    ok = t["slot_tri"] < T
    tri_pick[t["slot_tri"][ok]] = t["pick"][ok]
    return {"tris": t["tris"].astype(np.uint32), "prob": t["prob"], "alias": t["alias"], "light_p": tri_pick[t["tris"]]}


def env_q(arrays, fraction):
    """q as the host sets it: the emitter fraction capped at FSPT_LIGHTS_ENV_Q_MAX = 0.875 with an environment map, else 1."""
    return float(min(np.float32(fraction), np.float32(0.875))) if arrays.env is not None else 1.0


# ---- float64 restatement of one q > 0 vertex (DESIGN 8.3's formulas) -------------------------------------------------
def ggx_d(cos_h, a):
    a2 = a * a
    return a2 / (np.pi * ((a2 - 1.0) * cos_h * cos_h + 1.0) ** 2)


def smith_g(ndv, alpha_g):
    a, b = alpha_g * alpha_g, ndv * ndv
    return 1.0 / (ndv + np.sqrt(a + b - a * b))


def lobe(specular, n, wo, w, rho, metallic, rough):
    """(f, pdf_B) of the chosen lobe for outgoing wo (= incident), incoming w; float64, [k, 3] arrays."""
    dot = lambda a, b: (a * b).sum(-1)
    cn = dot(n, w)
    f_l = rho / np.pi
    pdf_l = np.abs(cn) / np.pi
    h = w + wo
    h /= np.linalg.norm(h, axis=-1, keepdims=True)
    a = np.maximum(0.001, rough)
    nh = dot(n, h)
    D = ggx_d(nh, a)
    pdf_s = D * np.abs(nh) / (4.0 * np.abs(dot(w, h)))
    rg = (0.5 * rough + 0.5) ** 2
    G = smith_g(cn, rg) * smith_g(dot(n, wo), rg)
    Fs = rho * metallic[:, None] + (1.0 - metallic)[:, None]
    f_s = (G * D)[:, None] * Fs
    sp = specular[:, None] > 0
    return np.where(sp, f_s, f_l), np.where(specular > 0, pdf_s, pdf_l)


def emitter_vertex(arrays, table, q, v):
    """The emitter strategy of vertices v (O.light_vertex_probe's fields, throughput 1) restated in float64: entry, point,
    pdf_L = p_e dist^2 / (A |n_g . w|), pdf_B, w_L = (q pdf_L)^2 / ((q pdf_L)^2 + pdf_B^2), contribution
    f Le max(n . w, 0) w_L / (q pdf_L) and the shadow bound dist (1 - 1e-4).  Flat-colour emitters."""
    f64 = lambda a: np.asarray(a, np.float64)
    u = v["u"]
    e = pick_entry(table["prob"], table["alias"], alias_v(u[:, 0], u[:, 1], q))
    tri = table["tris"][e].astype(np.int64)
    v1, e1, e2 = tri_geometry(arrays)
    su = np.sqrt(f64(u[:, 2]))
    b1, b2 = f64(u[:, 3]) * su, su - f64(u[:, 3]) * su
    x = v1[tri] + e1[tri] * b1[:, None] + e2[tri] * b2[:, None]
    d = x - f64(v["ro"])
    dist = np.linalg.norm(d, axis=1)
    w = d / dist[:, None]
    ng = np.cross(e1[tri], e2[tri])
    area = 0.5 * np.linalg.norm(ng, axis=1)
    cos_l = np.abs((ng * w).sum(1)) / (2.0 * area)
    p_e = realised(table["prob"], table["alias"])[e]
    pdf_L = p_e * dist * dist / (area * cos_l)
    n, wo = f64(v["normal"]), f64(v["incident"])
    f, pdf_B = lobe(f64(v["specular"]), n, wo, w, f64(v["diffuse"]), f64(v["metallic"]), f64(v["rough"]))
    w_L = (q * pdf_L) ** 2 / ((q * pdf_L) ** 2 + pdf_B ** 2)
    cn = (n * w).sum(1)
    contrib = f * flat_le(arrays)[tri] * (np.maximum(cn, 0.0) * w_L / (q * pdf_L))[:, None]
    return dict(entry=e, tri=tri, x=x, w=w, dist=dist, pdf_L=pdf_L, pdf_B=pdf_B, w_L=w_L, cn=cn, contrib=contrib,
                lt=dist * (1.0 - 1e-4), cos_l=cos_l)


def q_rule(v, q, bounce, num_bounces, n_lights=1, max_iters=64):
    """DESIGN 8.3's q rules for probe vertices: q where the extension ray's hit is shaded, outside a non-dielectric, on the
    Lambert lobe or the specular lobe at metallic = 1, with a non-empty table; 0 elsewhere."""
    lobe_ok = (v["specular"] == 0) | (v["metallic"] >= 1.0)
    ok = lobe_ok & (v["inside"] == 0) & (v["dielectric"] < 0) & (bounce + 1 < num_bounces) & (bounce + 1 < max_iters)
    return np.where(ok & (n_lights > 0), q, 0.0)
