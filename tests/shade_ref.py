"""One shading vertex in plain numpy float64: the formulas of the reference's tracer.fs (194-298: misWeights, gtr2, smithG,
gtr2Pdf, lambertPdf, sampleMicrofacet, sampleLambert, evalSpecular, evalLambert; 421-434: sampleEnv; 447-512: one
iteration of the bounce loop) and, for the emitter arm, of DESIGN 8.3.  Written from the shader's mathematics with the
exact pi, not from the oracle or the kernels: no fma, no float32 constant, no evaluation order of theirs.

The inputs are the hit record, the scene's arrays, the random numbers the vertex drew and its discrete decisions - the
specular coin, `inside`, total internal reflection, the strategy and the table entry of an emitter sample.  Those are
discontinuities, not arithmetic: the reference follows them and returns the continuous outputs."""
import numpy as np

import lookup_ref as LR

EPSILON = 0.000001
LIGHT_T_SCALE = 1.0 - 1.0e-4


def dot(a, b):
    return (a * b).sum(-1)


def unit(v):
    return v / np.sqrt(dot(v, v))[..., None]


def col(x):
    return np.asarray(x, np.float64)[..., None]


def mis_weights(a, b):
    """misWeights: the power heuristic, (1, 0) unless both pdfs are above EPSILON"""
    both = (a > EPSILON) & (b > EPSILON)
    with np.errstate(all="ignore"):
        a2, b2 = a * a, b * b
        return np.where(both, a2 / (a2 + b2), 1.0), np.where(both, b2 / (a2 + b2), 0.0)


def gtr2(ndh, a):
    a2 = a * a
    t = 1.0 + (a2 - 1.0) * ndh * ndh
    return a2 / (np.pi * t * t), t


def smith_g(ndv, alpha_g):
    a, b = alpha_g * alpha_g, ndv * ndv
    return 1.0 / (ndv + np.sqrt(a + b - a * b))


def gtr2_pdf(incident, normal, rough, w):
    h = unit(w + incident)
    cos_h = np.abs(dot(h, normal))
    return gtr2(cos_h, np.maximum(0.001, rough))[0] * cos_h / (4.0 * np.abs(dot(w, h)))


def eval_specular(incident, normal, diffuse, metallic, rough, w):
    h = unit(w + incident)
    d = gtr2(dot(normal, h), np.maximum(0.001, rough))[0]
    fs = 1.0 - col(metallic) + diffuse * col(metallic)                      # mix(1, diffuse, metallic)
    rg = (rough * 0.5 + 0.5) ** 2
    g = smith_g(dot(normal, w), rg) * smith_g(dot(normal, incident), rg)
    return col(g * d) * fs


def local_frame(n):
    up = np.where(col(np.abs(n[:, 2]) < 0.999), [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    t = unit(np.cross(up, n))
    return t, np.cross(n, t)


def sample_microfacet(n, rough, r1, r2):
    t, b = local_frame(n)
    a = np.maximum(0.001, rough)
    phi = r1 * 2.0 * np.pi
    cos_t = np.sqrt((1.0 - r2) / (1.0 + (a * a - 1.0) * r2))
    sin_t = np.clip(np.sqrt(1.0 - cos_t * cos_t), 0.0, 1.0)
    return t * col(sin_t * np.cos(phi)) + b * col(sin_t * np.sin(phi)) + n * col(cos_t)


def sample_lambert(n, r1, r2):
    t, b = local_frame(n)
    r, phi = np.sqrt(r1), 2.0 * np.pi * r2
    x, y = r * np.cos(phi), r * np.sin(phi)
    return t * col(x) + b * col(y) + n * col(np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y)))


def sample_env(arrays, env_theta, r0, r1, r2):
    """sampleEnv: a uniform bin, a uniform point of it -> (direction, pdf, sin phi)"""
    bins = np.asarray(arrays.bins, np.float64).reshape(-1, 4)
    nb = len(bins)
    b = bins[np.clip((nb * r0).astype(np.int64), 0, nb - 1)]
    dx, dy = (float(arrays.env_w), float(arrays.env_h)) if arrays.env is not None else (1.0, 2048.0)
    ux = -float(np.float32(env_theta)) + ((b[:, 2] - b[:, 0]) * r1 + b[:, 0]) / dx
    uy = ((b[:, 3] - b[:, 1]) * r2 + b[:, 1]) / dy
    theta, phi = ux * 2.0 * np.pi, uy * np.pi
    sp = np.sin(phi)
    d = np.stack([np.cos(theta) * sp, np.cos(phi), np.sin(theta) * sp], 1)
    with np.errstate(divide="ignore"):
        pdf = (dx * dy / nb) / ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) * 2.0 * np.pi * np.pi * sp)
    return d, pdf, sp


def vertex(arrays, rays, t, index, rnd, specular, inside, tir, env_theta):
    """The vertex at hits (t, index) of rays [n, 6] with the random numbers rnd [n, >= 8] (call order: two of
    sampleMicrofacet, three of sampleEnv, the specular coin, two of sampleLambert) and the decisions specular, inside and
    tir (refract() returned 0) -> dict of float64 arrays"""
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rays, t, rnd = f64(rays).reshape(-1, 6), f64(t).reshape(-1), f64(rnd)
    index = np.asarray(index).reshape(-1)
    specular, inside, tir = (np.asarray(x).reshape(-1) != 0 for x in (specular, inside, tir))
    s = LR.hit_surface(arrays, rays, t, index)
    mat = f64(arrays.mat).reshape(-1, 12)[index]
    ior, dielectric = mat[:, 9], mat[:, 10]
    diffuse, emissive = s["diffuse"], s["emissive"]
    metallic, rough = s["mr"][:, 0], s["mr"][:, 1] ** 2
    n = np.where(col(inside), -s["macro_normal"], s["macro_normal"])
    eta = np.where(inside, ior, 1.0 / ior)                                          # ns.x / ns.y
    off = n * EPSILON * 2.0
    incident = -rays[:, 3:]
    micro = sample_microfacet(n, rough, rnd[:, 0], rnd[:, 1])
    env_dir, env_pdf, sin_phi = sample_env(arrays, env_theta, rnd[:, 2], rnd[:, 3], rnd[:, 4])
    cos_env = dot(n, env_dir)
    refracted = ~specular & (dielectric >= 0.0)
    lambert = ~specular & ~refracted
    with np.errstate(all="ignore"):
        # reflect(-incident, micro) / refract(-incident, micro, eta) / sampleLambert
        i_ = -incident
        c = dot(micro, i_)
        rd_s = i_ - 2.0 * col(c) * micro
        kk = 1.0 - eta * eta * (1.0 - c * c)
        rd_r = np.where(col(tir), 0.0, col(eta) * i_ - col(eta * c + np.sqrt(np.maximum(kk, 0.0))) * micro)
        rd_l = sample_lambert(n, rnd[:, 6], rnd[:, 7])
        rd = np.where(col(specular), rd_s, np.where(col(refracted), rd_r, rd_l))
        ro = np.where(col(refracted), s["origin"] - off, s["origin"] + off)
        cl, ce = np.clip(dot(n, rd), 0.0, 1.0), np.clip(cos_env, 0.0, 1.0)
        pdf_s = gtr2_pdf(incident, n, rough, rd_s)
        pdf_l = np.abs(dot(rd_l, n)) / np.pi
        bsdf_pdf = np.where(specular, pdf_s, np.where(refracted, 1.0, pdf_l))
        f_rd = np.where(col(specular), eval_specular(incident, n, diffuse, metallic, rough, rd_s), diffuse / np.pi)
        f_env = np.where(col(specular), eval_specular(incident, n, diffuse, metallic, rough, env_dir), diffuse / np.pi)
        thr_b = np.where(col(refracted), 1.0, f_rd * col(cl) / col(bsdf_pdf))
        thr_e = np.where(col(refracted), 0.0, f_env * col(ce) / col(env_pdf))
        absorb = 1.0 - (1.0 - diffuse) * col(t) * col(dielectric)                   # "some bad approximation of beers law"
        thr_b = np.where(col(inside), np.maximum(absorb, 0.0), thr_b)
        wx, wy = mis_weights(env_pdf, bsdf_pdf)
        h_s = unit(rd_s + incident)
    return dict(origin=s["origin"], normal=n, micro_normal=micro, rd=rd, ro=ro, bsdf_pdf=bsdf_pdf, env_pdf=env_pdf, env_dir=env_dir,
                cos_env=cos_env, bsdf_throughput=thr_b, env_throughput=thr_e, weights=np.stack([wx, wy], 1),
                emission=30.0 * emissive * diffuse, diffuse=diffuse, metallic=metallic, rough=rough, incident=incident,
                dielectric=dielectric, refracted=refracted, lambert=lambert, has_shadow=(dielectric < 0.0) & (cos_env > 0.0),
                # what the exemptions look at
                gtr2_t=gtr2(np.abs(dot(h_s, n)), np.maximum(0.001, rough))[1], rd_dot_h=np.abs(dot(rd_s, h_s)), sin_phi=sin_phi,
                absorb=absorb, cl=dot(n, rd), kk=kk)


# ---- the emitter arm --------------------------------------------------------------------------------------
def tri_edges(arrays, tri):
    v = np.asarray(arrays.tri, np.float32).astype(np.float64).reshape(-1, 3, 3)[tri]
    return v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]


def emitter_vertex(arrays, v, table, q, entry, u, thr=1.0):
    """The emitter strategy of vertices v (vertex()'s dict) at emitter fraction q with the sample's table entry and its
    random numbers u [n, 4]: the point (b0 = 1 - sqrt(u2), b1 = u3 sqrt(u2)), Le = 30 E D there, pdf_L = p_e dist^2 /
    (A |n_g . w|) (0 edge-on), the lobe's f and pdf_B, w_L, sc = cos w_L / (q pdf_L), pend = thr f Le sc, lq = q / pb."""
    u = np.asarray(u, np.float32).astype(np.float64)
    entry = np.asarray(entry).astype(np.int64)
    tri = np.asarray(table["tris"]).astype(np.int64)[entry]
    p_e = np.asarray(table["light_p"], np.float32).astype(np.float64)[entry]
    v1, e1, e2 = tri_edges(arrays, tri)
    su = np.sqrt(u[:, 2])
    b1 = u[:, 3] * su
    b2, b0 = su - b1, 1.0 - su
    x = v1 + e1 * col(b1) + e2 * col(b2)
    uvs = np.asarray(arrays.uv, np.float32).astype(np.float64).reshape(-1, 3, 2)[tri]
    uv = uvs[:, 0] * col(b0) + uvs[:, 1] * col(b1) + uvs[:, 2] * col(b2)
    m = LR.material_lookup(arrays, tri, uv[:, 0], uv[:, 1])
    le = 30.0 * m["emissive"] * m["diffuse"]
    d = x - v["ro"]
    d2 = dot(d, d)
    dist = np.sqrt(d2)
    w = d / col(dist)
    gl = np.abs(dot(np.cross(e1, e2), w))                                           # 2 A |cos_l|
    n, inc = v["normal"], v["incident"]
    with np.errstate(all="ignore"):
        pdf_l = np.where(gl > 0.0, p_e * d2 * 2.0 / gl, 0.0)
        cn = dot(n, w)
        spec = ~v["lambert"]
        f = np.where(col(spec), eval_specular(inc, n, v["diffuse"], v["metallic"], v["rough"], w), v["diffuse"] / np.pi)
        pdf_b = np.where(spec, gtr2_pdf(inc, n, v["rough"], w), np.abs(cn) / np.pi)
        qp = q * pdf_l
        w_l = qp * qp / (qp * qp + pdf_b * pdf_b)
        sc = cn * w_l / qp
        pend = thr * f * le * col(sc)
        h = unit(w + inc)
    return dict(x=x, w=w, dist=dist, le=le, pdf_L=pdf_l, pdf_B=pdf_b, w_L=w_l, cn=cn, sc=sc, pend=pend, lt=dist * LIGHT_T_SCALE,
                gl=gl, has_shadow=(cn > 0.0) & (pdf_l > 0.0) & np.isfinite(sc),
                gtr2_t=gtr2(np.abs(dot(h, n)), np.maximum(0.001, v["rough"]))[1], w_dot_h=np.abs(dot(w, h)))


def environment_strategy(v, q, thr=1.0):
    """the environment strategy of a q > 0 vertex: the reference's NEE over 1 - q, its MIS weight folded in -> (sc, pend)"""
    sc = v["weights"][:, 0] / (1.0 - q)
    return sc, thr * v["env_throughput"] * col(sc)


def lq(v, q):
    with np.errstate(all="ignore"):
        return np.where(v["bsdf_pdf"] > 0.0, q / v["bsdf_pdf"], 0.0)


def emission_weight(arrays, pick, lq_, rd, t, index):
    """emw: pb^2 / (pb^2 + (q pick t^2 / (A |n_g . rd|))^2) with lq = q / pb; 1 for lq = 0 or pick = 0, 0 edge-on"""
    lq_, t = (np.asarray(a, np.float32).astype(np.float64) for a in (lq_, t))
    rd = np.asarray(rd, np.float32).astype(np.float64).reshape(-1, 3)
    index = np.asarray(index).astype(np.int64)
    pk = np.asarray(pick, np.float32).astype(np.float64)[index]
    _, e1, e2 = tri_edges(arrays, index)
    den = 0.5 * np.abs(dot(np.cross(e1, e2), rd))
    with np.errstate(all="ignore"):
        x = np.where(den > 0.0, lq_ * pk * t * t / den, np.inf)
        return np.where((lq_ > 0.0) & (pk > 0.0), 1.0 / (1.0 + x * x), 1.0)


# ---- a one-bounce sample and the running mean ------------------------------------------------------------------------
def env_radiance(arrays, dirs, env_theta):
    return LR.env_lookup(arrays.env.reshape(arrays.env_h, arrays.env_w, 4), arrays.env_w, arrays.env_h, dirs, env_theta)


def colour_one_bounce(arrays, v, shadow_missed, extension_missed, env_theta):
    """the sample of a path of one vertex (tracer.fs:467, 500-505, 509-511, 515): emission, the environment through the
    shadow ray where it was cast and missed, the environment through the extension ray where that missed; clamped"""
    with np.errstate(all="ignore"):
        nee = v["env_throughput"] * env_radiance(arrays, v["env_dir"], env_theta) * col(v["weights"][:, 0])
        ext = v["bsdf_throughput"] * env_radiance(arrays, v["rd"], env_theta) * col(v["weights"][:, 1])
    c = v["emission"] + np.where(col(v["has_shadow"] & shadow_missed), nee, 0.0) + np.where(col(extension_missed), ext, 0.0)
    return np.clip(c, 0.0, 1024.0)


def running_mean(prev, colour, tick):
    """tracer.fs:515-517: (clamp(colour, 0, 1024) + prev tick) / (tick + 1), exactly"""
    prev, colour = np.asarray(prev, np.float64), np.asarray(colour, np.float64)
    return (prev * float(tick) + np.clip(colour, 0.0, 1024.0)) / (float(tick) + 1.0)
