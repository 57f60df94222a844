"""Temporal accumulation (fspt_temporal_accumulate) restated in float64: what the GPU result is held to.

Operation order (the kernel's, include/fspt_tuning.h has the rule):

  centre ray   (float32, like k_temporal_gbuffer and camera_ray: the only float32 part here)
      fx = x + 0.5, fy = y + 0.5;  uvx = fma(fx / W, 2, -1), uvy = fma(fy / H, 2, -1)
      bX = normalize(cross(I, (0, 1, 0))), bY = normalize(cross(bX, I))       cross / dot / normalize as fspt_math.hpp
      icx = uvx * (W / H), icy = uvy
      screen_c = (fma(icy * bY_c, fov, (icx * bX_c) * fov) + I_c) + P_c
      o = P, d = normalize(screen - P)
  previous position
      X' = P + t d                                   (static scene)
      X' = v1' + bv e1' + bw e2'                     (motion origin: the snapshot's triangle in the same leaf slot)
      v  = X' - P_prev  (hit)   |   d  (miss)
  projection   (bX, bY of the PREVIOUS camera, from its I as above)
      a = (v . I) / (I . I);  a <= 0: kind 0
      icx = (v . bX) / (a fov), icy = (v . bY) / (a fov)
      sx = (icx (H / W) + 1) (W / 2) - 0.5,  sy = (icy + 1) (H / 2) - 0.5
      r = floor(s + 0.5);  |s - r| <= 1/128: s = r   (the snap)
      M = (sx, sy, |v| (hit) or 0 (miss), kind 1 (hit) / 2 (miss))
  blend        taps k = 0..3: q = (floor(sx) + (k & 1), floor(sy) + (k >> 1)), w = (ax or 1 - ax)(ay or 1 - ay), ax = sx - floor(sx)
      a tap counts when w > 0, q is inside, hit(q) == hit(p), and for hits |t_prev(q) - M.z| <= depth_tol M.z and
      n(p) . n_prev(q) >= normal_cos
      H = sum w hist(q).rgb / sum w;  N = min(sum w hist(q).w / sum w, max_history);  a_new = max(n / (N + n), alpha)
      out = (H + (I - H) a_new, min(N + n, max_history));   nothing counts: out = (I.rgb, min(n, max_history))
"""
import numpy as np

F = np.float32
SNAP = 1.0 / 128.0
MAX_T = 100000.0
DEFAULTS = {"alpha": 0.0, "max_history": 64.0, "depth_tol": 0.05, "normal_cos": 0.95}


# ---- float32 pieces (the kernel's inputs) ----------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; one rounding to float64 and one to float32 (the double
    rounding differs from a true fma about once in 2^29 operands)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def dot32(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F)))


def cross32(a, b):
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1]).astype(F)),
                     fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2]).astype(F)),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]).astype(F))], -1)


def normalize32(a):
    inv = (F(1.0) / np.sqrt(dot32(a, a))).astype(F)
    return (a * inv[..., None]).astype(F)


def basis32(I):
    I = np.asarray(I, F)
    bX = normalize32(cross32(I, np.array([0, 1, 0], F)))
    bY = normalize32(cross32(bX, I))
    return bX, bY


def centre_rays(W, H, P, I, fov):
    """(o float32 [3], d float32 [H, W, 3]): the pinhole ray through every pixel centre, rows bottom-up"""
    P, I, fov = np.asarray(P, F), np.asarray(I, F), F(fov)
    bX, bY = basis32(I)
    fx = (np.arange(W, dtype=F) + F(0.5))[None, :].repeat(H, 0)
    fy = (np.arange(H, dtype=F) + F(0.5))[:, None].repeat(W, 1)
    resx, resy = F(W), F(H)
    uvx = fma32((fx / resx).astype(F), F(2.0), F(-1.0))
    uvy = fma32((fy / resy).astype(F), F(2.0), F(-1.0))
    icx = (uvx * (resx / resy)).astype(F)
    icy = uvy
    scr = np.zeros((H, W, 3), F)
    for c in range(3):
        scr[..., c] = (fma32((icy * bY[c]).astype(F), fov, ((icx * bX[c]).astype(F) * fov).astype(F)) + I[c]).astype(F) + P[c]
    d = normalize32((scr - P).astype(F))
    return P, d


def rays6(o, d):
    """[H * W, 6] float32 rays for fspt_intersect / the oracle"""
    H, W = d.shape[:2]
    return np.concatenate([np.broadcast_to(o, (H, W, 3)), d], -1).reshape(-1, 6).astype(F)


# ---- float64 from here on ---------------------------------------------------------------------------------------------
EPSILON = float(F(1e-6))  # tracer.fs:8


def closest_hit(arrays, rays, chunk=None):
    """Section 2's trace, restated: the closest hit of float32 rays [n, 6] over EVERY triangle of the scene, no tree, float64
    Moller-Trumbore with rayTriangleIntersect's rule (tracer.fs:300-315: |det| >= EPSILON, 0 <= u, 0 <= v, u + v <= 1,
    dist > EPSILON) and intersectScene's dist < MAX_T; the first triangle in array order wins a tie.
    Returns (t float64 [n] (MAX_T: miss), index int64 [n] (-1: miss), bv, bw float64 [n])."""
    tri = np.asarray(arrays.tri, F).reshape(-1, 3, 3).astype(np.float64)
    rays = np.asarray(rays, F).reshape(-1, 6).astype(np.float64)
    v1, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n, T = rays.shape[0], tri.shape[0]
    chunk = chunk or max(1, (1 << 20) // max(T, 1))
    t_out, i_out = np.full(n, MAX_T), np.full(n, -1, np.int64)
    bv_out, bw_out = np.zeros(n), np.zeros(n)
    for s in range(0, n, chunk):
        o, d = rays[s:s + chunk, None, :3], rays[s:s + chunk, None, 3:]
        p = np.cross(d, e2[None])
        det = (e1[None] * p).sum(-1)
        tv = o - v1[None]
        q = np.cross(tv, e1[None])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            u, v, dist = (tv * p).sum(-1) * inv, (d * q).sum(-1) * inv, (e2[None] * q).sum(-1) * inv
            ok = (np.abs(det) >= EPSILON) & (u >= 0) & (v >= 0) & (u + v <= 1) & (dist > EPSILON) & (dist < MAX_T)
        dist = np.where(ok, dist, np.inf)
        j = dist.argmin(1)
        r = np.arange(len(j))
        h = np.isfinite(dist[r, j])
        t_out[s:s + chunk] = np.where(h, dist[r, j], MAX_T)
        i_out[s:s + chunk] = np.where(h, j, -1)
        bv_out[s:s + chunk] = np.where(h, u[r, j], 0.0)
        bw_out[s:s + chunk] = np.where(h, v[r, j], 0.0)
    return t_out, i_out, bv_out, bw_out


def gbuffer_exempt(arrays, W, H, P, I, fov, oracle_index):
    """The G-buffer test's exempt pixels, decided WITHOUT the GPU: where this restatement's own triangle on the float32 centre
    rays differs from the oracle's (oracle_index [H, W], -1 = miss).  Returns (exempt bool [H, W], t64, index, bv, bw as [H, W])."""
    o, d = centre_rays(W, H, P, I, fov)
    t, idx, bv, bw = (a.reshape(H, W) for a in closest_hit(arrays, rays6(o, d)))
    return idx != np.asarray(oracle_index).reshape(H, W), t, idx, bv, bw


def basis64(I):
    I = np.asarray(I, F).astype(np.float64)
    bX = np.cross(I, [0.0, 1.0, 0.0]); bX /= np.linalg.norm(bX)
    bY = np.cross(bX, I); bY /= np.linalg.norm(bY)
    return I, bX, bY


def snapshot_from_triangles(tri, slot_tri):
    """The motion origin a scene whose leaf-order triangles are `tri` takes: per leaf slot v1, e1, e2 (the hit record's float32
    edges), float64 [n_slots, 9]; empty slots zero."""
    t = np.asarray(tri, F).reshape(-1, 3, 3)
    rec = np.concatenate([t[:, 0], (t[:, 1] - t[:, 0]).astype(F), (t[:, 2] - t[:, 0]).astype(F)], 1).astype(np.float64)
    st = np.asarray(slot_tri).astype(np.int64)
    out = np.zeros((st.size, 9))
    ok = st < rec.shape[0]
    out[ok] = rec[st[ok]]
    return out


def permute_snapshot(snap_by_tri, order):
    """What a rebuild does to a per-TRIANGLE snapshot [T, 9]: new leaf position k holds old triangle order[k]"""
    return np.asarray(snap_by_tri)[np.asarray(order).astype(np.int64)]


def motion(G, d, cam, prev, snapshot=None):
    """M from a G-buffer (float32 [H, W, 8], the GPU's own or previous_position's), the centre-ray directions d, this
    frame's camera and the previous one ((P, I, fov) each), the per-slot snapshot or None.
    Returns dict: sx, sy (snapped), sx_raw, sy_raw, dist, kind, scale (the magnitude the float32 error bound scales with)."""
    H, W = G.shape[:2]
    P = np.asarray(cam[0], F).astype(np.float64)
    P2 = np.asarray(prev[0], F).astype(np.float64)
    I2, bX, bY = basis64(prev[1])
    fov2 = float(F(prev[2]))
    hit = G[..., 7] != 0
    t = G[..., 0].astype(np.float64)
    d64 = d.astype(np.float64)
    X = P + t[..., None] * d64
    if snapshot is not None:
        slot = np.ascontiguousarray(G[..., 1]).view(np.int32)
        s = snapshot[np.where(hit, slot, 0)]
        bv, bw = G[..., 2].astype(np.float64)[..., None], G[..., 3].astype(np.float64)[..., None]
        X = s[..., 0:3] + bv * s[..., 3:6] + bw * s[..., 6:9]
    v = np.where(hit[..., None], X - P2, d64)
    a = (v @ I2) / (I2 @ I2)
    front = a > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        icx = (v @ bX) / (a * fov2)
        icy = (v @ bY) / (a * fov2)
    sx = (icx * (H / W) + 1.0) * (W / 2.0) - 0.5
    sy = (icy + 1.0) * (H / 2.0) - 0.5

    def snap(s):
        r = np.floor(s + 0.5)
        return np.where(np.abs(s - r) <= SNAP, r, s)
    dist = np.where(hit, np.linalg.norm(v, axis=-1), 0.0)
    kind = np.where(front, np.where(hit, 1.0, 2.0), 0.0)
    # float32 error: every term of v carries ~eps (|X'| + |P_prev|); the projection divides by a |I| fov
    mag = np.where(hit, np.linalg.norm(X, axis=-1) + np.linalg.norm(P2), 1.0) + np.linalg.norm(v, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = mag / (np.abs(a) * np.linalg.norm(I2) * fov2)
    return {"sx": snap(sx), "sy": snap(sy), "sx_raw": sx, "sy_raw": sy, "dist": dist, "kind": kind, "a": a, "scale": scale}


def blend(I, M, G, hist, g_prev, n, alpha=0.0, max_history=64.0, depth_tol=0.05, normal_cos=0.95):
    """The blend pass on float32 arrays in the library's layouts, evaluated in float64.  hist None: no history.
    Returns (out float64 [H, W, 4], margin float64 [H, W]): margin = how far the pixel's nearest validity test (of a tap with
    w > 0 inside the image that agrees in hit / miss) lies from its threshold, relative to the threshold's scale - a pixel
    with a small margin may legitimately flip in float32."""
    I = np.asarray(I, np.float64); M = np.asarray(M, np.float64); G = np.asarray(G, np.float64)
    H, W = I.shape[:2]
    n = float(n)
    out = np.concatenate([I[..., :3], np.full((H, W, 1), min(n, max_history))], -1)
    margin = np.full((H, W), np.inf)
    if hist is None:
        return out, margin
    hist = np.asarray(hist, np.float64); gp = np.asarray(g_prev, np.float64)
    sx, sy, mz, kind = M[..., 0], M[..., 1], M[..., 2], M[..., 3]
    with np.errstate(invalid="ignore"):
        cand = (kind != 0) & (sx > -1.0) & (sy > -1.0) & (sx < W) & (sy < H)
    sxc, syc = np.where(cand, sx, 0.0), np.where(cand, sy, 0.0)
    flx, fly = np.floor(sxc), np.floor(syc)
    ax, ay = sxc - flx, syc - fly
    hp = G[..., 7]
    npx = G[..., 4:7]
    acc = np.zeros((H, W, 4)); sw = np.zeros((H, W))
    for k in range(4):
        i, j = k & 1, k >> 1
        xx, yy = (flx + i).astype(np.int64), (fly + j).astype(np.int64)
        w = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
        ok = cand & (xx >= 0) & (yy >= 0) & (xx < W) & (yy < H) & (w > 0)
        xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
        q0, q1 = gp[yc, xc, 0:4], gp[yc, xc, 4:8]
        ok &= q1[..., 3] == hp
        ishit = hp != 0
        dz = np.abs(q0[..., 0] - mz) - depth_tol * mz
        cs = (npx * q1[..., 0:3]).sum(-1) - normal_cos
        tested = ok & ishit
        with np.errstate(divide="ignore", invalid="ignore"):
            mk = np.minimum(np.abs(dz) / np.maximum(np.abs(mz), 1e-30), np.abs(cs))
        margin = np.where(tested, np.minimum(margin, mk), margin)
        ok &= ~ishit | ((dz <= 0) & (cs >= 0))
        h = hist[yc, xc]
        acc += np.where(ok[..., None], w[..., None] * h, 0.0)
        sw += np.where(ok, w, 0.0)
    valid = sw > 0
    swc = np.where(valid, sw, 1.0)
    Hc = acc[..., :3] / swc[..., None]
    N = np.minimum(acc[..., 3] / swc, max_history)
    a_new = np.maximum(n / (N + n), alpha)
    res = np.concatenate([Hc + (I[..., :3] - Hc) * a_new[..., None], np.minimum(N + n, max_history)[..., None]], -1)
    return np.where(valid[..., None], res, out), margin


def running_mean_f32(hist, I, n, alpha=0.0, max_history=64.0):
    """The blend of a pixel whose single tap of weight 1 is itself, by the kernel's float32 operations: sr = fma(1, h, 0) = h,
    sw = 1, H = h / 1, N = min(h.w / 1, max_history), a = max(n / (N + n), alpha), out = H + (I - H) * a (multiply, then add)."""
    hist, I = np.asarray(hist, F), np.asarray(I, F)
    n, alpha, mh = F(n), F(alpha), F(max_history)
    N = np.minimum(hist[..., 3], mh)
    a = np.maximum((n / (N + n)).astype(F), alpha)[..., None]
    Hc = hist[..., :3]
    rgb = (Hc + ((I[..., :3] - Hc).astype(F) * a).astype(F)).astype(F)
    return np.concatenate([rgb, np.minimum((N + n).astype(F), mh)[..., None]], -1).astype(F)
