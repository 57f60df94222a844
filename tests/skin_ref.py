"""The rule of DESIGN 8.16 (GPU skinning: linear-blend skinning with morph targets) in numpy, bit for bit.

Per triangle corner (3 T of them; leaf order): four joint ids and four weights (used as given), a rest vertex r and,
with a rest norm, three rest frame vectors n, t, bt.  A frame is one row-major 3 x 4 matrix J per joint and one weight per
morph target.  float32, an fma exactly where one is written (fma32 of tests/exposure_ref.py: exact), every other
product, quotient and square root rounded on its own:
    morph    r_c = fma(w_m, morph_m_c, r_c) for m = 0 .. n_morph - 1 in order; the frame vectors alike with morph_norm
    blend    B_e = w_0 J0_e, then B_e = fma(w_k, Jk_e, B_e) for k = 1, 2, 3                      (the 12 entries e)
    vertex   p'_c = fma(B_c2, z, fma(B_c1, y, fma(B_c0, x, B_c3)))
    frame    q = B00 B00, then q = fma(B_ij, B_ij, q) over the other eight entries of the 3 x 3, row-major
             g2 = q / 3, ig = 1 / sqrt(g2), ig2 = 1 / g2
             C_ij = fma(B_i1j1, B_i2j2, -(B_i1j2 B_i2j1)), i1 = (i + 1) % 3, i2 = (i + 2) % 3, j alike
             t, bt    d'_c = fma(B_c2, z, fma(B_c1, y, B_c0 x)) ig
             n        n'_c = fma(C_c2, z, fma(C_c1, y, C_c0 x)) ig2
Nothing is normalised; q == 0 gives inf / NaN.

The error bound (`skin64`).  u = 2^-24, gamma(k) = k u / (1 - k u): a value that went through k roundings, each of
relative size <= u, is off by at most gamma(k) times the sum of the MAGNITUDES of its terms (Higham, Accuracy and Stability,
3.1-3.4; cancellation is why the magnitudes, not the value).  Write X~ for that magnitude sum, evaluated in float64:
    r~ = |rest| + sum |w_m| |morph_m|        a term of r carries <= M roundings (M = n_morph; one per fma it passes)
    B~_e = sum_k |w_k| |Jk_e|                a term of B_e carries <= 4 (one product, three fmas)
    vertex: a term B_ci r_i carries <= 4 + M from its factors and <= 3 from the chain's fmas:
        |p'_c - exact| <= gamma(7 + M) P~_c,     P~_c = B~_c3 + sum_i B~_ci r~_i
    q: a term B_e^2 carries 2 x 4 from its factors and <= 9 from the chain: |q - exact| <= gamma(17) Q~, Q~ = sum B~_e^2,
        so q is off by the RELATIVE rho_q = gamma(17) Q~ / q  (large when the blend cancels: the rule is ill-conditioned there
        and the bound says so).  g2 adds one rounding, ig a square root (which halves a relative error) and two roundings,
        ig2 one:  rho_ig = rho_q / 2 + 3 u,   rho_ig2 = rho_q + 2 u,  each taken as x / (1 - x) to cover the second order.
    t, bt: a term B_ci f_i carries <= 4 + M + 3 (product, two fmas), the product by ig one more and ig's own error:
        |d'_c - exact| <= ig D~_c (gamma(8 + M) + rho_ig),       D~_c = sum_i B~_ci f~_i
    n: a cofactor's term carries 4 + 4 + 2 = 10, so a term C_ci f_i carries <= 10 + M + 3, then ig2:
        |n'_c - exact| <= ig2 N~_c (gamma(14 + M) + rho_ig2),    N~_c = sum_i C~_ci f~_i,  C~_ij = B~_i1j1 B~_i2j2 + B~_i1j2 B~_i2j1
"exact" is evaluated in float64, whose own roundings (2^-53 each, the same counts) are covered by one more unit in every
gamma.  The model has no underflow term: the bound holds for values whose products stay normal in float32."""
import numpy as np

from exposure_ref import fma32

F = np.float32
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def _inputs(dt, joints, weights, tri, norm, xf, morph, morph_norm, morph_w):
    joints = np.asarray(joints).astype(np.int64).reshape(-1, 4)
    nc = joints.shape[0]
    w = np.asarray(weights, F).astype(dt).reshape(nc, 4)
    J = np.asarray(xf, F).astype(dt).reshape(-1, 12)
    r = np.asarray(tri, F).astype(dt).reshape(nc, 3).copy()
    f = None if norm is None else np.asarray(norm, F).astype(dt).reshape(nc, 9).copy()
    M = MN = mw = None
    if morph is not None and np.size(morph):
        M = np.asarray(morph, F).astype(dt).reshape(-1, nc, 3)
        mw = np.asarray(morph_w, F).astype(dt).reshape(-1)
        assert mw.size == M.shape[0]
        if morph_norm is not None:
            assert f is not None
            MN = np.asarray(morph_norm, F).astype(dt).reshape(-1, nc, 9)
    return joints, nc, w, J, r, f, M, MN, mw


def skin(joints, weights, tri, norm, xf, morph=None, morph_norm=None, morph_w=None):
    """joints [T, 3, 4] ids, weights [T, 3, 4], rest tri [T, 9] / norm [T, 27] (or None), xf [n_joints, 12], morph
    [n_morph, T, 9] / morph_norm [n_morph, T, 27] (or None), morph_w [n_morph] -> (tri' [T, 9], norm' [T, 27] or None),
    float32, what k_skin_transform writes"""
    joints, nc, w, J, r, f, M, MN, mw = _inputs(F, joints, weights, tri, norm, xf, morph, morph_norm, morph_w)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for m in range(0 if M is None else M.shape[0]):
            r = fma32(mw[m], M[m], r)
            if MN is not None:
                f = fma32(mw[m], MN[m], f)
        B = (w[:, 0:1] * J[joints[:, 0]]).astype(F)
        for k in (1, 2, 3):
            B = fma32(w[:, k:k + 1], J[joints[:, k]], B)
        B = B.reshape(nc, 3, 4)
        x, y, z = r[:, 0:1], r[:, 1:2], r[:, 2:3]
        p = fma32(B[:, :, 2], z, fma32(B[:, :, 1], y, fma32(B[:, :, 0], x, B[:, :, 3])))
        if f is None:
            return p.reshape(-1, 9), None
        A = B[:, :, :3]
        q = (A[:, 0, 0] * A[:, 0, 0]).astype(F)
        for e in range(1, 9):
            b = A[:, e // 3, e % 3]
            q = fma32(b, b, q)
        g2 = (q / F(3.0)).astype(F)
        ig = (F(1.0) / np.sqrt(g2).astype(F)).astype(F)
        ig2 = (F(1.0) / g2).astype(F)
        Cf = np.zeros((nc, 3, 3), F)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                Cf[:, i, j] = fma32(A[:, i1, j1], A[:, i2, j2], -(A[:, i1, j2] * A[:, i2, j1]).astype(F))
        out = np.zeros((nc, 9), F)
        for v in range(3):
            fx, fy, fz = f[:, 3 * v:3 * v + 1], f[:, 3 * v + 1:3 * v + 2], f[:, 3 * v + 2:3 * v + 3]
            rows, scale = (Cf, ig2) if v == 0 else (A, ig)
            acc = fma32(rows[:, :, 2], fz, fma32(rows[:, :, 1], fy, (rows[:, :, 0] * fx).astype(F)))
            out[:, 3 * v:3 * v + 3] = (acc * scale[:, None]).astype(F)
        return p.reshape(-1, 9), out.reshape(-1, 27)


def skin64(joints, weights, tri, norm, xf, morph=None, morph_norm=None, morph_w=None):
    """The same rule evaluated in float64 (an fma is a product and a sum there), and the bound of the docstring on
    |skin(...) - it| per output: (tri' [T, 9], norm' [T, 27] or None, bound_tri [T, 9], bound_norm [T, 27] or None)"""
    D = np.float64
    joints, nc, w, J, r, f, M, MN, mw = _inputs(D, joints, weights, tri, norm, xf, morph, morph_norm, morph_w)
    nm = 0 if M is None else M.shape[0]
    ra = np.abs(r)
    fa = None if f is None else np.abs(f)
    for m in range(nm):
        r = mw[m] * M[m] + r
        ra = np.abs(mw[m]) * np.abs(M[m]) + ra
        if MN is not None:
            f = mw[m] * MN[m] + f
            fa = np.abs(mw[m]) * np.abs(MN[m]) + fa
    B = np.zeros((nc, 12), D)
    Ba = np.zeros((nc, 12), D)
    for k in range(4):
        B = w[:, k:k + 1] * J[joints[:, k]] + B
        Ba = np.abs(w[:, k:k + 1]) * np.abs(J[joints[:, k]]) + Ba
    B, Ba = B.reshape(nc, 3, 4), Ba.reshape(nc, 3, 4)
    p = B[:, :, 3] + (B[:, :, :3] * r[:, None, :]).sum(-1)
    pa = Ba[:, :, 3] + (Ba[:, :, :3] * ra[:, None, :]).sum(-1)
    bp = gamma(7 + nm + 1) * pa
    if f is None:
        return p.reshape(-1, 9), None, bp.reshape(-1, 9), None
    A, Aa = B[:, :, :3], Ba[:, :, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (A * A).sum((1, 2))
        rho_q = gamma(17 + 1) * (Aa * Aa).sum((1, 2)) / q
        x = rho_q / 2 + 3 * U
        rho_ig = x / (1 - x)
        x = rho_q + 2 * U
        rho_ig2 = x / (1 - x)
        g2 = q / 3.0
        ig, ig2 = 1.0 / np.sqrt(g2), 1.0 / g2
        Cf, Ca = np.zeros((nc, 3, 3), D), np.zeros((nc, 3, 3), D)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                Cf[:, i, j] = A[:, i1, j1] * A[:, i2, j2] - A[:, i1, j2] * A[:, i2, j1]
                Ca[:, i, j] = Aa[:, i1, j1] * Aa[:, i2, j2] + Aa[:, i1, j2] * Aa[:, i2, j1]
        out, bound = np.zeros((nc, 9), D), np.zeros((nc, 9), D)
        for v in range(3):
            fv, fva = f[:, None, 3 * v:3 * v + 3], fa[:, None, 3 * v:3 * v + 3]
            if v == 0:
                out[:, 0:3] = (Cf * fv).sum(-1) * ig2[:, None]
                bound[:, 0:3] = ig2[:, None] * (Ca * fva).sum(-1) * (gamma(14 + nm + 1) + rho_ig2)[:, None]
            else:
                out[:, 3 * v:3 * v + 3] = (A * fv).sum(-1) * ig[:, None]
                bound[:, 3 * v:3 * v + 3] = ig[:, None] * (Aa * fva).sum(-1) * (gamma(8 + nm + 1) + rho_ig)[:, None]
    return p.reshape(-1, 9), out.reshape(-1, 27), bp.reshape(-1, 9), bound.reshape(-1, 27)


def pose_bound(tri, norm, xf):
    """What tests/pose_ref.py's pose() of ONE matrix may differ from the exact value by, per output, by the same count:
    the vertex chain is three fmas on exact inputs (gamma(3)); D = float32(A / g) and N = float32(C / g^2) come from
    float64 with one rounding to float32, then the product and two fmas: gamma(4) on the magnitudes.  (tri, norm) bounds."""
    D = np.float64
    m = np.asarray(xf, F).astype(D).reshape(3, 4)
    A = m[:, :3]
    r = np.abs(np.asarray(tri, F).astype(D).reshape(-1, 3))
    f = np.abs(np.asarray(norm, F).astype(D).reshape(-1, 3, 3))
    g2 = (A * A).sum() / 3.0
    Ca = np.zeros((3, 3), D)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            Ca[i, j] = abs(A[i1, j1] * A[i2, j2]) + abs(A[i1, j2] * A[i2, j1])
    bt = gamma(3 + 1) * (np.abs(m[:, 3]) + (np.abs(A) * r[:, None, :]).sum(-1))
    bn = np.zeros(f.shape, D)
    bn[:, 0] = gamma(4 + 1) * (Ca * f[:, None, 0, :]).sum(-1) / g2
    for v in (1, 2):
        bn[:, v] = gamma(4 + 1) * (np.abs(A) * f[:, None, v, :]).sum(-1) / np.sqrt(g2)
    return bt.reshape(-1, 9), bn.reshape(-1, 27)
