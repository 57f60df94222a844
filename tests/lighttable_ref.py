"""The GPU builder's emitter light table (fspt_scene_set_light_builder) restated in Python integers and numpy
float64: `build` follows the closed form the kernels follow, `light_p_of` computes light_p of any (prob, alias) from its
definition alone.  Every sum is an integer sum, so the order they are taken in here is of no consequence."""
import bisect
from itertools import accumulate

import numpy as np

TWO32 = float(2 ** 32)
TWO40 = 2 ** 40
MAX_ENTRIES = 2 ** 23


def quantise(w):
    """q_e = max(1, rint((double)w_e / (double)w_max * 2^32)), round to nearest even; 0 for a weight of 0 (the raw hook)."""
    w = np.asarray(w, np.float32)
    assert w.ndim == 1 and w.size and np.isfinite(w).all() and (w >= 0).all() and (w > 0).any()
    x = np.rint(w.astype(np.float64) / np.float64(w.max()) * TWO32)
    return [0 if wi == 0 else max(1, int(xi)) for wi, xi in zip(w, x)]


def build(w):
    """The table of weights w (float32, finite, >= 0, some > 0): dict of prob float32, alias uint32, light_p float32 and
    the integers behind them (q, T, r per entry, the lists)."""
    q = quantise(w)
    n = len(q)
    assert n <= MAX_ENTRIES
    T = sum(q)
    m = [n * qe for qe in q]
    assert sum(m) == n * T
    lights = [e for e in range(n) if m[e] < T]
    heavies = [e for e in range(n) if m[e] >= T]
    a, b = len(lights), len(heavies)
    D = list(accumulate(T - m[e] for e in lights))   # D[j - 1] = D_j
    X = list(accumulate(m[e] - T for e in heavies))  # X[k - 1] = X_k
    assert (D[-1] if a else 0) == X[-1]
    Dprev = [0] + D[:-1] if a else []                # Dprev[j - 1] = D_{j-1}
    r = [0] * n
    alias = np.arange(n, dtype=np.uint32)
    for j, e in enumerate(lights):
        k = bisect.bisect_right(X, Dprev[j])         # min{k : X_k > D_{j-1}}
        assert k < b
        r[e] = m[e]
        alias[e] = heavies[k]
    jstar = [bisect.bisect_left(Dprev, X[k]) for k in range(b)]  # #{j : D_{j-1} < X_k}
    for k, e in enumerate(heavies):
        r[e] = T + X[k] - (D[jstar[k] - 1] if jstar[k] else 0)
        assert 0 < r[e] <= T, (k, r[e], T)
        if r[e] < T:
            alias[e] = heavies[k + 1]
    assert r[heavies[-1]] == T
    # (float)((double)r / (double)T): int -> float64 rounds to nearest even, like the device's conversion
    prob = (np.array([float(x) for x in r], np.float64) / np.float64(float(T))).astype(np.float32)
    give = (TWO40 - np.floor(prob.astype(np.float64) * float(TWO40)).astype(np.int64)).tolist()  # = moved(prob[e])
    # S of heavy k: the lights j*(k - 1) < j <= j*(k) and heavy k - 1 when it was cut below T
    C = [0] + list(accumulate(give[e] for e in lights))   # C[j] = C_j
    S = [0] * n
    for k, e in enumerate(heavies):
        S[e] = C[jstar[k]] - (C[jstar[k - 1]] if k else 0)
        if k and r[heavies[k - 1]] < T:
            S[e] += give[heavies[k - 1]]
    light_p = ((prob.astype(np.float64) + np.array([float(x) for x in S], np.float64) * 2.0 ** -40) / np.float64(n)).astype(np.float32)
    return {"prob": prob, "alias": alias, "light_p": light_p, "q": q, "T": T, "r": r, "S": S, "lights": lights, "heavies": heavies}


def light_p_of(prob, alias):
    """light_p[e] = (float)(((double)prob_e + (double)S_e 2^-40) / n), S_e = sum over j != e with alias_j = e of
    (2^40 - floor((double)prob_j 2^40)) in uint64: from the definition, by scatter-add."""
    prob = np.asarray(prob, np.float32)
    alias = np.asarray(alias, np.int64)
    n = prob.size
    give = (np.uint64(TWO40) - np.floor(prob.astype(np.float64) * float(TWO40)).astype(np.uint64)).astype(np.uint64)
    S = np.zeros(n, np.uint64)
    other = alias != np.arange(n)
    np.add.at(S, alias[other], give[other])
    return ((prob.astype(np.float64) + S.astype(np.float64) * 2.0 ** -40) / np.float64(n)).astype(np.float32)


def scene_table(t):
    """The restatement of a scene's table t (Scene.light_table()) from its weights: prob, alias, pick"""
    w = t["weights"]
    tris = np.nonzero(w > 0)[0].astype(np.uint32)
    if tris.size == 0:
        return {"tris": tris, "prob": np.zeros(0, np.float32), "alias": np.zeros(0, np.uint32), "pick": np.zeros(t["slot_tri"].size, np.float32)}
    b = build(w[tris])
    tri_p = np.zeros(w.size, np.float32)
    tri_p[tris] = b["light_p"]
    st = t["slot_tri"]
    pick = np.where(st < w.size, tri_p[np.minimum(st, w.size - 1)], np.float32(0)).astype(np.float32)
    return {"tris": tris, "prob": b["prob"], "alias": b["alias"], "pick": pick}


# ---- the weight vectors of tests/test_lighttable_*.py: the smallest at which each piece can go wrong -------------------
def one_heavy(n):
    w = np.full(n, 0.001, np.float32)
    w[n // 3] = 50.0
    return w


def vectors():
    rng = np.random.default_rng(23)
    v = {
        "n1": np.float32([3.5]),
        "n2": np.float32([1.0, 3.0]),
        "zero_excess": np.float32([1, 1, 2, 4]),                 # entry 2 has m == T: a heavy of excess 0
        "equal257": np.full(257, 0.25, np.float32),              # no lights, every prob = 1
        "heavy255": one_heavy(255), "heavy256": one_heavy(256), "heavy257": one_heavy(257),  # a 256-wide scan's block edges
        "heavy65537": one_heavy(65537),                          # ... and its second level's
        "loguniform4099": (10.0 ** rng.uniform(-3.0, 3.0, 4099)).astype(np.float32),  # chains of heavies finalised at once
        "clamp": np.float32([1.0, 2.0 ** -40, 3e-12, 0.5, 2.0 ** -34, 2.0 ** -33, 1e-3]),  # more than 2^33 apart: q = 1
        "zeros": np.float32([0.0, 1.0, 0.0, 3.0, 0.0, 0.0, 2.0, 0.0]),                    # the hook's q = 0
    }
    # half bright, half 1000 times fainter at n = 2^18 + 3: the deficits sum to ~2^66, past 64 bits (why D and X are 128-bit)
    wide = np.where(np.arange(262147) % 2 == 0, 1.0, 1e-3) * rng.uniform(0.5, 1.0, 262147)
    v["wide262147"] = wide.astype(np.float32)
    return v
