"""CPU checks of the GPU light-table builder's definition (fspt_scene_set_light_builder) through its
restatement tests/lighttable_ref.py: the table's invariants, what it realises against the quantised and the raw weights in
exact fractions, its light_p against the oracle's and against the device's alias draw; and of the new entry points, the
Python host and the render CLI without a device."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import lights_ref as R
import lighttable_ref as T
import oracle as O
from fspt_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = T.vectors()
# the comparison with the oracle's float64 light_p alone has a size cap (its docstring); every other property runs on every vector
ORACLE = [k for k, w in VECTORS.items() if w.size <= 4099]


@pytest.fixture(scope="module")
def tables():
    return {k: T.build(w) for k, w in VECTORS.items()}


@pytest.mark.parametrize("name", list(VECTORS))
def test_invariants(tables, name):
    b = tables[name]
    prob, alias, r, Tq = b["prob"], b["alias"].astype(np.int64), b["r"], b["T"]
    n = prob.size
    assert prob.dtype == np.float32 and b["alias"].dtype == np.uint32 and b["light_p"].dtype == np.float32
    assert (alias >= 0).all() and (alias < n).all()
    assert (prob >= 0).all() and (prob <= 1).all()
    own = alias == np.arange(n)
    assert np.array_equal(own, np.array([x == Tq for x in r]))  # alias_e == e iff r == T
    assert (prob[own] == 1.0).all()
    light = np.zeros(n, bool); light[b["lights"]] = True
    assert not light[alias].any()                               # no entry aliases to a light
    assert not own[light].any()
    # The table's mass in units of 2^-40, from the definition: entry e realises P_e + S_e with P_e = floor(prob_e 2^40) and
    # S_e = sum over j != e with alias_j = e of (2^40 - P_j).  Summed over e every j with alias_j != j contributes P_j +
    # (2^40 - P_j) = 2^40, and every j with alias_j == j contributes P_j = 2^40 (its prob is 1): n 2^40 exactly.
    P = np.floor(prob.astype(np.float64) * 2.0 ** 40).astype(np.int64).tolist()
    S = [0] * n
    for j in range(n):
        if alias[j] != j:
            S[alias[j]] += 2 ** 40 - P[j]
    assert S == b["S"]
    assert sum(P) + sum(S) == n * 2 ** 40
    assert sum(P[j] for j in range(n) if own[j]) + 2 ** 40 * int((~own).sum()) == n * 2 ** 40
    lp = T.light_p_of(prob, b["alias"])
    assert np.array_equal(lp.view(np.uint32), b["light_p"].view(np.uint32))
    assert np.array_equal(lp[~np.isin(np.arange(n), alias[~own])], (prob.astype(np.float64) / n).astype(np.float32)[~np.isin(np.arange(n), alias[~own])])


# Exact rational arithmetic.  Every float32 is an integer multiple of 2^-149, so a Fraction of one has the denominator 2^149
# at the most: the two bound tests work on the numerators over that common denominator and compare a / b <= c / d as
# a d <= c b, in Python integers - the inequalities of fractions.Fraction, term for term, without its gcd at every step (the
# 262 147-entry vector takes a second instead of nine).  The vectors up to 4099 entries are also put through Fraction itself.
U = 149


def units(a):
    """float32 array -> its values as integers in units of 2^-149 (exact)"""
    out = []
    for x in np.asarray(a, np.float32).tolist():
        num, den = float(x).as_integer_ratio()
        assert (1 << U) % den == 0
        out.append(num * ((1 << U) // den))
    return out


def realised_units(P, alias):
    """What the stored float32 table realises per entry, exactly, times n, in units of 2^-149: a slot is drawn with
    probability 1 / n, its entry kept with probability prob (1 for an entry that is its own alias)."""
    real = [0] * len(P)
    for j, p in enumerate(P):
        if alias[j] == j:
            real[j] += 1 << U
        else:
            real[j] += p
            real[alias[j]] += (1 << U) - p
    return real


@pytest.mark.parametrize("name", list(VECTORS))
def test_realises_the_quantised_weights(tables, name):
    """|prob_e - r_e / T| <= 2^-25 (one float32 rounding of a value in [0, 1]) and
    |realised_e - q_e / T| <= (1 + #aliased to e) 2^-25 / n, exactly."""
    b = tables[name]
    prob, alias, Tq, n, r, q = b["prob"], b["alias"].astype(np.int64).tolist(), b["T"], b["prob"].size, b["r"], b["q"]
    P = units(prob)
    tol = Tq << (U - 25)  # 2^-25, over the denominator 2^149 T
    for e in range(n):
        assert abs(P[e] * Tq - (r[e] << U)) <= tol, (e, r[e])
    real = realised_units(P, alias)
    assert sum(real) == n << U
    into = np.bincount(np.array([alias[j] for j in range(n) if alias[j] != j], np.int64), minlength=n).tolist()
    for e in range(n):  # realised_e = real[e] / (n 2^149)
        assert abs(real[e] * Tq - ((q[e] * n) << U)) <= (1 + into[e]) * tol, e
    if n <= 4099:
        for e in range(n):
            assert abs(Fraction(float(prob[e])) - Fraction(r[e], Tq)) <= Fraction(1, 2 ** 25), (e, r[e])
            assert abs(Fraction(real[e], n << U) - Fraction(q[e], Tq)) <= (1 + into[e]) * Fraction(1, 2 ** 25) / n, e


@pytest.mark.parametrize("name", list(VECTORS))
def test_quantised_weights_against_the_raw_weights(tables, name):
    """q_e / T against p_e = w_e / sum w.  With s_e = w_e / w_max 2^32 (exact) and q_e = s_e + d_e:
      - the device rounds x' = fl(fl(w_e / w_max) 2^32), |x' - s_e| <= s_e 2^-53 <= 2^-21 (one float64 division; the
        scaling is exact), so |d_e| <= 1/2 + 2^-21 where rint decides;
      - where s_e < 1/2 + 2^-21 the clamp may decide: q_e = 1, 0 < d_e <= 1;
      - d_e = 0 for a weight of 0 (q_e = 0).
    Let B_e be that bound on |d_e|, Sg = sum s = 2^32 sum w / w_max and Dl = sum d, |Dl| <= sum B.  Then
      q_e / T - p_e = (s_e + d_e) / (Sg + Dl) - s_e / Sg = (d_e - p_e Dl) / (Sg + Dl),
    so |q_e / T - p_e| <= (B_e + p_e sum B) / (Sg - sum B).
    In integers: W = the weights in units of 2^-149, b_e = 2^21 B_e, sb = sum b; then Sg - sum B = (2^53 tot - sb Wmax) /
    (2^21 Wmax), and the bound cross-multiplied is |q_e tot - W_e T| (2^53 tot - sb Wmax) <= (b_e tot + W_e sb) Wmax T."""
    b = tables[name]
    q, Tq = b["q"], b["T"]
    W = units(VECTORS[name])
    wmax, tot = max(W), sum(W)
    half = (1 << 20) + 1                       # 2^21 (1/2 + 2^-21)
    bb = [0 if x == 0 else ((1 << 21) if (x << 53) < half * wmax else half) for x in W]  # s_e < 1/2 + 2^-21: the clamp's 1
    sb = sum(bb)
    room = (tot << 53) - sb * wmax
    assert room > 0
    for e in range(len(W)):
        assert abs(q[e] * tot - W[e] * Tq) * room <= (bb[e] * tot + W[e] * sb) * wmax * Tq, e
    if len(W) <= 4099:
        w = [Fraction(float(x)) for x in VECTORS[name]]
        fmax, ftot = max(w), sum(w)
        s_ = [x / fmax * 2 ** 32 for x in w]
        rnd = Fraction(1, 2) + Fraction(1, 2 ** 21)
        B = [Fraction(0) if x == 0 else (Fraction(1) if x < rnd else rnd) for x in s_]
        Sg, sB = sum(s_), sum(B)
        assert Sg > sB
        for e in range(len(w)):
            assert abs(Fraction(q[e], Tq) - w[e] / ftot) <= (B[e] + w[e] / ftot * sB) / (Sg - sB), e


@pytest.mark.parametrize("name", ORACLE)
def test_light_p_agrees_with_the_oracle(tables, name):
    """oracle.realised_p sums 1 - prob_j in float64; light_p truncates each to 2^-40: below #aliased 2^-40 / n in all, against
    a float32 ulp of at least 2^-24 / n for an entry somebody aliases to (its probability is at least 1 / n).  One ulp is
    promised for n <= 4096; the argument holds while fewer than 2^16 entries alias to one, so the 4099-entry vector is held
    to it too, and the vectors from 65 537 entries on (65 536 aliased to one entry) are not."""
    b = tables[name]
    want = O.realised_p(b["prob"], b["alias"])
    got = b["light_p"]
    assert (np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1).all()


# The device's draw is float32: slot floor(v n) and the coin its fraction, from one 24-bit v, so the coin has 24 - log2(n) bits.
# At 262 147 entries that is 6: an entry kept with prob = 0.002 is kept whenever the coin is 0, once in 64.  What such a
# table realises under that draw is a property of the sampler of DESIGN 8.3 under either builder, not of the table, and a
# chi-square of the draw against light_p measures the coin there; the vector is left to the exact tests above.
DRAWN = [k for k in VECTORS if k != "wide262147"]


@pytest.mark.parametrize("name", DRAWN)
def test_the_draw_realises_light_p(tables, name):
    """Entries drawn as the device draws them (lights_ref.alias_v / pick_entry) over a fine, jittered grid of u1 against
    light_p: chi-square against its degrees of freedom, as test_rnd_draws_realise_light_p.  At least 128 grid points per
    entry, so that an entry of probability 1 / (2 n) still expects more than 50 draws; taken 2^22 at a time."""
    b = tables[name]
    n = b["prob"].size
    alias = b["alias"].astype(np.int64)
    rng = np.random.default_rng(7)
    CH = 1 << 22
    chunks = max(1, -(-128 * n // CH))
    N = chunks * CH
    cnt = np.zeros(n)
    for c in range(chunks):
        u1 = ((np.arange(c * CH, (c + 1) * CH) + rng.uniform(0.0, 1.0, CH)) / N).astype(np.float32)
        u1 = np.minimum(u1, np.float32(1.0 - 2.0 ** -24))
        u0 = rng.uniform(0.0, 0.5, CH).astype(np.float32)
        cnt += np.bincount(R.pick_entry(b["prob"], alias, R.alias_v(u0, u1, 0.5)), minlength=n)
    exp = b["light_p"].astype(np.float64) * N
    big = exp > 50
    assert big.any()
    chi2, dof = float(((cnt[big] - exp[big]) ** 2 / exp[big]).sum()), max(int(big.sum()) - 1, 1)
    print("%s: %d draws, chi2 %.1f over %d dof; faint entries %d for %.1f expected" % (name, N, chi2, dof, cnt[~big].sum(), exp[~big].sum()))
    assert chi2 < dof + 6.0 * np.sqrt(2.0 * dof)
    assert cnt[~big].sum() <= 2.0 * exp[~big].sum() + 10
    assert (cnt[b["light_p"] == 0] == 0).all()


def test_restatement_refuses_bad_weights():
    for bad in ([0.0, 0.0], [1.0, -1.0], [1.0, np.nan], [np.inf, 1.0], []):
        with pytest.raises(AssertionError):
            T.quantise(np.float32(bad))


# ---- the ABI, the Python host and the CLI without a device -----------------------------------------------------------------
NEW = ("fspt_scene_set_light_builder", "fspt_scene_get_light_builder", "fspt_light_alias_table_gpu", "fspt_scene_light_build_stats")


def test_entry_points_exist_and_validate():
    raw = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n) and n in L.SIGNATURES
    lib = L.lib()
    assert lib.fspt_abi_version() == 4
    b = C.c_int(-1)
    assert lib.fspt_scene_set_light_builder(None, 1) == -1
    assert lib.fspt_scene_get_light_builder(None, C.byref(b)) == -1
    assert lib.fspt_scene_light_build_stats(None, None, None, None) == -1
    assert lib.fspt_light_alias_table_gpu(0, None, 3, None, None, None) == -1
    w = np.ones(3, np.float32)
    assert lib.fspt_light_alias_table_gpu(0, L.fptr(w), 0, None, None, None) == -1
    assert lib.fspt_light_alias_table_gpu(0, L.fptr(w), (1 << 23) + 1, None, None, None) == -1 and b"at most" in lib.fspt_last_error()
    fake = C.cast(C.create_string_buffer(8192), C.c_void_p)  # bad arguments are refused before the handle is looked at
    for bad in (2, -1, 7):
        assert lib.fspt_scene_set_light_builder(fake, bad) == -1, bad
        assert b"FSPT_LIGHT_BUILDER_GPU" in lib.fspt_last_error()
    assert lib.fspt_scene_get_light_builder(fake, None) == -1
    assert lib.fspt_scene_get_light_builder(fake, C.byref(b)) == 0 and b.value == 0  # (zeroed: the default, HOST)
    d, h = C.c_uint64(5), C.c_uint64(5)
    assert lib.fspt_scene_light_build_stats(fake, C.byref(d), C.byref(h), None) == 0 and d.value == 0 and h.value == 0


def test_no_device():
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    fake = C.cast(C.create_string_buffer(8192), C.c_void_p)  # (zeroed: device 0, no table yet)
    n = C.c_uint32()
    want = lib.fspt_scene_light_count(fake, C.byref(n))      # what the neighbouring entries return: no device
    assert want == -2
    assert lib.fspt_scene_set_light_builder(fake, 1) == want and b"no CPU fallback" in lib.fspt_last_error()
    assert lib.fspt_scene_set_light_builder(fake, 0) == want
    ms = C.c_float()
    assert lib.fspt_scene_light_build_stats(fake, None, None, C.byref(ms)) == want
    w = np.ones(3, np.float32)
    assert lib.fspt_light_alias_table_gpu(0, L.fptr(w), 3, None, None, None) == want


def test_python_argument_checks():
    from fspt_amd import scene_file as F
    from fspt_amd.tracer import LIGHT_BUILDERS, Scene
    assert LIGHT_BUILDERS == {"host": 0, "gpu": 1}
    sc = Scene.__new__(Scene)  # (the check runs before the library is called)
    sc._h = C.c_void_p()
    for bad in ("device", 1, None):
        with pytest.raises(ValueError):
            sc.set_light_builder(bad)
    with pytest.raises(ValueError, match="one of"):
        F.render_frame(None, None, 8, 8, lights="emitters", light_builder="device")
    with pytest.raises(ValueError, match='needs lights="emitters"'):
        F.render_frame(None, None, 8, 8, light_builder="gpu")
    with pytest.raises(ValueError, match='needs lights="emitters"'):
        F.render_sequence("x_{frame}.json", range(1), "o_{frame}.png", 8, 8, bvh="refit", light_builder="gpu")
    from fspt_amd import light_alias_table_gpu
    with pytest.raises(ValueError):
        light_alias_table_gpu([])


def test_cli_flag():
    r = subprocess.run([sys.executable, "-m", "fspt_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--light-builder" in r.stdout
    for args, msg in ((["--light-builder", "gpu"], "--light-builder needs --lights"), (["--lights", "--light-builder", "device"], "invalid choice")):
        r = subprocess.run([sys.executable, "-m", "fspt_amd.render"] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)
