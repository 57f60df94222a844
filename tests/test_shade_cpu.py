"""The shading vertex of the ORACLE on the committed zoo (tests/shade_cases.py): which branches the cases reach, read from
the oracle's own probes (bounce_probe, light_vertex_probe, emission_weight_probe), and the oracle's arithmetic against the
float64 statement of one vertex (tests/shade_ref.py).  The tolerances of shade_cases.MEASURED are measured here.  What is
held to the oracle bit for bit on the GPU (tests/test_shade_gpu.py) is so shown to go where a kernel can go wrong, and the
arithmetic the oracle and the kernels share to be the shader's.  No GPU."""
import numpy as np
import pytest

import oracle as O
import shade_cases as SC
import shade_ref as SR

MIN_CASES = 16
MAX_EXEMPT = 0.02


@pytest.fixture(scope="module")
def zoo():
    return SC.vertices("zoo")


@pytest.fixture(scope="module")
def dim():
    return SC.vertices("dim")


@pytest.fixture(scope="module")
def lit():
    return {f: SC.light_vertices(f) for f in SC.EMITTER_FRACTIONS}


def edge_on_emission_weights(V):
    """emission_weight_probe for a direction in the plane of every emitter triangle (den = 0: no ray can hit a triangle
    from inside its plane, so no vertex of a path gets there; the probe does)"""
    table, _ = SC.host_light_table()
    tris = table["tris"].astype(np.int64)
    _, e1, e2 = SR.tri_edges(V.arrays, tris)
    rd = (e1 / np.linalg.norm(e1, axis=1, keepdims=True)).astype(np.float32)
    return O.emission_weight_probe(V.arrays, (table, 0.5), np.ones(len(tris), np.float32), rd, np.ones(len(tris), np.float32), tris)


# ---- the census ----------------------------------------------------------------------------------------------------------
def pooled(lit, f):
    """f(L) of every emitter fraction's vertices, concatenated: the cases of the emitter arm"""
    return np.concatenate([f(L) for L in lit.values()])


def branches(V, D, lit):
    """name -> (bool over the cases that reach the branch, bool over the same cases: exempt from the float64 bound).  The
    cases are the first vertices of the zoo's rays (V), of the dim scene's (D), for the emitter arm the zoo's vertices at
    each emitter fraction (pooled), for emw the hits of their extension rays, and for den = 0 the probe's own."""
    thr = V.got["bsdf_throughput"]
    _, pick = SC.host_light_table()
    ex_v, ex_d, mid = V.any_exempt(), D.any_exempt(), lit[0.5]
    ex_lit = pooled(lit, lambda L: L.exempt())
    ex_ext = pooled(lit, lambda L: L.exempt()[L.ext])
    edge_on = edge_on_emission_weights(V) == 0
    return {
        "refract: kk < 0, rd = 0": (V.tir, ex_v),
        "absorption: max(., 0) clamps": (V.inside & (V.dielectric > 0) & (thr == 0).any(1), ex_v),
        "absorption: max(., 0) leaves it": (V.inside & (V.dielectric > 0) & (thr > 0).all(1), ex_v),
        "cl = 0: macroNormal faces away from rd": (~V.refracted & ~V.inside & (V.ref["cl"] <= 0) & (thr == 0).all(1), ex_v),
        "weights (1, 0): envPdf <= EPSILON": (D.got["env_pdf"] <= SC.EPSILON, ex_d),
        "emw: den = 0, x infinite": (edge_on, np.zeros(len(edge_on), bool)),        # (the probe's cases: nothing to condition)
        "emitter sample: sc not finite": (pooled(lit, lambda L: L.emitter & ~np.isfinite(L.v["sc"])), ex_lit),
        "emw: pk = 0": (pooled(lit, lambda L: (L.v["lq"][L.ext] > 0) & (pick[L.V.next_index[L.ext]] == 0)), ex_ext),
        "q > 0 on the specular lobe: metallic >= 1": ((mid.v["q"] > 0) & V.specular, mid.exempt()),
        "rough = 0 meets max(0.001, .)": (V.specular & (V.ref["rough"] == 0), ex_v),
        "opaque triangle hit from behind": (V.inside & (V.dielectric < 0), ex_v),
    }


def decisions(V, D, lit):
    """name -> (bool, bool, exempt): the two sides of each two-sided decision and the exempt cases among the same cases"""
    ex_v = V.any_exempt()
    out = {}
    for m in SC.MATERIALS:
        if m.metallic != 255:                   # 0 < P(specular) < 1: metallic + F (1 - metallic) with metallic below 1
            of = V.material == m.name
            out[f"specular coin, {m.name}"] = (of & V.specular, of & ~V.specular, ex_v)
    out["hasShadow"] = (V.has_shadow, ~V.has_shadow, ex_v)
    out["shadow ray misses / hits"] = (V.has_shadow & V.shadow_missed, V.has_shadow & ~V.shadow_missed, ex_v)
    out["extension ray misses / hits"] = (V.extension_missed, ~V.extension_missed, ex_v)
    out["strategy emitter / environment"] = (pooled(lit, lambda L: L.emitter), pooled(lit, lambda L: L.environment), pooled(lit, lambda L: L.exempt()))
    out["envPdf above / at most EPSILON"] = (D.got["env_pdf"] > SC.EPSILON, D.got["env_pdf"] <= SC.EPSILON, D.any_exempt())
    out["emw: pk > 0 / pk = 0"] = (pooled(lit, lambda L: (L.v["lq"][L.ext] > 0) & (L.emw < 1)), pooled(lit, lambda L: (L.v["lq"][L.ext] > 0) & (L.emw == 1)),
                                   pooled(lit, lambda L: L.exempt()[L.ext]))
    return out


def test_branch_census(zoo, dim, lit):
    """Every branch named in shade_cases is reached by at least 16 cases, every two-sided decision by 16 on each side
    (printed with -s).  A condition on the inputs: the zoo was enlarged until the oracle met it."""
    print()
    for name, (m, _) in branches(zoo, dim, lit).items():
        print(f"  {name:45s} {int(m.sum()):5d}")
        assert m.sum() >= MIN_CASES, name
    for name, (a, b, _) in decisions(zoo, dim, lit).items():
        print(f"  {name:45s} {int(a.sum()):5d} / {int(b.sum())}")
        assert a.sum() >= MIN_CASES and b.sum() >= MIN_CASES, name


def test_zoo_holds_what_it_claims(zoo):
    """both texture fetch paths, every kind of item hit, rays that miss, hits at t from 1e-3 to 1e3, the razor quads"""
    import lookup_cases as LC
    from appearance_cases import TEXSET_CONST, TEXSET_QUAD, TEXSET_SEPARATE
    kinds = LC.classify(zoo.arrays, 8 << 30)
    first = {it.material.name: it.first_quad for it in zoo.items if it.kind == "quad"}
    assert kinds[2 * first["tex_quad"]] == TEXSET_QUAD and kinds[2 * first["tex_sep"]] == TEXSET_SEPARATE
    assert kinds[2 * first["opaque_m0_r0"]] == TEXSET_CONST
    assert set(zoo.which) == set(range(len(zoo.items))) and (~zoo.hit).sum() >= MIN_CASES
    assert zoo.t.min() < 2e-3 and zoo.t.max() > 900
    assert zoo.tir.sum() == len(SC.TIR_RAZOR) and (zoo.material[zoo.tir] == "razor").all()
    # ... and what the zero direction finds is seen: the throughput behind it and the sample are not black
    assert (zoo.got["bsdf_throughput"][zoo.tir] > 0).all() and (zoo.colour[zoo.hit][zoo.tir] > 0).all()
    assert len(zoo.all_rays) < 6000


def test_exempt_share(zoo, dim, lit):
    """At most 2 % of all cases, and of the cases of every branch and of every side of every decision, are exempt from the
    float64 bound - each against the exempt cases among its own cases; every share is printed with -s.  The sides of a
    single material's specular coin are the stated exception: they keep 16 cases that are not exempt."""
    print()
    for V, name in ((zoo, "zoo"), (dim, "dim")):
        for k, m in V.exempt().items():
            print(f"  {name}: {k:26s} {int(m.sum()):4d} of {len(m)}")
    share = np.concatenate([zoo.any_exempt(), dim.any_exempt()] + [L.exempt() for L in lit.values()]).mean()
    print(f"  exempt: {100 * share:.2f} % of all cases")
    assert share <= MAX_EXEMPT
    masks = dict(branches(zoo, dim, lit))
    masks.update({f"{k} ({side})": (m, ab[2]) for k, ab in decisions(zoo, dim, lit).items() for side, m in zip("ab", ab[:2])})
    over = []
    for k, (m, ex) in masks.items():
        assert m.shape == ex.shape, k
        n = int((m & ex).sum())
        print(f"  {k:49s} {n:4d} of {int(m.sum()):5d} exempt: {100 * n / m.sum():.2f} %")
        if k.startswith("specular coin"):
            # The one exception: the grazing rays the cases must hold are specular by Fresnel and, on a lobe of width
            # 0.001, exempt by |dot(rd, h)| - a handful per material, against a coin side of a few dozen cases.  The side
            # keeps its 16 cases without them.
            assert (m & ~ex).sum() >= MIN_CASES, k
        elif n > MAX_EXEMPT * m.sum():
            over.append((k, n, int(m.sum())))
    assert not over, over


# ---- the float64 bound -----------------------------------------------------------------------------------------------
def accumulate_cases():
    """-> per tick of ACC_TICKS: (the oracle's accumulator after the tick, the float64 running mean, the pixels compared:
    all but those whose sample is NaN - what the clamp makes of NaN is the oracle's to say)"""
    rays, colour, kind = SC.acc_frame()
    pos, d = SC.acc_frame_arrays()
    keep = np.array([k != "nan" for k in kind])
    out = {}
    for tick in SC.ACC_TICKS:
        acc = SC.acc_preload()
        O.trace(SC.acc_scene(), 8, 8, pos, d, tick, SC.RAND_BASE, SC.ENV_THETA, 1, acc)
        out[tick] = (acc.reshape(-1, 4)[:, :3], SR.running_mean(SC.acc_preload().reshape(-1, 4)[:, :3], colour, tick), keep)
    return out


def comparisons(zoo, dim, lit):
    """-> [(field of MEASURED, the oracle's values, the float64 values)] over the non-exempt cases"""
    out = []
    for V in (zoo, dim):
        ok = ~V.any_exempt()
        for k, got in V.got.items():
            if k == "bsdf_pdf":          # a lobe of width a = 0.001 is a near-delta: its density is ill-conditioned by construction
                out.append(("bsdf_pdf", got[ok & ~V.sharp], V.ref[k][ok & ~V.sharp]))
                out.append(("bsdf_pdf_sharp", got[ok & V.sharp], V.ref[k][ok & V.sharp]))
            else:
                out.append((k, got[ok], V.ref[k][ok]))
        one = ok & (~V.refracted | V.extension_missed)       # a refracted ray that hits shades on: not one vertex
        out.append(("colour", V.colour[V.hit][one], V.ref_colour[one]))
        out.append(("colour", V.colour[~V.hit], V.miss_colour))
    for L in lit.values():
        ok, on = ~L.exempt(), L.strategy > 0
        sharp = L.V.sharp
        out.append(("lq", L.v["lq"][ok & ~sharp], L.ref_lq[ok & ~sharp]))
        out.append(("lq_sharp", L.v["lq"][ok & sharp], L.ref_lq[ok & sharp]))
        out.append(("sc", L.v["sc"][ok & on], L.ref_sc[ok & on]))
        out.append(("pend", L.v["pend"][ok & on], L.ref_pend[ok & on]))
        out.append(("emw", L.emw[ok[L.ext]], L.ref_emw[ok[L.ext]]))
    for got, ref, keep in accumulate_cases().values():
        out.append(("accumulate", got[keep], ref[keep]))
    return out


def measure(zoo, dim, lit):
    m = dict.fromkeys(SC.MEASURED, 0.0)
    for k, got, ref in comparisons(zoo, dim, lit):
        m[k] = max(m[k], SC.deviation(got, ref).max())
    return m


def test_measured_tolerances_are_current(zoo, dim, lit):
    """The figures of shade_cases.MEASURED are what the oracle deviates from the float64 vertex by (printed with -s)"""
    m = measure(zoo, dim, lit)
    print("\nMEASURED = {\n" + "".join(f'    "{k}": {float(f"{v:.3g}") + 10 ** (np.floor(np.log10(v)) - 2):.3g},\n' for k, v in m.items()) + "}")
    assert set(m) == set(SC.MEASURED)
    for k, v in m.items():
        assert np.isfinite(v), k
        assert v <= SC.MEASURED[k] <= 1.25 * v + 1e-12, (k, v, SC.MEASURED[k])


def test_oracle_matches_float64(zoo, dim, lit):
    for k, got, ref in comparisons(zoo, dim, lit):
        dev = SC.deviation(got, ref)
        assert dev.max() <= SC.BOUND[k], (k, int(dev.argmax()), dev.max())


def test_accumulate_exact_cases():
    """tick 0 leaves the clamped sample itself: +inf becomes 1024, a negative sample 0 (a NaN one: whatever the oracle's
    clamp makes of it - the kernels are held to that on the GPU, nothing is assumed here)"""
    _, colour, kind = SC.acc_frame()
    got = accumulate_cases()[0][0]
    kind = np.array(kind)
    with np.errstate(invalid="ignore"):
        want = np.clip(colour.astype(np.float64), 0, 1024)
    known = kind != "nan"
    assert np.array_equal(got[known], want[known].astype(np.float32))
    assert (got[kind == "inf"] == 1024).any() and (got[kind == "negative"] == 0).any() and (got[kind == "above"] == 1024).any()


def test_reference_rejects_mutants(zoo):
    """One-token defects of the vertex - in the TIR arm, the absorption, and the MIS weights - move a compared field beyond
    its bound on the zoo: the cases and the tolerances can tell them from the oracle."""
    ok = ~zoo.any_exempt()
    r = zoo.ref
    mutants = {
        "tir: rd = I instead of 0": ("rd", np.where(zoo.tir[:, None], -r["incident"], r["rd"])),
        "absorption: t dropped": ("bsdf_throughput", np.where(zoo.inside[:, None], np.maximum(1 - (1 - r["diffuse"]) * r["dielectric"][:, None], 0), r["bsdf_throughput"])),
        "absorption: no max(., 0)": ("bsdf_throughput", np.where(zoo.inside[:, None], r["absorb"], r["bsdf_throughput"])),
        "weights: balance instead of power": ("weights", np.stack(SR.mis_weights(np.sqrt(np.abs(r["env_pdf"])), np.sqrt(np.abs(r["bsdf_pdf"]))), 1)),
        "ro: offset along +normal when refracted": ("ro", r["origin"] + r["normal"] * 2e-6),
    }
    for name, (k, ref) in mutants.items():
        dev = SC.deviation(zoo.got[k][ok], ref[ok])
        assert dev.max() > SC.BOUND[k], name
