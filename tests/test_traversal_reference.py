"""intersectScene (tracer.fs:366-404) of the CPU oracle against an independent float64 closest hit (tests/hitref.py) on
labelled families of edge-case rays (tests/rays.py), and the structural invariants of the native SAH builder's trees.

The HIP traversals are compared bit for bit with the oracle (tests/test_traversal_gpu.py), so an error the oracle and
the kernels share - a box that does not contain its triangles, a culled box, a skipped leaf triangle - shows up here."""
import numpy as np
import pytest

import hitref as HR
import oracle as O
import rays as R

FUZZ_SEEDS = range(8)

# Decisive fraction floors per family (tests/hitref.py).  Bunny scenes: small (0.02 - 0.05) triangles of a closed
# mesh.  Fuzz scenes: triangles of size ~1 with slivers, huge and duplicate triangles, where more rays meet a
# triangle within the float32 error; on_surface there is not decidable at all (the origin's own triangle is met at
# t = 0 +- tau_t > EPSILON) and has no floor.
FLOORS = {
    "bunny": dict(axis=0.8, plane=0.8, vertex_edge=0.6, grazing=0.4, on_surface=0.6, far=0.4, tiny=0.9, inside=0.9, scaled=0.9),
    "fuzz": dict(axis=0.9, plane=0.8, vertex_edge=0.45, grazing=0.6, on_surface=0.0, far=0.1, tiny=0.9, inside=0.9, scaled=0.9),
}


@pytest.fixture(scope="module")
def scenes(small_scene, medium_scene):
    out = {"small": small_scene, "medium": medium_scene}
    for s in FUZZ_SEEDS:
        out[f"fuzz{s}"] = R.fuzz_scene(s)[0]
    return out


def _check_families(arrays, name, n):
    kind = "fuzz" if name.startswith("fuzz") else "bunny"
    report, failures = [], []
    for rays, fam in R.all_families(arrays, 1, n):
        c = HR.classify(arrays, rays)
        t, idx, steps, leaves = O.intersect(arrays, rays)
        bad = c.mismatches(t, idx)
        report.append(f"{fam} {c.fraction():.2f} (hit {(c.kind == 1).mean():.2f} miss {(c.kind == 0).mean():.2f})")
        failures += [f"{fam}: " + c.describe(i, t, idx) + f" ray {rays[i].tolist()}" for i in bad[:5]]
        if c.fraction() < FLOORS[kind][fam]:
            failures.append(f"{fam}: decisive fraction {c.fraction():.3f} < {FLOORS[kind][fam]}")
        assert (steps >= 1).all() and (leaves <= steps).all()
    print(f"\n{name}: decisive fractions: " + ", ".join(report))
    return failures


@pytest.mark.parametrize("name", ["small", "medium"] + [f"fuzz{s}" for s in FUZZ_SEEDS])
def test_oracle_traversal_vs_float64(scenes, name):
    """Every decisive ray of every family: the oracle's hit index is the float64 closest triangle (one of a tie band)
    and its t is within tau_t; a decisive miss is index -1, t == MAX_T."""
    arrays = scenes[name]
    failures = _check_families(arrays, name, 512 if name == "medium" else 1024)
    assert not failures, "\n".join(failures)


def _leaves(arrays):
    """Pre-order walk of the tree from the root: (leaf node, first triangle, depth) in visiting order, and the
    (parent, child) pairs."""
    w = arrays.bvh.reshape(-1, 9)[:, :3].view(np.int32)
    leaves, edges, stack = [], [], [(0, 0)]
    seen = np.zeros(arrays.n_nodes, bool)
    while stack:
        node, depth = stack.pop()
        assert 0 <= node < arrays.n_nodes and not seen[node], f"node {node} reached twice or out of range"
        seen[node] = True
        if w[node, 2] > -1:
            leaves.append((node, int(w[node, 2]), depth))
        else:
            l, r = int(w[node, 0]), int(w[node, 1])
            edges += [(node, l), (node, r)]
            stack += [(r, depth + 1), (l, depth + 1)]
    assert seen.all(), "nodes not reachable from the root"
    return leaves, edges


BUILDER_SCENES = [f"bunny6-leaf{k}" for k in range(1, 6)] + [f"fuzz{s}" for s in FUZZ_SEEDS]


def _builder_scene(name):
    from fspt_amd import scene as S
    if name.startswith("fuzz"):
        return R.fuzz_scene(int(name[4:]))[0]
    texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(6), "synthetic/quad.obj": S.QUAD_OBJ}
    return S.build_scene(S.bunny_props(), texts, leaf_size=int(name[-1]))


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_bvh_structural_invariants(name, small_scene, medium_scene):
    """The native SAH builder's trees (leaf sizes 1 - 5, degenerate / sliver / duplicate triangles): leaf triangle
    ranges partition [0, n_tris) in pre-order; every leaf box holds its own triangles' float32 vertices exactly (no
    tolerance: traversal culls with these boxes); every parent box holds both children's; the depth is at most the
    declared `depth` (tracer.fs:368's 64-entry stack depends on it).  (The bunny scenes of the other tests too.)"""
    arrays = _builder_scene(name)
    for nm, a in [(name, arrays), ("small", small_scene), ("medium", medium_scene)]:
        b = a.bvh.reshape(-1, 9)
        bmin, bmax = b[:, 3:6], b[:, 6:9]
        tri = a.tri.reshape(-1, 3, 3)
        leaves, edges = _leaves(a)
        first = np.array([f for _, f, _ in leaves])
        count = np.diff(np.append(first, a.n_tris))
        assert first[0] == 0 and (count >= 1).all() and (count <= a.leaf_size).all(), nm
        assert count.sum() == a.n_tris, nm
        for (node, f, _), c in zip(leaves, count):
            v = tri[f:f + c].reshape(-1, 3)
            assert (bmin[node] <= v).all() and (v <= bmax[node]).all(), f"{nm}: leaf {node} does not hold its triangles"
        for p, ch in edges:
            assert (bmin[p] <= bmin[ch]).all() and (bmax[ch] <= bmax[p]).all(), f"{nm}: node {p} does not hold child {ch}"
        assert max(d for _, _, d in leaves) <= a.depth, nm
        assert np.isfinite(b[:, 3:]).all() and (bmin <= bmax).all(), nm
