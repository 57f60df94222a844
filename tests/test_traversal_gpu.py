"""Every HIP traversal on the edge-case ray families of tests/rays.py: bit-equal to the oracle, and on the rays float64
decides (tests/hitref.py) equal to the float64 closest hit.  Zero direction components (1/d = +-inf, 0 * inf = NaN on
box planes), denormal components, far origins, origins on surfaces and inside boxes reach the packed-FP32 slab test,
the two-level box unions, k_wf_trace's LDS tree top, the tail kernel, k_wf_primary and the suspended traversals."""
import numpy as np
import pytest

import hitref as HR
import oracle as O
import rays as R
from fspt_amd import PathTracer, Scene

pytestmark = pytest.mark.gpu


def _scene(name, small_scene, medium_scene):
    if name == "small":
        return small_scene
    if name == "medium":
        return medium_scene
    return R.fuzz_scene(int(name[4:]))[0]


@pytest.mark.parametrize("name", ["small", "medium"] + [f"fuzz{s}" for s in range(8)])
def test_intersect_edge_rays_bitwise_and_float64(name, small_scene, medium_scene):
    """Scene.intersect on every family, both node forms: t bits, index, steps and leaves equal the oracle's; every
    decisive ray equals the float64 closest hit."""
    arrays = _scene(name, small_scene, medium_scene)
    sc = Scene(arrays)
    two_level = sc.two_level_nodes()[0]
    assert two_level or arrays.n_nodes == 1
    report = []
    for rays, fam in R.all_families(arrays, 2, 512):
        rt, ridx, rsteps, rleaves = O.intersect(arrays, rays)
        ref = HR.classify(arrays, rays)
        for tl in ((False, True) if two_level else (False,)):
            t, idx, steps, leaves = sc.intersect(rays, two_level=tl)
            assert np.array_equal(idx, ridx), (fam, tl, int((idx != ridx).sum()))
            assert np.array_equal(t.view(np.uint32), rt.view(np.uint32)), (fam, tl)
            assert np.array_equal(steps, rsteps) and np.array_equal(leaves, rleaves), (fam, tl)
            bad = ref.mismatches(t, idx)
            assert not bad, f"{fam} two_level={tl}: " + "; ".join(ref.describe(i, t, idx) for i in bad[:3])
        report.append(f"{fam} {ref.fraction():.2f}")
    print(f"\n{name}: decisive fractions: " + ", ".join(report))


def _frame(arrays, W, H, seed):
    """The unit-direction families packed into a W x H frame of ray buffers (pos.w = 1, dir.w = 0)."""
    fams = R.all_families(arrays, seed, -(-W * H // len(R.UNIT_FAMILIES)), R.UNIT_FAMILIES)
    rays = np.concatenate([r for r, _ in fams])[:W * H]
    pos = np.zeros((H, W, 4), np.float32); d = np.zeros((H, W, 4), np.float32)
    pos[..., :3] = rays[:, :3].reshape(H, W, 3); pos[..., 3] = 1.0
    d[..., :3] = rays[:, 3:].reshape(H, W, 3)
    return pos, d


CONFIGS = ([("wavefront", dict(tail=t, prim=p)) for t in (0, 1, -1) for p in (0, 1, 2)]
           + [("wavefront", dict(budget=b)) for b in (1, 3, 0)]
           + [("wavefront", dict(forms=f)) for f in ((1, 1, 1), (0, 0, 0), (0, 0, 2))]
           + [("megakernel", {}), ("stream", dict(pool=0)), ("stream", dict(pool=600))])


def test_production_kernels_on_edge_rays(small_scene, camera):
    """setRays + drawTracer (tracer.fs main for injected rays) with 1 and 4 bounces, through every pipeline and the
    traversal variants of the wavefront one (tail kernel round, primary launch form, suspension budget, node forms):
    the oracle's radiance bit for bit, finite; the reference's work counters on each pipeline's default
    configuration; and the bvh_test.fs step heat map."""
    W, H = 96, 64
    arrays = small_scene
    pos, d = _frame(arrays, W, H, 3)
    sc = Scene(arrays)
    for nb in (1, 4):
        want = np.zeros((H, W, 4), np.float32)
        oc = O.OCounters()
        O.trace(arrays, W, H, pos, d, 0, 123.0, camera["env_theta"], nb, want, counters=oc)
        assert np.isfinite(want).all()
        for pipeline, cfg in CONFIGS:
            pt = PathTracer(sc, W, H, num_bounces=nb)
            pt.envTheta = camera["env_theta"]
            pt.set_pipeline(pipeline, 0)
            if "tail" in cfg:
                pt.set_tail(cfg["tail"])
                pt.set_primary_form(cfg["prim"])
            if "budget" in cfg:
                pt.set_trace_budget(cfg["budget"])
            if "forms" in cfg:
                pt.set_node_form(*cfg["forms"])
            if cfg.get("pool"):
                pt.set_pool(cfg["pool"])
            pt.setRays(pos, d)
            pt.drawTracer(0, 123.0)
            got = pt.readRadiance()
            assert np.isfinite(got).all(), (nb, pipeline, cfg)
            assert np.array_equal(got, want), f"{nb} bounces, {pipeline} {cfg}: {(got != want).any(-1).sum()} pixels differ"
            pt.close()
        for pipeline in ("wavefront", "megakernel", "stream"):
            pt = PathTracer(sc, W, H, num_bounces=nb)
            pt.envTheta = camera["env_theta"]
            pt.set_pipeline(pipeline, 0)
            pt.enable_counters(True)
            pt.clear()
            pt.setRays(pos, d)
            pt.drawTracer(0, 123.0)
            assert np.array_equal(pt.readRadiance(), want), (nb, pipeline, "counting")
            assert pt.counters() == oc.as_dict(), (nb, pipeline)
            pt.close()
    want = np.zeros((H, W, 4), np.float32)
    O.trace_test(arrays, W, H, pos, d, 0, want)
    pt = PathTracer(sc, W, H)
    pt.setRays(pos, d)
    pt.drawTracerTest(0)
    assert np.array_equal(pt.readRadiance(), want) and want[..., 0].max() > 0
    pt.close()
