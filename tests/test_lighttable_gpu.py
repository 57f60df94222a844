"""The GPU builder of the emitter light table (fspt_scene_set_light_builder) on the MI355X: the raw-weights
hook and the scenes' tables byte for byte against the restatement tests/lighttable_ref.py, frames bit for bit against the
oracle fed the device's table, live updates against freshly created scenes, and the switch between the two builders."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lights_ref as R
import lighttable_ref as T
import oracle as O
import rebuild_ref as RB
import refit_ref as RF
from fspt_amd import FsptError, PathTracer, Scene, light_alias_table, light_alias_table_gpu
from fspt_amd import _lib as L
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu
CAM = S.BUNNY_CAMERA
W, H = 48, 32
VECTORS = T.vectors()
KEYS = ("weights", "prob", "alias", "tris", "pick", "slot_tri")


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def scenes():
    return {"e1": R.scene_e1(), "e2": R.scene_e2(), "e3": R.scene_e3()}


# ---- the raw hook ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VECTORS))
def test_raw_hook_equals_the_restatement(name):
    w = VECTORS[name]
    want = T.build(w)
    prob, alias, lp = light_alias_table_gpu(w)
    assert np.array_equal(alias, want["alias"]), int((alias != want["alias"]).sum())
    assert same(prob, want["prob"]), int((prob.view(np.uint32) != want["prob"].view(np.uint32)).sum())
    assert same(lp, want["light_p"]), int((lp.view(np.uint32) != want["light_p"].view(np.uint32)).sum())
    again = light_alias_table_gpu(w)
    assert same(again[0], prob) and np.array_equal(again[1], alias) and same(again[2], lp)


@pytest.mark.parametrize("bad", ([1.0, np.nan, 2.0], [np.inf, 1.0], [1.0, -1.0], [0.0, 0.0, 0.0], [1.0] * 300 + [-np.inf]))
def test_raw_hook_refuses_bad_weights(bad):
    w = np.float32(bad)
    out = np.zeros(w.size, np.float32); al = np.zeros(w.size, np.uint32)
    assert L.lib().fspt_light_alias_table_gpu(0, L.fptr(w), w.size, L.fptr(out), L.u32ptr(al), None) == -1
    assert b"bad weights" in L.lib().fspt_last_error()
    with pytest.raises(FsptError):
        light_alias_table_gpu(w)


# ---- scene tables ----------------------------------------------------------------------------------------------------
def gpu_scene(arrays):
    sc = Scene(arrays)
    assert sc.light_builder == "host"
    sc.set_light_builder("gpu")
    assert sc.light_builder == "gpu"
    return sc


def check_against_restatement(t):
    want = T.scene_table(t)
    assert np.array_equal(t["tris"], want["tris"])
    assert same(t["prob"], want["prob"]) and np.array_equal(t["alias"], want["alias"]) and same(t["pick"], want["pick"])


@pytest.mark.parametrize("name", ["e1", "e2", "e3"])
def test_scene_table(scenes, name):
    arrays = scenes[name]
    host = Scene(arrays)
    th = host.light_table()
    host.close()
    sc = gpu_scene(arrays)
    assert sc.light_build_stats() == (0, 0, 0.0)
    n = sc.light_count()
    d2h, h2d, ms = sc.light_build_stats()  # (before any host copy is asked for)
    assert 0 < d2h <= 16 and h2d == 0 and ms > 0
    t = sc.light_table()
    assert sc.light_build_stats()[:2] == (d2h, h2d)
    assert n == th["tris"].size == t["tris"].size and n > 0
    for key in ("weights", "tris", "slot_tri"):
        assert same(t[key], th[key]), key
    check_against_restatement(t)
    if name == "e3":
        assert (t["alias"] != np.arange(n)).any()
    sc.set_light_builder("gpu")  # drops the table: the next build writes the same buffers again
    t2 = sc.light_table()
    for key in KEYS:
        assert same(t[key], t2[key]), key
    q = np.zeros((64, 10), np.float32)
    q[:, 0:3] = [0.1, -0.3, 0.4]; q[:, 4] = 1.0; q[:, 6:10] = np.random.default_rng(2).random((64, 4), dtype=np.float32)
    tri, out = sc.light_sample_eval(q)
    otri, oout = O.light_sample(arrays, R.device_table(t), q)
    assert np.array_equal(tri, otri) and same(out, oout)
    sc.close()


# ---- frames against the oracle -----------------------------------------------------------------------------------------
def make_pt(sc, nb=4, pipeline="wavefront", lights=True, fraction=0.5, seed=7):
    pt = PathTracer(sc, W, H, num_bounces=nb)
    pt.set_camera(**CAM)
    pt.seed(seed)
    pt.set_pipeline(pipeline)
    if lights:
        pt.set_lights("emitters", fraction)
    return pt


@pytest.mark.parametrize("name,nb", [("e3", 2), ("e3", 4), ("e1", 4)])
def test_frames_match_the_oracle(scenes, name, nb):
    arrays = scenes[name]
    sc = gpu_scene(arrays)
    lights = (R.device_table(sc.light_table()), R.env_q(arrays, 0.5))
    want = None
    for pipeline in ("megakernel", "wavefront", "stream"):
        pt = make_pt(sc, nb=nb, pipeline=pipeline)
        if want is None:
            want = np.zeros((H, W, 4), np.float32)
            O.render(arrays, W, H, pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta, nb, 0, 2, 7, want, lights=lights)
        pt.render(2)
        got = pt.readRadiance()
        pt.close()
        assert np.array_equal(got, want), (pipeline, int((got != want).any(-1).sum()))
    assert want[..., :3].max() > 0
    sc.close()


# ---- live updates on E3 ------------------------------------------------------------------------------------------------
def live_frame(pt):
    pt.clear()
    pt.seed(7)
    pt.render(2)
    return pt.readRadiance()


def emitter_layer(arrays, tri):
    return int(np.clip(np.floor(arrays.mat.reshape(-1, 12)[tri, 1] + np.float32(0.5)), 0, arrays.atlas_layers - 1))


def e3_cases(e3):
    """name -> (what to do to the live scene, the arrays a fresh scene is created from)"""
    emit = np.nonzero(R.flat_weights(e3) > 0)[0]
    lamp = emit[:2]
    tri = e3.tri.reshape(-1, 3, 3).copy()
    c = tri[lamp].reshape(-1, 3).mean(0)
    tri[lamp] = ((tri[lamp] - c) * np.float32(1.7) + c + np.float32([0.3, -0.05, 0.2])).astype(np.float32)
    tri = tri.reshape(-1)
    n = e3.atlas_res * e3.atlas_res * 4
    atlas = e3.atlas.copy()
    Lr = emitter_layer(e3, emit[-1])
    atlas[Lr * n:(Lr + 1) * n] = np.tile(np.uint8([40, 200, 90, 255]), e3.atlas_res * e3.atlas_res)
    dark_tri = int(np.nonzero(R.flat_weights(e3) == 0)[0][0])
    off = e3.mat.reshape(-1, 12).copy()
    off[:, 1] = e3.mat.reshape(-1, 12)[dark_tri, 1]  # everybody's emissive layer: a black one
    off = off.reshape(-1)
    tri2 = (e3.tri.reshape(-1, 3) * np.float32([1.0, 1.0, 1.6])).astype(np.float32).reshape(-1)
    _, rebuilt = RB.expected(e3, tri2, None)
    return {
        "geometry": (lambda sc: sc.update_geometry(tri), dataclasses.replace(e3, tri=tri, bvh=RF.refit(e3.bvh, tri))),
        "colour": (lambda sc: sc.update_materials(e3.mat, None, atlas, e3.atlas_res, e3.atlas_layers), dataclasses.replace(e3, atlas=atlas)),
        "off": (lambda sc: sc.update_materials(off, None, e3.atlas, e3.atlas_res, e3.atlas_layers), dataclasses.replace(e3, mat=off)),
        "rebuild": (lambda sc: sc.rebuild_geometry(tri2), rebuilt),
    }


@pytest.mark.parametrize("case", ["geometry", "colour", "off", "rebuild"])
def test_live_update_equals_a_fresh_scene(scenes, case):
    e3 = scenes["e3"]
    change, fresh_arrays = e3_cases(e3)[case]
    A = gpu_scene(e3)
    pa = make_pt(A)
    t0 = A.light_table()
    first = live_frame(pa)
    change(A)
    ta, fa = A.light_table(), live_frame(pa)
    d2h, h2d, _ = A.light_build_stats()
    assert d2h <= 16 and h2d == 0
    B = gpu_scene(fresh_arrays)
    pb = make_pt(B)
    tb, fb = B.light_table(), live_frame(pb)
    for key in KEYS:
        assert same(ta[key], tb[key]), key
    check_against_restatement(ta)
    assert np.array_equal(fa, fb), int((fa != fb).any(-1).sum())
    assert not np.array_equal(fa, first)
    if case == "off":
        assert ta["tris"].size == 0 and A.light_count() == 0 and not ta["pick"].any()
        pa.set_lights("off")
        assert np.array_equal(live_frame(pa), fa)  # n = 0: the bits of FSPT_LIGHTS_OFF
    else:
        assert ta["tris"].size > 0 and not all(same(ta[k], t0[k]) for k in ("weights", "prob", "pick"))
    if case == "rebuild":
        assert not np.array_equal(ta["slot_tri"], t0["slot_tri"])
    pa.close(); pb.close(); A.close(); B.close()


# ---- switching builders ------------------------------------------------------------------------------------------------
def test_switching_builders_on_a_live_scene(scenes):
    e3 = scenes["e3"]
    sc = Scene(e3)
    pt = make_pt(sc)
    th, fh = sc.light_table(), live_frame(pt)
    d2h, h2d, _ = sc.light_build_stats()
    assert d2h == 4 * (th["slot_tri"].size + th["weights"].size) and h2d > 0
    sc.set_light_builder("gpu")
    tg, fg = sc.light_table(), live_frame(pt)
    assert sc.light_build_stats()[:2] == (8, 0)
    check_against_restatement(tg)
    assert not (same(tg["prob"], th["prob"]) and np.array_equal(tg["alias"], th["alias"]))  # an alias table is not unique
    assert np.isfinite(fg).all() and fg[..., :3].max() > 0
    sc.set_light_builder("host")
    t1, f1 = sc.light_table(), live_frame(pt)
    for key in KEYS:
        assert same(t1[key], th[key]), key
    assert np.array_equal(f1, fh)
    with pytest.raises(FsptError):
        L.check(L.lib().fspt_scene_set_light_builder(sc._h, 2))
    assert sc.light_builder == "host"
    pt.close(); sc.close()


@pytest.mark.parametrize("name", ["e1", "e3"])
def test_a_scene_that_never_opts_in_has_the_host_table(scenes, name):
    sc = Scene(scenes[name])
    assert sc.light_builder == "host"
    t = sc.light_table()
    prob, alias = light_alias_table(t["weights"][t["tris"]])
    assert same(t["prob"], prob) and np.array_equal(t["alias"], alias)
    assert same(R.device_table(t)["light_p"], O.realised_p(prob, alias))
    sc.close()
