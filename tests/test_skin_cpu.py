"""GPU skinning, what needs no device: the rule's restatement against float64 under its counted bound,
similarities, a single joint against the part-transform rule, fspt_skin_check_eval's refusals and accepted corners,
the Python hosts' argument checks, NULL handles."""
import ctypes as C

import numpy as np
import pytest

import pose_ref as PR
import skin_ref as SR
from fspt_amd import _lib as L
from fspt_amd import scene as S
from fspt_amd.tracer import MultiPathTracer, Scene

U = 2.0 ** -24


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return S._rotation_matrix(axis, angle)


def xf_of(A, t=(0, 0, 0)):
    return np.concatenate([np.asarray(A, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(np.float32).reshape(12)


def random_skin(T, n_joints, n_morph, seed, morph_norm=True):
    rng = np.random.default_rng(seed)
    joints = rng.integers(0, n_joints, (T, 3, 4)).astype(np.uint16)
    weights = rng.dirichlet(np.ones(4), (T, 3)).astype(np.float32)
    tri = rng.normal(0, 2, (T, 9)).astype(np.float32)
    norm = rng.normal(0, 1, (T, 27)).astype(np.float32)
    xf = np.stack([xf_of(rot(rng.normal(0, 1, 3), rng.uniform(-1, 1)) * rng.uniform(0.5, 2.0), rng.normal(0, 1, 3)) for _ in range(n_joints)])
    morph = rng.normal(0, 0.3, (n_morph, T, 9)).astype(np.float32) if n_morph else None
    mnorm = rng.normal(0, 0.3, (n_morph, T, 27)).astype(np.float32) if n_morph and morph_norm else None
    mw = rng.uniform(-1, 1, n_morph).astype(np.float32) if n_morph else None
    return joints, weights, tri, norm, xf, morph, mnorm, mw


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_morph,signed", ((0, False), (3, False), (2, True)))
def test_float32_rule_is_within_the_counted_bound_of_float64(n_morph, signed):
    j, w, tri, norm, xf, morph, mnorm, mw = random_skin(200, 7, n_morph, 11 + n_morph)
    if signed:  # weights of both signs: the blend cancels in part, the magnitudes in the bound do not
        w = (w * np.where(np.arange(4) % 2, -0.6, 1.0)).astype(np.float32)
    t32, n32 = SR.skin(j, w, tri, norm, xf, morph, mnorm, mw)
    t64, n64, bt, bn = SR.skin64(j, w, tri, norm, xf, morph, mnorm, mw)
    assert t32.dtype == np.float32 and n32.dtype == np.float32 and np.isfinite(bn).all()
    et, en = np.abs(t32 - t64), np.abs(n32 - n64)
    print(f"n_morph {n_morph} signed {signed}: worst error / bound: tri {np.max(et / bt):.3f}, norm {np.max(en / bn):.3f}")
    assert (et <= bt).all() and (en <= bn).all()
    assert et.max() > 0 and en.max() > 0  # (float32 it is)
    # without a rest norm the vertices are the same words
    t2, n2 = SR.skin(j, w, tri, None, xf, morph, None, mw)
    assert n2 is None and np.array_equal(t2.view(np.uint32), t32.view(np.uint32))


@pytest.mark.parametrize("scale", (1.0, 0.37, 250.0))
def test_similarity_gives_the_rotation(scale):
    """D = N = R for s R with one-hot weights: the frame of a rotated, uniformly scaled joint is the rotated rest frame"""
    R = rot([1, 2, -0.5], 0.83) @ rot([0, 1, 0], -2.1)
    xf = np.stack([xf_of(np.eye(3)), xf_of(R * scale, (1, 2, 3))])
    T = 4
    joints = np.ones((T, 3, 4), np.uint16); joints[:, :, 1:] = 0
    weights = np.zeros((T, 3, 4), np.float32); weights[:, :, 0] = 1.0
    norm = np.tile(np.eye(3, dtype=np.float32).reshape(9), T * 3).reshape(T, 27)  # n, t, bt = e_x, e_y, e_z
    tri = np.random.default_rng(1).normal(0, 1, (T, 9)).astype(np.float32)
    t32, n32 = SR.skin(joints, weights, tri, norm, xf)
    t64, n64, bt, bn = SR.skin64(joints, weights, tri, norm, xf)
    want = np.tile(R.T.reshape(9), T * 3).reshape(T, 27)  # column v of R per frame vector v
    # the float64 rule on the float32 matrix against R: every entry of float32(s R) and hence g is off by u relatively: 2 u for D, 3 u for N
    assert np.abs(n64 - want).max() <= 4 * U
    assert (np.abs(n32 - n64) <= bn).all()
    want_t = tri.reshape(-1, 3).astype(np.float64) @ xf[1].reshape(3, 4)[:, :3].astype(np.float64).T + xf[1].reshape(3, 4)[:, 3]
    assert (np.abs(t32.reshape(-1, 3) - want_t) <= bt.reshape(-1, 3)).all()


@pytest.mark.parametrize("which", ("rotate", "scale", "shear_mirror"))
def test_single_joint_agrees_with_the_part_transform_rule(which):
    """One joint with weight 1 (the other three slots weigh 0): B is the matrix itself, so the vertices are pose_ref's words;
    the frames differ only in where D and N are derived (float64 on the host there, float32 per corner here), each within
    its own counted bound of the exact value."""
    A = {"rotate": rot([1, 2, -0.5], 0.83), "scale": 0.37 * np.eye(3),
         "shear_mirror": (np.diag([1.3, 0.6, 0.9]) + np.array([[0, 0.4, 0], [0, 0, 0], [0.1, 0, 0]])) @ np.diag([1.0, -1.0, 1.0])}[which]
    xf = xf_of(A, (0.05, -0.03, 0.02))
    rng = np.random.default_rng(9)
    T = 50
    tri = rng.normal(0, 2, (T, 9)).astype(np.float32)
    norm = rng.normal(0, 1, (T, 27)).astype(np.float32)
    joints = np.zeros((T, 3, 4), np.uint16)
    weights = np.zeros((T, 3, 4), np.float32); weights[:, :, 0] = 1.0
    t32, n32 = SR.skin(joints, weights, tri, norm, xf.reshape(1, 12))
    pt, pn = PR.pose(np.zeros(T, np.int64), tri, norm, xf.reshape(1, 12))
    assert np.array_equal(t32.view(np.uint32), pt.view(np.uint32))
    _, n64, _, bn = SR.skin64(joints, weights, tri, norm, xf.reshape(1, 12))
    _, pbn = SR.pose_bound(tri, norm, xf)
    assert (np.abs(n32 - n64) <= bn).all() and (np.abs(pn - n64) <= pbn).all()
    assert (np.abs(n32.astype(np.float64) - pn) <= bn + pbn).all()


def test_identity_reproduces_the_rest_mesh_under_one_hot_and_dyadic_weights():
    j, _, tri, norm, _, _, _, _ = random_skin(40, 5, 0, 3)
    tri[0, 0] = -0.0
    xf = np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (5, 1))
    for w in ((1, 0, 0, 0), (0, 0, 1, 0), (0.5, 0.25, 0.125, 0.125)):
        weights = np.tile(np.float32(w), (40, 3, 1))
        t, n = SR.skin(j, weights, tri, norm, xf)
        assert (t == tri).all() and (n == norm).all()


# ---- fspt_skin_check_eval --------------------------------------------------------------------------------------------
def check(T, joints, weights, n_joints, tri, norm=None, morph=None, morph_norm=None, n_morph=0):
    f = lambda a: None if a is None else L.fptr(a)
    d = L.SkinDesc(None if joints is None else joints.ctypes.data_as(C.POINTER(C.c_uint16)), f(weights), n_joints, f(tri), f(norm), f(morph), f(morph_norm), n_morph)
    bad = C.c_uint64(0xFFFFFFFF)
    rc = L.lib().fspt_skin_check_eval(C.byref(d), T, C.byref(bad))
    return rc, int(bad.value), L.lib().fspt_last_error().decode()


def good(T, n_morph=2):
    j, w, tri, norm, _, morph, mnorm, _ = random_skin(T, 9, n_morph, 21)
    return dict(joints=j.reshape(-1).copy(), weights=w.reshape(-1).copy(), n_joints=9, tri=tri.reshape(-1).copy(), norm=norm.reshape(-1).copy(),
                morph=morph.reshape(-1).copy(), morph_norm=mnorm.reshape(-1).copy(), n_morph=n_morph)


@pytest.mark.parametrize("T", (1, 22))
def test_check_accepts_a_good_skin_and_the_corners(T):
    g = good(T)
    assert check(T, **g)[0] == 0
    assert check(T, **dict(g, norm=None, morph_norm=None))[0] == 0
    assert check(T, **dict(g, morph=None, morph_norm=None, n_morph=0))[0] == 0
    assert check(T, **dict(g, weights=np.zeros(T * 12, np.float32)))[0] == 0                 # weights all zero
    assert check(T, **dict(g, weights=-g["weights"]))[0] == 0                                  # negative weights
    top = g["joints"].copy(); top[-1] = 65534
    assert check(T, **dict(g, joints=top, n_joints=65535))[0] == 0                             # the largest table
    assert check(T, **dict(g, n_joints=1, joints=np.zeros(T * 12, np.uint16)))[0] == 0
    g64 = good(T, 64)
    assert check(T, **g64)[0] == 0                                                             # FSPT_SKIN_MAX_MORPH targets


@pytest.mark.parametrize("T", (1, 22))
def test_check_refuses_naming_the_index(T):
    g = good(T)
    last = T * 12 - 1
    for at in (0, last // 2, last):
        j = g["joints"].copy(); j[at] = 9
        rc, bad, msg = check(T, **dict(g, joints=j))
        assert rc == -1 and bad == at and f"joints[{at}] = 9" in msg
    j = g["joints"].copy(); j[last] = 65535
    rc, bad, msg = check(T, **dict(g, joints=j, n_joints=65535))
    assert rc == -1 and bad == last and f"joints[{last}]" in msg
    for name, per in (("weights", 12), ("tri", 9), ("norm", 27), ("morph", 18), ("morph_norm", 54)):
        for at in (0, T * per - 1):
            for v in (np.nan, np.inf, -np.inf):
                a = g[name].copy(); a[at] = v
                rc, bad, msg = check(T, **dict(g, **{name: a}))
                assert rc == -1 and bad == at and f"{name}[{at}] is not finite" in msg, (name, at, msg)
    for n_joints in (0, 65536, 1 << 20):
        rc, _, msg = check(T, **dict(g, n_joints=n_joints))
        assert rc == -1 and "n_joints" in msg
    g65 = good(T, 65)
    rc, _, msg = check(T, **g65)
    assert rc == -1 and "n_morph = 65" in msg
    rc, _, msg = check(T, **dict(g, norm=None))
    assert rc == -1 and "morph_norm needs a rest norm" in msg
    rc, _, msg = check(T, **dict(g, morph=None))
    assert rc == -1 and "morph is NULL" in msg
    for missing in ("joints", "weights", "tri"):
        rc, _, msg = check(T, **dict(g, **{missing: None}))
        assert rc == -1 and "NULL" in msg
    assert L.lib().fspt_skin_check_eval(None, T, None) == -1


def test_form_switch_takes_0_and_1():
    lib = L.lib()
    assert lib.fspt_skin_set_form(2) == -1 and lib.fspt_skin_set_form(-1) == -1
    assert lib.fspt_skin_set_form(1) == 0 and lib.fspt_skin_set_form(0) == 0


# ---- the Python hosts' argument checks (no call reaches the library) -------------------------------------------------
class _Arrays:
    n_tris = 2
    tri = np.zeros(18, np.float32)
    norm = np.zeros(54, np.float32)


def _host(cls):
    h = cls.__new__(cls)
    h.arrays = _Arrays()
    h.device = 0
    h._h = h._m = None  # a call that got past the checks would be refused by the library: NULL handle
    return h


@pytest.mark.parametrize("cls", (Scene, MultiPathTracer))
def test_python_argument_checks(cls):
    h = _host(cls)
    j, w = np.zeros((2, 3, 4), np.int64), np.zeros((2, 3, 4), np.float32)
    with pytest.raises(ValueError, match="without weights"):
        h.set_skin(j)
    with pytest.raises(ValueError, match="3 x 4"):
        h.set_skin(j[:1], w)
    with pytest.raises(ValueError, match="3 x 4"):
        h.set_skin(j, w[:1])
    with pytest.raises(TypeError, match="integers"):
        h.set_skin(j.astype(np.float32), w)
    with pytest.raises(ValueError, match="65535"):
        h.set_skin(j + 65536, w)
    with pytest.raises(ValueError):
        h.set_skin(j - 1, w)
    with pytest.raises(ValueError, match="x 9"):
        h.set_skin(j, w, np.zeros(9, np.float32))
    with pytest.raises(ValueError, match="x 27"):
        h.set_skin(j, w, np.zeros(18, np.float32), np.zeros(27, np.float32))
    with pytest.raises(ValueError, match="norm given without tri"):
        h.set_skin(j, w, None, np.zeros(54, np.float32))
    with pytest.raises(ValueError, match="n_morph x 2 x 9"):
        h.set_skin(j, w, morph=np.zeros(19, np.float32))
    with pytest.raises(ValueError, match="morph_norm has"):
        h.set_skin(j, w, morph=np.zeros(36, np.float32), morph_norm=np.zeros(54, np.float32))
    with pytest.raises(ValueError, match="morph_norm needs a rest norm"):
        h.set_skin(j, w, np.zeros(18, np.float32), None, np.zeros(18, np.float32), np.zeros(54, np.float32))
    with pytest.raises(ValueError, match="n_joints"):
        h.set_skin(j, w, n_joints=0)
    with pytest.raises(ValueError, match="n_joints"):
        h.set_skin(j, w, n_joints=65536)
    with pytest.raises(ValueError, match="n_joints x 12"):
        h.update_skin(np.zeros(13, np.float32))
    with pytest.raises(ValueError, match="n_joints x 12"):
        h.update_skin(np.zeros(0, np.float32))
    with pytest.raises(L.FsptError):  # past the checks: the library sees the NULL handle
        h.set_skin(j, w)
    with pytest.raises(L.FsptError):
        h.update_skin(np.zeros(12, np.float32), np.zeros(1, np.float32))
    if cls is Scene:
        h._moved = True
        with pytest.raises(ValueError, match="no longer that of its arrays"):
            h.set_skin(j, w)


# ---- NULL handles, no device -----------------------------------------------------------------------------------------
def test_null_handles_are_refused_without_a_device():
    lib = L.lib()
    one = np.zeros(12, np.float32)
    assert lib.fspt_scene_set_skin(None, None) == -1
    assert lib.fspt_scene_update_skin(None, L.fptr(one), 1, None, 0) == -1
    assert lib.fspt_scene_update_skin_device(None, None, 1, None, 0) == -1
    assert lib.fspt_scene_read_skin(None, L.fptr(one), None) == -1
    assert lib.fspt_scene_last_skin_ms(None, None, None, None, None) == -1
    assert lib.fspt_multi_set_skin(None, None) == -1
    assert lib.fspt_multi_update_skin(None, L.fptr(one), 1, None, 0) == -1
