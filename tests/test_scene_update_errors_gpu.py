"""Every host-side refusal of the entries that change a live scene (refit, rebuild, pose, skin, appearance, motion origin and
their read-outs): the code AND the full text of fspt_last_error, one rule broken at a time on the `small` scene - plus calls
that break two rules, which must report the one checked first.  Refusals only: every call returns before it launches.

EXPECT is a literal table.  It was filled from a library built from the commit BEFORE these entries moved to
fspt_scene_update.cpp (tools/build_ab.sh, FSPT_LIB), never from the code under test: the order of an entry's checks and
the entry name in each text are part of its behaviour."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from fspt_amd import Scene
from fspt_amd import _lib as L

pytestmark = pytest.mark.gpu

NOT_REFITTABLE = "scene is not refittable (the leaves' triStarts must be distinct and tile [0, n_tris), every node have one parent)"
NOT_REBUILDABLE = ("scene is not refittable (the leaves' triStarts must be distinct and tile [0, n_tris) in steps of at most leaf_size, "
                   "every node have one parent)")
ON_DEVICE = "a value of tri / norm is not finite (scene unchanged)"
UG, UGD = "fspt_scene_update_geometry", "fspt_scene_update_geometry_device"
RG, RGD = "fspt_scene_rebuild_geometry", "fspt_scene_rebuild_geometry_device"
SP, UT, RP = "fspt_scene_set_pose", "fspt_scene_update_transforms", "fspt_scene_read_pose"
SS, US, USD, RS = "fspt_scene_set_skin", "fspt_scene_update_skin", "fspt_scene_update_skin_device", "fspt_scene_read_skin"
UM, UE, RA = "fspt_scene_update_materials", "fspt_scene_update_environment", "fspt_scene_read_appearance"

# case -> (code, text).  -1 FSPT_E_INVALID, -6 FSPT_E_STATE.
EXPECT = {
    # in-place geometry update
    "ug_null_tri": (-1, f"{UG}: NULL scene or tri"),
    "ugd_null_tri": (-1, f"{UGD}: NULL scene or tri"),
    "ug_tri_nan": (-1, f"{UG}: tri[37] is not finite"),
    "ug_norm_inf": (-1, f"{UG}: norm[64] is not finite"),
    "ugd_tri_nan": (-1, f"{UGD}: {ON_DEVICE}"),
    "ugd_norm_inf": (-1, f"{UGD}: {ON_DEVICE}"),
    "ug_not_refittable": (-6, f"{UG}: {NOT_REFITTABLE}"),
    "ugd_not_refittable": (-6, f"{UGD}: {NOT_REFITTABLE}"),
    "ug_two_rules": (-1, f"{UG}: tri[37] is not finite"),  # non-finite AND not refittable: the finite check comes first
    "ug_tri_and_norm": (-1, f"{UG}: tri[37] is not finite"),  # both arrays bad: tri is checked first
    # in-place rebuild
    "rg_null_tri": (-1, f"{RG}: NULL scene or tri"),
    "rgd_null_tri": (-1, f"{RGD}: NULL scene or tri"),
    "rg_tri_nan": (-1, f"{RG}: tri[37] is not finite"),
    "rg_norm_inf": (-1, f"{RG}: norm[64] is not finite"),
    "rgd_tri_nan": (-1, f"{RGD}: {ON_DEVICE}"),
    "rgd_norm_inf": (-1, f"{RGD}: {ON_DEVICE}"),
    "rg_not_refittable": (-6, f"{RG}: {NOT_REBUILDABLE}"),
    "rg_two_rules": (-1, f"{RG}: tri[37] is not finite"),
    # part transforms
    "sp_not_refittable": (-6, f"{SP}: {NOT_REFITTABLE}"),
    "sp_part_range": (-1, f"{SP}: part[5] = 3, n_parts = 3"),
    "sp_tri_nan": (-1, f"{SP}: tri[37] is not finite"),
    "sp_norm_inf": (-1, f"{SP}: norm[64] is not finite"),
    "sp_null_tri": (-1, f"{SP}: tri is NULL or n_parts is 0"),
    "sp_no_parts": (-1, f"{SP}: tri is NULL or n_parts is 0"),
    "sp_two_rules": (-1, f"{SP}: part[5] = 3, n_parts = 3"),  # a part id out of range AND a non-finite tri
    "ut_no_pose": (-6, f"{UT}: the scene has no pose (fspt_scene_set_pose)"),
    "ut_count": (-1, f"{UT}: 2 matrices, the pose has 3 parts"),
    "ut_not_finite": (-1, f"{UT}: part 1: an entry is not finite (scene unchanged)"),
    "ut_singular": (-1, f"{UT}: part 2: the matrix is singular (scene unchanged)"),
    "rp_before_update": (-6, f"{RP}: no fspt_scene_update_transforms since the pose was set, the scene rebuilt or its geometry uploaded"),
    "rp_no_rest_norm": (-6, f"{RP}: the pose has no rest norm"),
    # skinning: one case per line of the validation
    "ss_not_refittable": (-6, f"{SS}: {NOT_REFITTABLE}"),
    "ss_null_joints": (-1, f"{SS}: joints, weights or tri is NULL"),
    "ss_n_joints": (-1, f"{SS}: n_joints = 0, must lie in [1, 65535]"),
    "ss_n_morph": (-1, f"{SS}: n_morph = 65, at most 64"),
    "ss_morph_null": (-1, f"{SS}: n_morph = 1 but morph is NULL"),
    "ss_morph_norm_needs_norm": (-1, f"{SS}: morph_norm needs a rest norm"),
    "ss_morph_norm_no_morph": (-1, f"{SS}: morph_norm given with n_morph = 0"),
    "ss_joint_range": (-1, f"{SS}: joints[17] = 2, n_joints = 2"),
    "ss_weights_nan": (-1, f"{SS}: weights[11] is not finite"),
    "ss_tri_nan": (-1, f"{SS}: tri[37] is not finite"),
    "ss_norm_inf": (-1, f"{SS}: norm[64] is not finite"),
    "ss_morph_nan": (-1, f"{SS}: morph[40] is not finite"),
    "ss_morph_norm_nan": (-1, f"{SS}: morph_norm[70] is not finite"),
    "us_no_skin": (-6, f"{US}: the scene has no skin (fspt_scene_set_skin)"),
    "usd_no_skin": (-6, f"{USD}: the scene has no skin (fspt_scene_set_skin)"),
    "us_joint_count": (-1, f"{US}: 3 matrices, the skin has 2 joints"),
    "us_morph_count": (-1, f"{US}: 0 morph weights, the skin has 1 targets"),
    "us_null_morph_w": (-1, f"{US}: morph_w is NULL, the skin has 1 targets"),
    "usd_misaligned": (-1, f"{USD}: xf must be 16-byte aligned"),
    "us_joint_nan": (-1, f"{US}: joint 1: an entry is not finite (scene unchanged)"),
    "us_weight_nan": (-1, f"{US}: morph target 0: its weight is not finite (scene unchanged)"),
    "rs_before_update": (-6, f"{RS}: no fspt_scene_update_skin since the skin was set, the scene rebuilt, posed or its geometry uploaded"),
    "rs_no_rest_norm": (-6, f"{RS}: the skin has no rest norm"),
    # appearance
    "um_null_mat": (-1, f"{UM}: NULL scene or mat"),
    "um_atlas_zero": (-1, f"{UM}: atlas must have at least one layer"),
    "um_no_atlas": (-6, f"{UM}: atlas is NULL and no earlier call of this scene carried one"),
    "ue_no_bins": (-1, f"{UE}: radianceBins must hold at least one bin (main.js:292)"),
    "ue_zero_bins": (-1, f"{UE}: radianceBins must hold at least one bin (main.js:292)"),
    "ue_env_zero": (-1, f"{UE}: env given with zero size"),
    "ra_what": (-1, f"{RA}: NULL scene or what not in [0, 5]"),
    "ra_what_negative": (-1, f"{RA}: NULL scene or what not in [0, 5]"),
    # NULL scene
    "null_last_update_ms": (-1, "fspt_scene_last_update_ms: NULL scene"),
    "null_last_pose_ms": (-1, "fspt_scene_last_pose_ms: NULL scene"),
    "null_last_skin_ms": (-1, "fspt_scene_last_skin_ms: NULL scene"),
    "null_last_rebuild_ms": (-1, "fspt_scene_last_rebuild_ms: NULL scene"),
    "null_last_appearance_ms": (-1, "fspt_scene_last_appearance_ms: NULL scene"),
    "null_sah_cost": (-1, "fspt_scene_sah_cost: NULL argument"),
    "null_motion_begin": (-1, "fspt_scene_motion_begin: NULL scene"),
    "null_motion_end": (-1, "fspt_scene_motion_end: NULL scene"),
}


class Ctx:
    """The scenes every case shares (a refusal leaves its scene as it was) and the arrays the calls are made of."""

    def __init__(self, arrays):
        import torch
        self.torch = torch
        self.lib = lib = L.lib()
        self.arrays = arrays
        self.T = T = int(arrays.n_tris)
        assert T >= 8
        self.tri, self.norm = arrays.tri.astype(np.float32), arrays.norm.astype(np.float32)
        self.plain = Scene(arrays)
        # two leaves that share a triStart: the scene renders, but cannot be refitted (tests/test_refit_gpu.py)
        bvh = arrays.bvh.copy().reshape(-1, 9)
        w = bvh[:, :3].view(np.int32)
        leaves = np.flatnonzero(w[:, 2] > -1)
        w[leaves[1], 2] = w[leaves[0], 2]
        self.shared = Scene(dataclasses.replace(arrays, bvh=bvh.reshape(-1)))
        self.part = (np.arange(T, dtype=np.uint32) % 3).astype(np.uint32)
        self.ident = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), 3)
        # a pose that was never run; a pose without rest normals, run once
        self.posed = Scene(arrays)
        assert lib.fspt_scene_set_pose(self.posed._h, L.u32ptr(self.part), 3, L.fptr(self.tri), L.fptr(self.norm)) == 0
        self.posed_no_norm = Scene(arrays)
        assert lib.fspt_scene_set_pose(self.posed_no_norm._h, L.u32ptr(self.part), 3, L.fptr(self.tri), None) == 0
        assert lib.fspt_scene_update_transforms(self.posed_no_norm._h, L.fptr(self.ident), 3) == 0
        # a skin of 2 joints and 1 morph target without rest normals: never run, and run once
        self.joints = np.zeros(T * 12, np.uint16)
        self.weights = np.tile(np.float32([1, 0, 0, 0]), T * 3)
        self.morph = np.zeros(T * 9, np.float32)
        self.morph_norm = np.zeros(T * 27, np.float32)
        self.xf2 = self.ident[:24].copy()
        self.mw = np.zeros(1, np.float32)
        self.skin_set, self.skinned = Scene(arrays), Scene(arrays)
        for sc in (self.skin_set, self.skinned):
            assert self.set_skin(sc) == 0
        assert lib.fspt_scene_update_skin(self.skinned._h, L.fptr(self.xf2), 2, L.fptr(self.mw), 1) == 0
        self.scenes = (self.plain, self.shared, self.posed, self.posed_no_norm, self.skin_set, self.skinned)

    def bad(self, a, i, v=np.nan):
        a = a.copy()
        a[i] = v
        return a

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(a).to("cuda:0")

    def geometry(self, fn, sc, tri, norm, device=False):
        """update_geometry / rebuild_geometry in either form"""
        f = getattr(self.lib, fn + ("_device" if device else ""))
        extra = (None,) if "rebuild" in fn else ()
        if device:
            dt, dn = self.dev(tri), self.dev(norm)
            self.torch.cuda.synchronize()
            return f(sc._h, dt.data_ptr() if dt is not None else None, dn.data_ptr() if dn is not None else None, *extra)
        return f(sc._h, None if tri is None else L.fptr(tri), None if norm is None else L.fptr(norm), *extra)

    def set_pose(self, sc, part=None, n_parts=3, tri=None, norm=None, null_tri=False):
        part = self.part if part is None else part
        tri = self.tri if tri is None else tri
        return self.lib.fspt_scene_set_pose(sc._h, L.u32ptr(part), n_parts, None if null_tri else L.fptr(tri), None if norm is None else L.fptr(norm))

    def set_skin(self, sc, **over):
        a = dict(joints=self.joints, weights=self.weights, n_joints=2, tri=self.tri, norm=None, morph=self.morph, morph_norm=None, n_morph=1)
        a.update(over)
        d = L.SkinDesc()
        d.joints = None if a["joints"] is None else a["joints"].ctypes.data_as(C.POINTER(C.c_uint16))
        for k in ("weights", "tri", "norm", "morph", "morph_norm"):
            setattr(d, k, None if a[k] is None else L.fptr(a[k]))
        d.n_joints, d.n_morph = a["n_joints"], a["n_morph"]
        return self.lib.fspt_scene_set_skin(sc._h, C.byref(d))

    def close(self):
        for sc in self.scenes:
            sc.close()


@pytest.fixture(scope="module")
def ctx(small_scene):
    c = Ctx(small_scene)
    yield c
    c.close()


def _ut(c, xf, n=3, sc=None):
    return c.lib.fspt_scene_update_transforms((sc or c.posed)._h, L.fptr(np.ascontiguousarray(xf, np.float32)), n)


def _us(c, sc, xf, nj, mw, nm):
    return c.lib.fspt_scene_update_skin(sc._h, L.fptr(xf), nj, None if mw is None else L.fptr(mw), nm)


def _usd(c, sc, offset=0):
    xf, mw = c.dev(np.concatenate([c.xf2, c.xf2])), c.dev(c.mw)
    c.torch.cuda.synchronize()
    return c.lib.fspt_scene_update_skin_device(sc._h, xf.data_ptr() + offset, 2, mw.data_ptr(), 1)


def _singular(c):
    xf = c.ident.copy()
    xf[24:36] = [1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0]  # part 2: three parallel rows
    return xf


def _buf(c, k):
    return L.fptr(np.zeros(c.T * k, np.float32))


CALLS = {
    "ug_null_tri": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, None, None),
    "ugd_null_tri": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, None, None, device=True),
    "ug_tri_nan": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, c.bad(c.tri, 37), c.norm),
    "ug_norm_inf": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, c.tri, c.bad(c.norm, 64, np.inf)),
    "ugd_tri_nan": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, c.bad(c.tri, 37), c.norm, device=True),
    "ugd_norm_inf": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, c.tri, c.bad(c.norm, 64, np.inf), device=True),
    "ug_not_refittable": lambda c: c.geometry("fspt_scene_update_geometry", c.shared, c.tri, None),
    "ugd_not_refittable": lambda c: c.geometry("fspt_scene_update_geometry", c.shared, c.tri, None, device=True),
    "ug_two_rules": lambda c: c.geometry("fspt_scene_update_geometry", c.shared, c.bad(c.tri, 37), None),
    "ug_tri_and_norm": lambda c: c.geometry("fspt_scene_update_geometry", c.plain, c.bad(c.tri, 37), c.bad(c.norm, 3)),
    "rg_null_tri": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, None, None),
    "rgd_null_tri": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, None, None, device=True),
    "rg_tri_nan": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, c.bad(c.tri, 37), c.norm),
    "rg_norm_inf": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, c.tri, c.bad(c.norm, 64, np.inf)),
    "rgd_tri_nan": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, c.bad(c.tri, 37), c.norm, device=True),
    "rgd_norm_inf": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.plain, c.tri, c.bad(c.norm, 64, np.inf), device=True),
    "rg_not_refittable": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.shared, c.tri, None),
    "rg_two_rules": lambda c: c.geometry("fspt_scene_rebuild_geometry", c.shared, c.bad(c.tri, 37), None),
    "sp_not_refittable": lambda c: c.set_pose(c.shared),
    "sp_part_range": lambda c: c.set_pose(c.plain, part=c.bad(c.part, 5, 3)),
    "sp_tri_nan": lambda c: c.set_pose(c.plain, tri=c.bad(c.tri, 37)),
    "sp_norm_inf": lambda c: c.set_pose(c.plain, norm=c.bad(c.norm, 64, np.inf)),
    "sp_null_tri": lambda c: c.set_pose(c.plain, null_tri=True),
    "sp_no_parts": lambda c: c.set_pose(c.plain, n_parts=0),
    "sp_two_rules": lambda c: c.set_pose(c.plain, part=c.bad(c.part, 5, 3), tri=c.bad(c.tri, 37)),
    "ut_no_pose": lambda c: _ut(c, c.ident, sc=c.plain),
    "ut_count": lambda c: _ut(c, c.ident[:24], 2),
    "ut_not_finite": lambda c: _ut(c, c.bad(c.ident, 12 + 7, np.inf)),
    "ut_singular": lambda c: _ut(c, _singular(c)),
    "rp_before_update": lambda c: c.lib.fspt_scene_read_pose(c.posed._h, _buf(c, 9), None),
    "rp_no_rest_norm": lambda c: c.lib.fspt_scene_read_pose(c.posed_no_norm._h, _buf(c, 9), _buf(c, 27)),
    "ss_not_refittable": lambda c: c.set_skin(c.shared),
    "ss_null_joints": lambda c: c.set_skin(c.plain, joints=None),
    "ss_n_joints": lambda c: c.set_skin(c.plain, n_joints=0),
    "ss_n_morph": lambda c: c.set_skin(c.plain, n_morph=65),
    "ss_morph_null": lambda c: c.set_skin(c.plain, morph=None),
    "ss_morph_norm_needs_norm": lambda c: c.set_skin(c.plain, morph_norm=c.morph_norm),
    "ss_morph_norm_no_morph": lambda c: c.set_skin(c.plain, norm=c.norm, morph_norm=c.morph_norm, n_morph=0),
    "ss_joint_range": lambda c: c.set_skin(c.plain, joints=c.bad(c.joints, 17, 2)),
    "ss_weights_nan": lambda c: c.set_skin(c.plain, weights=c.bad(c.weights, 11)),
    "ss_tri_nan": lambda c: c.set_skin(c.plain, tri=c.bad(c.tri, 37)),
    "ss_norm_inf": lambda c: c.set_skin(c.plain, norm=c.bad(c.norm, 64, np.inf)),
    "ss_morph_nan": lambda c: c.set_skin(c.plain, morph=c.bad(c.morph, 40)),
    "ss_morph_norm_nan": lambda c: c.set_skin(c.plain, norm=c.norm, morph_norm=c.bad(c.morph_norm, 70)),
    "us_no_skin": lambda c: _us(c, c.plain, c.xf2, 2, c.mw, 1),
    "usd_no_skin": lambda c: _usd(c, c.plain),
    "us_joint_count": lambda c: _us(c, c.skin_set, c.ident, 3, c.mw, 1),
    "us_morph_count": lambda c: _us(c, c.skin_set, c.xf2, 2, None, 0),
    "us_null_morph_w": lambda c: _us(c, c.skin_set, c.xf2, 2, None, 1),
    "usd_misaligned": lambda c: _usd(c, c.skin_set, offset=4),
    "us_joint_nan": lambda c: _us(c, c.skin_set, c.bad(c.xf2, 12 + 3), 2, c.mw, 1),
    "us_weight_nan": lambda c: _us(c, c.skin_set, c.xf2, 2, c.bad(c.mw, 0), 1),
    "rs_before_update": lambda c: c.lib.fspt_scene_read_skin(c.skin_set._h, _buf(c, 9), None),
    "rs_no_rest_norm": lambda c: c.lib.fspt_scene_read_skin(c.skinned._h, _buf(c, 9), _buf(c, 27)),
    "um_null_mat": lambda c: c.lib.fspt_scene_update_materials(c.plain._h, None, None, None, 0, 0),
    "um_atlas_zero": lambda c: c.lib.fspt_scene_update_materials(c.plain._h, L.fptr(c.arrays.mat), None, c.arrays.atlas.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 1),
    "um_no_atlas": lambda c: c.lib.fspt_scene_update_materials(c.plain._h, L.fptr(c.arrays.mat), None, None, 0, 0),
    "ue_no_bins": lambda c: c.lib.fspt_scene_update_environment(c.plain._h, None, 0, 0, None, 1),
    "ue_zero_bins": lambda c: c.lib.fspt_scene_update_environment(c.plain._h, None, 0, 0, L.u32ptr(c.arrays.bins), 0),
    "ue_env_zero": lambda c: c.lib.fspt_scene_update_environment(c.plain._h, c.arrays.env.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 32, L.u32ptr(c.arrays.bins), 1),
    "ra_what": lambda c: c.lib.fspt_scene_read_appearance(c.plain._h, 6, None, 0, None),
    "ra_what_negative": lambda c: c.lib.fspt_scene_read_appearance(c.plain._h, -1, None, 0, None),
    "null_last_update_ms": lambda c: c.lib.fspt_scene_last_update_ms(None, None, None),
    "null_last_pose_ms": lambda c: c.lib.fspt_scene_last_pose_ms(None, None, None, None),
    "null_last_skin_ms": lambda c: c.lib.fspt_scene_last_skin_ms(None, None, None, None, None),
    "null_last_rebuild_ms": lambda c: c.lib.fspt_scene_last_rebuild_ms(None, None, None, None, None, None),
    "null_last_appearance_ms": lambda c: c.lib.fspt_scene_last_appearance_ms(None, None, None, None, None),
    "null_sah_cost": lambda c: c.lib.fspt_scene_sah_cost(None, None),
    "null_motion_begin": lambda c: c.lib.fspt_scene_motion_begin(None),
    "null_motion_end": lambda c: c.lib.fspt_scene_motion_end(None),
}


def test_the_table_covers_every_call():
    assert sorted(EXPECT) == sorted(CALLS)


def test_every_refusal_has_its_code_and_text(ctx):
    """One test for the whole table (the scenes are made once; a case is a call that returns at once).  Every mismatch is
    reported, not only the first."""
    wrong = []
    for case, (code, text) in EXPECT.items():
        rc = CALLS[case](ctx)
        got = ctx.lib.fspt_last_error().decode("utf-8", "replace")
        print(f"{case}: {rc} {got!r}")
        if (rc, got) != (code, text):
            wrong.append((case, rc, got, code, text))
    assert not wrong, wrong


def test_the_refusals_left_the_scenes_as_they_were(ctx):
    """(after the table) the plain scene still takes a valid update, the posed and skinned ones still hold what they held"""
    lib = ctx.lib
    assert lib.fspt_scene_update_geometry(ctx.plain._h, L.fptr(ctx.tri), L.fptr(ctx.norm)) == 0
    assert lib.fspt_scene_read_pose(ctx.posed_no_norm._h, _buf(ctx, 9), None) == 0  # still posed / skinned
    assert lib.fspt_scene_read_skin(ctx.skinned._h, _buf(ctx, 9), None) == 0
    assert _ut(ctx, ctx.ident) == 0  # the never-run pose and skin are intact: they run
    assert _us(ctx, ctx.skin_set, ctx.xf2, 2, ctx.mw, 1) == 0
