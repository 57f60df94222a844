"""What fspt_scene_create puts on the device, byte for byte: per scene a sha256 of each buffer Scene.read_appearance returns
(texture-set table, single-layer atlas, interleaved atlas, environment, bins, hit records), of slot_triangles, depth,
two_level_nodes, sah_cost and the emitter light table, and of intersect (t, index, steps together) for 256 fixed rays in both
node forms where the scene has two-level nodes.  The scenes cover both atlas forms at a size that is a multiple of neither
tile, an environment that is a multiple of neither tiling, none at all, another leaf size and refused two-level nodes.

EXPECT is a literal table.  It was filled on an MI355X from a library built from the commit BEFORE fspt_scene_create moved
to fspt_scene.cpp and became named steps (tools/build_ab.sh, FSPT_LIB), never from the code under test.  On that build each
scene did what its description says; the observed counts stand next to its rows."""
import dataclasses
import hashlib

import numpy as np
import pytest

from conftest import random_rays
from fspt_amd import Scene
from fspt_amd import _lib as L
from fspt_amd import scene as S

pytestmark = pytest.mark.gpu

SCENES = ("a_small", "b_atlas6", "c_env10x5", "d_no_env", "e_leaf1", "f_no_quads")
QUAD_IMAGE_BYTES = 2 * 3 * 128  # one interleaved image at res 6: ceil(6 / 4) x ceil(6 / 2) tiles of 128 bytes


def arrays_of(name, small):
    if name == "b_atlas6":
        # five layers of 6 x 6 texels: 0 a flat colour, 1 - 4 images; three texture sets in first-appearance order:
        # (1, 2, 4, 3) four images, (2, 3, 0, 0) two, (1, 0, 0, 0) one - under a budget of one interleaved image the first
        # is QUAD and the other two SEPARATE
        rng = np.random.default_rng(6)
        atlas = rng.integers(0, 256, (5, 6, 6, 4), dtype=np.uint8)
        atlas[0] = (10, 20, 30, 255)
        mat = small.mat.reshape(-1, 12).copy()
        third = len(mat) // 3
        mat[:third, 0:4] = (1, 2, 3, 4)
        mat[third:2 * third, 0:4] = (2, 3, 0, 0)
        mat[2 * third:, 0:4] = (1, 0, 0, 0)
        return dataclasses.replace(small, atlas=atlas.reshape(-1), atlas_res=6, atlas_layers=5, mat=mat.reshape(-1))
    if name == "c_env10x5":
        env = np.random.default_rng(10).integers(0, 256, 10 * 5 * 4, dtype=np.uint8)
        return dataclasses.replace(small, env=env, env_w=10, env_h=5)
    if name == "d_no_env":
        return dataclasses.replace(small, env=None, env_w=0, env_h=0)
    if name == "e_leaf1":
        texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(8), "synthetic/quad.obj": S.QUAD_OBJ}
        env, w, h = S.synthetic_env(64, 32, sun_deg=1.5, sun_gain=60.0)
        return S.build_scene(S.bunny_props(), texts, env=env, env_w=w, env_h=h, leaf_size=1)
    if name == "f_no_quads":
        bvh = small.bvh.copy()
        assert bvh.view(np.int32)[1 * 9 + 2] <= -1  # node 1, the root's left child, is an interior node:
        bvh[1 * 9 + 6] = np.nextafter(bvh[1 * 9 + 6], np.float32(np.inf))  # its box's max.x, one ulp up - no longer the union
        return dataclasses.replace(small, bvh=bvh)
    return small


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def digests(arrays):
    """name -> sha256 of what a scene created from `arrays` holds, and (two-level nodes present, kinds of its texture sets)"""
    sc = Scene(arrays)
    try:
        d = {what: sha(sc.read_appearance(what)) for what in Scene.APPEARANCE}
        two_level, two_level_bytes = sc.two_level_nodes()
        lt = sc.light_table()
        d["slot_triangles"] = sha(sc.slot_triangles())
        d["depth"] = sha(np.uint32(sc.depth))
        d["two_level_nodes"] = sha(np.uint64([two_level, two_level_bytes]))
        d["sah_cost"] = sha(np.float64(sc.sah_cost()))
        d["light_table"] = sha(*(lt[k] for k in ("weights", "prob", "alias", "tris", "pick", "slot_tri")))
        rays = random_rays(arrays, 256, seed=0)
        for form in range(2 if two_level else 1):
            t, index, steps, _ = sc.intersect(rays, two_level=bool(form))
            d[f"intersect_form{form}"] = sha(t, index, steps)
        kinds = sc.read_appearance("tex_sets").view(np.uint32).reshape(-1, 12)[:, 0].tolist()
        return d, two_level, kinds
    finally:
        sc.close()


# scene -> {what -> sha256}
EXPECT = {
    # observed on the parent build: two-level nodes present; texture sets: 0 QUAD, 0 SEPARATE, 2 CONST
    "a_small": {
        "tex_sets": "588775c183e07cb7ee0d4cf2e0b0c21b28cf6d75f1386c3932f21ebdef4d82f2",
        "atlas": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "atlas4": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "env": "0a48d3b5fa31997bebaccf434f682719381829b3fb7844a7bd1b186ee3a3afed",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "c3a5dabe936576773242c12a5305c7fa05f754b43c761b5718521e8375453e08",
        "slot_triangles": "99cdb3907a49ff8c7429e19a0d4889b14b51a93a2864d5a1e63fc5e72596146a",
        "depth": "075de2b906dbd7066da008cab735bee896370154603579a50122f9b88545bd45",
        "two_level_nodes": "71fe95d0b18161bd0f8e884070df525e31c4f53cc61ed36ab376cd3be0465738",
        "sah_cost": "ac622ec1a8c6566eccd88fb8a04e25380ef7216f901040cf0572f1c63b54f437",
        "light_table": "10e27f0568d52c9f8825b020718383bce39a2789b26dd0d5b0fb4272a88e68b2",
        "intersect_form0": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
        "intersect_form1": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
    },
    # observed on the parent build: two-level nodes present; texture sets: 1 QUAD, 2 SEPARATE, 0 CONST
    "b_atlas6": {
        "tex_sets": "54eb3207bfb13e4f9a09f851be9a2e10a07e242d8e82146bd75719e02ee2ca29",
        "atlas": "387359954d1a02f554394c9f213042078f34e3dfd8fa6dccd606cb2ac707acf2",
        "atlas4": "ad8c53719b42a98ace28cdb94faed8d06ca846876c17560f3338729ac837ce1e",
        "env": "0a48d3b5fa31997bebaccf434f682719381829b3fb7844a7bd1b186ee3a3afed",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "66210e6bf393edd5aa1dee8827c5736b3413a5cbe46df88bf4271ffca75a2695",
        "slot_triangles": "99cdb3907a49ff8c7429e19a0d4889b14b51a93a2864d5a1e63fc5e72596146a",
        "depth": "075de2b906dbd7066da008cab735bee896370154603579a50122f9b88545bd45",
        "two_level_nodes": "71fe95d0b18161bd0f8e884070df525e31c4f53cc61ed36ab376cd3be0465738",
        "sah_cost": "ac622ec1a8c6566eccd88fb8a04e25380ef7216f901040cf0572f1c63b54f437",
        "light_table": "4c94794c02c10ecdf084002aede66089446c6fb88bd262f997b48fc4a3bc43df",
        "intersect_form0": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
        "intersect_form1": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
    },
    # observed on the parent build: two-level nodes present; texture sets: 0 QUAD, 0 SEPARATE, 2 CONST
    "c_env10x5": {
        "tex_sets": "588775c183e07cb7ee0d4cf2e0b0c21b28cf6d75f1386c3932f21ebdef4d82f2",
        "atlas": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "atlas4": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "env": "eeb59b520e1fb39aea8cff1314aafea3f89b892b83c4ad22ddc8ffb397b66528",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "c3a5dabe936576773242c12a5305c7fa05f754b43c761b5718521e8375453e08",
        "slot_triangles": "99cdb3907a49ff8c7429e19a0d4889b14b51a93a2864d5a1e63fc5e72596146a",
        "depth": "075de2b906dbd7066da008cab735bee896370154603579a50122f9b88545bd45",
        "two_level_nodes": "71fe95d0b18161bd0f8e884070df525e31c4f53cc61ed36ab376cd3be0465738",
        "sah_cost": "ac622ec1a8c6566eccd88fb8a04e25380ef7216f901040cf0572f1c63b54f437",
        "light_table": "10e27f0568d52c9f8825b020718383bce39a2789b26dd0d5b0fb4272a88e68b2",
        "intersect_form0": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
        "intersect_form1": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
    },
    # observed on the parent build: two-level nodes present; texture sets: 0 QUAD, 0 SEPARATE, 2 CONST
    "d_no_env": {
        "tex_sets": "588775c183e07cb7ee0d4cf2e0b0c21b28cf6d75f1386c3932f21ebdef4d82f2",
        "atlas": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "atlas4": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "env": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "c3a5dabe936576773242c12a5305c7fa05f754b43c761b5718521e8375453e08",
        "slot_triangles": "99cdb3907a49ff8c7429e19a0d4889b14b51a93a2864d5a1e63fc5e72596146a",
        "depth": "075de2b906dbd7066da008cab735bee896370154603579a50122f9b88545bd45",
        "two_level_nodes": "71fe95d0b18161bd0f8e884070df525e31c4f53cc61ed36ab376cd3be0465738",
        "sah_cost": "ac622ec1a8c6566eccd88fb8a04e25380ef7216f901040cf0572f1c63b54f437",
        "light_table": "10e27f0568d52c9f8825b020718383bce39a2789b26dd0d5b0fb4272a88e68b2",
        "intersect_form0": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
        "intersect_form1": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
    },
    # observed on the parent build: two-level nodes present; texture sets: 0 QUAD, 0 SEPARATE, 2 CONST
    "e_leaf1": {
        "tex_sets": "588775c183e07cb7ee0d4cf2e0b0c21b28cf6d75f1386c3932f21ebdef4d82f2",
        "atlas": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "atlas4": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "env": "0a48d3b5fa31997bebaccf434f682719381829b3fb7844a7bd1b186ee3a3afed",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "c40368b3222929bb15a87655a5e4de7271302159a24de15dac956e37044baf87",
        "slot_triangles": "a23304a9f46fca86a13ea0199afc8e96d29a22eca88d40e8c89c3b552991f016",
        "depth": "42f4aeb81c1ef81f771f3de8abca9dcf66901c575530e7672e4b1146474ae650",
        "two_level_nodes": "63cac635bc5fd2d4ddffb4ae81b74cb1259f858e74eaee6bc0c4154ea4efd223",
        "sah_cost": "59fdf306f62a7994c544027671632ea076dee210c366bc712ec7d24c970ab8c2",
        "light_table": "2afbbe325910f6b700a3149f1e416da48f6147d271b66ae110b73ecccf95063b",
        "intersect_form0": "9a40928c9c407b13a208330eeba00d639fbbca295d178a3322107506e8f45fb6",
        "intersect_form1": "9a40928c9c407b13a208330eeba00d639fbbca295d178a3322107506e8f45fb6",
    },
    # observed on the parent build: two-level nodes absent; texture sets: 0 QUAD, 0 SEPARATE, 2 CONST
    "f_no_quads": {
        "tex_sets": "588775c183e07cb7ee0d4cf2e0b0c21b28cf6d75f1386c3932f21ebdef4d82f2",
        "atlas": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "atlas4": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
        "env": "0a48d3b5fa31997bebaccf434f682719381829b3fb7844a7bd1b186ee3a3afed",
        "bins": "6e8a7667404f8b9f3ea696ecb592b1b2b166d8cb337c990e995334ee54ec0ce3",
        "hitrec": "c3a5dabe936576773242c12a5305c7fa05f754b43c761b5718521e8375453e08",
        "slot_triangles": "99cdb3907a49ff8c7429e19a0d4889b14b51a93a2864d5a1e63fc5e72596146a",
        "depth": "075de2b906dbd7066da008cab735bee896370154603579a50122f9b88545bd45",
        "two_level_nodes": "374708fff7719dd5979ec875d56cd2286f6d3cf7ec317a3b25632aab28ec37bb",
        "sah_cost": "39f7efc047b00d8aaf6be313f26a9c692cad5ce44bf31a04aba9fb1095e23ff7",
        "light_table": "10e27f0568d52c9f8825b020718383bce39a2789b26dd0d5b0fb4272a88e68b2",
        "intersect_form0": "2cd11ac7a425e854c8553582d65cee8fa056914c88f1f7653a4b4301a3f75137",
    },
}


@pytest.mark.parametrize("name", SCENES)
def test_created_scene_is_byte_identical(name, small_scene):
    lib = L.lib()
    if name == "b_atlas6":
        L.check(lib.fspt_set_texture_interleave_budget(QUAD_IMAGE_BYTES))
    try:
        got, two_level, kinds = digests(arrays_of(name, small_scene))
    finally:
        L.check(lib.fspt_set_texture_interleave_budget(8 << 30))
    print(name, "two-level nodes", two_level, "set kinds", kinds)
    for what, h in got.items():
        print(f'        "{what}": "{h}",')
    # each scene does what its description says
    assert two_level == (name != "f_no_quads")
    if name == "b_atlas6":
        assert kinds == [2, 1, 1]  # fspt_device.hpp: TEXSET_QUAD, TEXSET_SEPARATE, TEXSET_SEPARATE
    assert got == EXPECT[name]
