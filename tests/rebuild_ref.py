"""What fspt_scene_rebuild_geometry must produce: the binned-SAH tree of tests/bvh_binned_ref.py over the new
triangles in the order given, and the scene's per-triangle data permuted by it.  Nothing else."""
import dataclasses

import numpy as np

import bvh_binned_ref as B


def expected(arrays, tri, norm=None):
    """arrays: the scene as it is now (reference layout, leaf order); tri / norm (None: the scene's own records): the
    call's input in that order -> (order uint32, the arrays fspt_scene_create would be handed for the same result)"""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    norm = (arrays.norm if norm is None else np.ascontiguousarray(norm, np.float32)).reshape(-1, 27)
    t = B.build(tri, arrays.leaf_size)
    o = t.order.astype(np.int64)
    fresh = dataclasses.replace(arrays, bvh=t.bvh, tri=np.ascontiguousarray(tri[o]).reshape(-1),
                                norm=np.ascontiguousarray(norm[o]).reshape(-1),
                                uv=np.ascontiguousarray(arrays.uv.reshape(-1, 6)[o]).reshape(-1),
                                mat=np.ascontiguousarray(arrays.mat.reshape(-1, 12)[o]).reshape(-1), depth=t.depth)
    return t.order, fresh
