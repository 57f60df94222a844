#!/usr/bin/env python3
"""tools/texpack_bench.py - the texture packer on the GPU against the numpy packer.

    python tools/texpack_bench.py --reps 3 [--source-res 1024] [--atlas-res 2048]

One JSON line.  The atlas is bench.py's image-mapped scene's: its 7 image layers resampled to --atlas-res^2 from procedural
--source-res^2 sources, plus its flat-colour layers.  Medians of --reps with the per-rep values, everything timed in one
process, interleaved rep by rep, wall clock around the blocking calls:
  cpu_get_pixels_s        TexturePacker.get_pixels(): scene.resample_image per image layer, in numpy
  gpu_get_pixels_s        TexturePacker.get_pixels(device=0) = fspt_atlas_pack_gpu, and its split as the library took it:
                          upload_ms (sources and records, host clock), kernel_ms (k_tex_resample, HIP events), readback_ms (the
                          atlas, host clock)
  update_materials_s      Scene.update_materials(mat, uv, atlas, ...) carrying the CPU-resampled atlas (not counting its resample)
  update_textures_s       Scene.update_textures(mat, uv, packer): the sources go, the device resamples
  patch_textures_s        Scene.patch_textures([l], ...): one image layer replaced from its source
and for the three scene calls Scene.last_appearance(): kernel ms first to last, launches, bytes uploaded, bytes retained.
The two atlases are compared: bytes that differ, and the largest difference in codes (the sRGB-corrected layers decode
through the committed table on the GPU, through numpy's float32 pow on the CPU)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--source-res", type=int, default=1024)
    ap.add_argument("--atlas-res", type=int, default=2048)
    ap.add_argument("--mesh-n", type=int, default=76)
    args = ap.parse_args(argv)
    import __graft_entry__ as g
    g.build()
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S

    reps = max(args.reps, 1)
    texts = {"synthetic/cube_sphere.obj": S.cube_sphere_obj(args.mesh_n), "synthetic/quad.obj": S.QUAD_OBJ}
    env, w, h = S.synthetic_env(256, 128)
    arrays = S.build_scene(S.bunny_props_textured(), texts, env=env, env_w=w, env_h=h, images=S.procedural_maps(args.source_res),
                           atlas_res=args.atlas_res)
    packer = arrays.meta["packer"]
    # the reference's packer shrinks the atlas to its tallest source; the bench asks for the magnified atlas
    packer.max_res = max(packer.max_res, args.atlas_res)
    packer.res = args.atlas_res
    desc = packer.pack_desc()
    image_layers = [l for l, y in enumerate(desc["layers"]) if y["kind"] == "image"]
    src_bytes = sum(int(im.size) for im in desc["images"])

    live = Scene(arrays)
    pt = PathTracer(live, 640, 360, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.prepare()
    keys = ("cpu_get_pixels_s", "gpu_get_pixels_s", "update_materials_s", "update_textures_s", "patch_textures_s")
    out = {k: [] for k in keys}
    split = {k: [] for k in ("upload_ms", "kernel_ms", "readback_ms")}
    last = {k: [] for k in ("update_materials", "update_textures", "patch_textures")}
    packer.get_pixels(device=0)  # (the first call loads the code object)
    cpu_atlas = gpu_atlas = None
    for r in range(reps):
        t, cpu_atlas = timed(packer.get_pixels)
        out["cpu_get_pixels_s"].append(t)
        t, gpu_atlas = timed(lambda: packer.get_pixels(device=0))
        out["gpu_get_pixels_s"].append(t)
        for k, v in S.atlas_pack_last_ms().items():
            split[k].append(v)
        t, _ = timed(lambda: live.update_materials(arrays.mat, arrays.uv, cpu_atlas, desc["res"], len(desc["layers"])))
        out["update_materials_s"].append(t); last["update_materials"].append(live.last_appearance())
        t, _ = timed(lambda: live.update_textures(arrays.mat, arrays.uv, desc))
        out["update_textures_s"].append(t); last["update_textures"].append(live.last_appearance())
        l = image_layers[r % len(image_layers)]
        y = dict(desc["layers"][l], image=0)
        t, _ = timed(lambda: live.patch_textures([l], [y], [desc["images"][desc["layers"][l]["image"]]]))
        out["patch_textures_s"].append(t); last["patch_textures"].append(live.last_appearance())
    pt.close(); live.close()
    diff = np.abs(cpu_atlas.astype(np.int16) - gpu_atlas.astype(np.int16))
    res = {"tool": "texpack_bench", "reps": reps, "atlas": f"{desc['res']}^2 x {len(desc['layers'])}", "image_layers": len(image_layers),
           "sources": f"{len(desc['images'])} x {args.source_res}^2", "source_bytes": src_bytes, "atlas_bytes": int(cpu_atlas.size),
           "n_tris": int(arrays.n_tris)}
    res.update({k: float(np.median(v)) for k, v in out.items()})
    res.update({"gpu_" + k: float(np.median(v)) for k, v in split.items()})
    res["per_rep"] = {k: [round(x, 6) for x in v] for k, v in {**out, **split}.items()}
    for k, v in last.items():
        res[k] = dict(kernel_ms=float(np.median([x["ms"] for x in v])), launches=v[-1]["launches"], uploaded=v[-1]["uploaded"], retained=v[-1]["retained"])
    res["cpu_vs_gpu_atlas"] = dict(bytes_differ=int((diff > 0).sum()), max_codes=int(diff.max()), fraction=float((diff > 0).mean()))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
