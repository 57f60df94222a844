"""Scene files and frame sequences: the host steps either side of the path tracer that the reference does in
`PathTracer()` / `start()` / `tick()` (main.js:17-75, 284-445, 838-866, 869-975) when it is pointed at
`scene/<name>.json?frame=N`:

  * read the scene JSON, merge props + static_props + animated_props (main.js:869-871);
  * fetch every asset it names: OBJ texts, the MTL libraries their `mtllib` lines name, texture images
    (prop-level `diffuse` / `metallicRoughness` / `normal` / `emission` strings and MTL `map_*` urls), the RGBE
    environment image (main.js:926-946, obj_loader.js:185-190);
  * build the scene (initBVH) and shoot the auto-focus ray (main.js:903);
  * per frame: render `samples` ticks, tone-map with draw.fs, write the image, go to frame + 1 (main.js:851-866).

Image files are decoded with PIL to straight-alpha RGBA8, row 0 = top - what a browser hands to texImage2D.
Paths in the JSON are relative to the web root (`asset_root`, default: the parent of the scene file's folder)."""
import json
import os

import numpy as np

from . import scene as S


def _read_text(root, rel):
    with open(os.path.join(root, rel), "r", encoding="utf-8", errors="replace") as fh:
        return fh.read()


def _read_image(root, rel):
    from PIL import Image
    with Image.open(os.path.join(root, rel)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))


def mtllib_urls(obj_text, base_path):
    """The urls obj_loader.js:185-187 fetches while parsing: base_path + '/' + the rest of each `mtllib` line."""
    urls = []
    for line in obj_text.split("\n"):
        tok = S._js_split_spaces(line)
        if tok[0] == "mtllib":
            urls.append(base_path + "/" + " ".join(tok[1:]))
    return urls


def load_scene_file(scene_path, asset_root=None, leaf_size=4, bvh="sah", device=0, keep_order=False, geometry_only=False, textures="cpu", keep_mesh=False):
    """Returns (SceneArrays, settings).  settings = camera and display values with the reference's defaults
    (initGlobals, main.js:50-75): eye, dir, fov_scale, env_theta, exposure, samples, focus (lensFeatures[0]
    after shootAutoFocusRay), aperture (index.html default 0.02).  bvh / device: scene.build_scene's builder choice;
    keep_order / geometry_only: as scene.build_scene (the latter: triangles in parse order, no tree); textures: "cpu" or "gpu",
    where the atlas is resampled (scene.build_scene); keep_mesh: as scene.build_scene, and
    meta["obj_texts"] = the props' OBJ texts in merge_scene_props order."""
    with open(scene_path, "r", encoding="utf-8") as fh:
        scene = json.load(fh)
    root = asset_root or os.path.dirname(os.path.dirname(os.path.abspath(scene_path)))
    props = S.merge_scene_props(scene)
    obj_texts, mtl_texts, images = {}, {}, {}

    def want_image(url):
        if url not in images:
            images[url] = _read_image(root, url)

    for p in props:
        if p["path"] not in obj_texts:
            obj_texts[p["path"]] = _read_text(root, p["path"])
        base = "/".join(p["path"].split("/")[:-1])
        for url in mtllib_urls(obj_texts[p["path"]], base):
            if url not in mtl_texts:
                mtl_texts[url] = _read_text(root, url)
            for tex_url in S.parse_materials(mtl_texts[url], base)[1]:
                want_image(tex_url)
        for key in ("diffuse", "metallicRoughness"):
            if isinstance(p.get(key), str):
                want_image(p[key])
        for key in ("normal", "emission"):
            if p.get(key) and isinstance(p[key], str):
                want_image(p[key])
    env, env_w, env_h = None, 0, 0
    e = scene.get("environment")
    if isinstance(e, str):
        img = _read_image(root, e)
        env_h, env_w = img.shape[:2]
        env = img.reshape(-1)
    elif e:
        # array-of-stops skies (main.js:182-204) are broken in the reference itself
        raise ValueError("array-of-stops environments are not supported; use an RGBE image or none")
    eye, d = _camera_ray(scene)
    arrays = S.build_scene_json(scene, obj_texts, mtl_texts, images, env=env, env_w=env_w, env_h=env_h,
                                leaf_size=leaf_size, focus_rays=[(eye, d)], bvh=bvh, device=device, keep_order=keep_order,
                                geometry_only=geometry_only, textures=textures, keep_mesh=keep_mesh)
    if keep_mesh:
        arrays.meta["obj_texts"] = [obj_texts[p["path"]] for p in props]
    return arrays, _settings(scene, arrays.meta["focus"][0])


def _camera_ray(scene):
    return ([float(x) for x in (scene.get("cameraPos") or [0, 0, 2])], [float(x) for x in (scene.get("cameraDir") or [0, 0, -1])])


def _settings(scene, focus):
    eye, d = _camera_ray(scene)
    return dict(eye=eye, dir=d, fov_scale=float(scene.get("fovScale") or 0.5),
                env_theta=float(scene.get("environmentTheta") or 0), exposure=float(scene.get("exposure") or 1.0),
                samples=int(scene.get("samples") or 2000), focus=focus, aperture=0.02)


def render_frame(arrays, settings, width, height, samples=None, bounces=4, seed=1, saturation=1.0, denoise=False,
                 max_sigma=3.0, device=0, lights=None, emitter_fraction=0.5, adaptive=None, sample_map=None, auto_exposure=None,
                 bloom=None, camera=None, light_builder=None):
    """One frame as the reference produces it in frame mode: `samples` ticks from a cleared accumulator
    (main.js:838-857; its very first, discarded tick is not reproduced), then drawQuad.  Returns
    (rgba8 [H, W, 4] top row first - what canvas.toBlob encodes -, radiance [H, W, 4] bottom row first).
    lights="emitters": next-event estimation of emissive triangles (PathTracer.set_lights).  adaptive=REL_MSE:
    adaptive sampling with `samples` as the most ticks a tile gets (PathTracer.render_adaptive); sample_map:
    then also write its ticks per pixel as a grey PNG there (white = `samples`).  auto_exposure: True or a dict of
    PathTracer.set_auto_exposure's parameters: the frame is metered on the GPU and the scene's `exposure`
    becomes a compensation; a still adapts instantly.  bloom: True or a dict of PathTracer.set_bloom's parameters (DESIGN
    8.12): the drawing mixes the HDR pyramid's glow in before the exposure.  camera: None or a dict of
    PathTracer.set_camera_model's arguments (not with adaptive).  light_builder: None, "host" or "gpu" - who
    builds the emitter light table of lights="emitters" (Scene.set_light_builder)."""
    from .tracer import PathTracer
    _light_builder(light_builder, lights)
    auto_exposure = _auto_exposure_params(auto_exposure)
    bloom = _bloom_params(bloom)
    camera = _camera_model_params(camera, adaptive)
    pt = PathTracer(arrays, width, height, device=device, num_bounces=bounces)
    try:
        if camera is not None:
            pt.set_camera_model(**camera)
        if auto_exposure is not None:
            pt.set_auto_exposure(True, **auto_exposure)
        if bloom is not None:
            pt.set_bloom(True, **bloom)
        if light_builder is not None:
            pt.scene.set_light_builder(light_builder)
        rgba, rad = _render_on(pt, settings, samples, seed, saturation, denoise, max_sigma, lights, emitter_fraction, adaptive,
                               sample_map)
    finally:
        pt.close()
        pt.scene.close()
    return rgba[::-1].copy(), rad


SEQUENCE_ADAPT = 0.25  # render_sequence's auto-exposure step per frame, in log2 (1 = instant): within 10 % of a new light in 8 frames


def _light_builder(light_builder, lights):
    """refuses a light_builder the library would refuse, or one without the lights it builds the table of"""
    from .tracer import LIGHT_BUILDERS
    if light_builder is None:
        return
    if light_builder not in LIGHT_BUILDERS:
        raise ValueError("light_builder must be one of %s, got %r" % (sorted(LIGHT_BUILDERS), light_builder))
    if lights != "emitters":
        raise ValueError('light_builder needs lights="emitters"')


def _auto_exposure_params(auto_exposure, adapt=None):
    """None (off) or PathTracer.set_auto_exposure's keyword arguments from True / a dict, refused here if the library would;
    adapt: the adapt_up / adapt_down a dict that names neither gets."""
    if auto_exposure is None or auto_exposure is False:
        return None
    from .tracer import _exposure_params
    params = {} if auto_exposure is True else dict(auto_exposure)
    if adapt is not None and "adapt_up" not in params and "adapt_down" not in params:
        params.update(adapt_up=adapt, adapt_down=adapt)
    _exposure_params(params)
    return params


def _camera_model_params(camera, adaptive=None, temporal=None):
    """None (pinhole) or PathTracer.set_camera_model's keyword arguments, refused here if the library would (but for the
    target's height, which it checks)"""
    if camera is None:
        return None
    from .tracer import camera_model_params
    camera = dict(camera)
    if set(camera) - {"model", "angle", "ipd"}:
        raise TypeError(f"unknown camera parameters {sorted(set(camera) - {'model', 'angle', 'ipd'})}")
    if camera_model_params(**camera).model == 0:
        return None
    if adaptive is not None or temporal is not None:
        raise ValueError("a camera model other than pinhole cannot be combined with adaptive sampling or temporal accumulation")
    return camera


def _bloom_params(bloom):
    """None (off) or PathTracer.set_bloom's keyword arguments from True / a dict, refused here if the library would"""
    if bloom is None or bloom is False:
        return None
    from .tracer import _bloom_params as check
    params = {} if bloom is True else dict(bloom)
    check(params)
    return params


def _render_on(pt, settings, samples, seed, saturation, denoise, max_sigma, lights, emitter_fraction, adaptive, sample_map, draw=True):
    """render_frame's work on an existing tracer, from a cleared accumulator (bottom row first); draw=False: no picture
    (None comes back in its place; a draw under auto-exposure would adapt the exposure once more)"""
    pt.clear()
    pt.eye, pt.dir = list(settings["eye"]), list(settings["dir"])
    pt.fovScale, pt.envTheta = settings["fov_scale"], settings["env_theta"]
    pt.lensFeatures = [settings["focus"], settings["aperture"]]
    if lights is not None:
        pt.set_lights(lights, emitter_fraction)
    pt.seed(seed)
    n = int(samples if samples is not None else settings["samples"])
    if adaptive is None:
        pt.render(n)
    else:
        pt.render_adaptive(adaptive, max_ticks=n)
        if sample_map:
            write_sample_map(sample_map, pt.sample_counts(), n)
    rgba = pt.draw(settings["exposure"], saturation, denoise, max_sigma) if draw else None
    rad = pt.readRadiance()
    return rgba, rad


def is_jpeg_path(path):
    return str(path).lower().endswith((".jpg", ".jpeg"))


def is_exr_path(path):
    return str(path).lower().endswith(".exr")


EXR_KEYS = ("compression", "float32", "layers", "chunk_bytes")


def exr_settings(exr):
    """None or a dict of tracer.exr_encode's compression / float32 / layers / chunk_bytes, checked: (the dict, its layer bits)"""
    from .tracer import exr_params
    exr = {} if exr is None else dict(exr)
    if set(exr) - set(EXR_KEYS):
        raise TypeError(f"unknown exr parameters {sorted(set(exr) - set(EXR_KEYS))}")
    return exr, int(exr_params(**exr).layers)


def write_image(path, rgba, jpeg=None, device=0, png=None, exr=None, features=None):
    """An RGBA8 frame [H, W, 4], row 0 = top, as the picture `path` names: .jpg / .jpeg = a baseline JPEG encoded on the GPU
    (tracer.jpeg_encode; jpeg = None or a dict of its quality / subsampling / restart_mcus), anything else
    through Pillow as before - unless png is "gpu" or a dict of tracer.png_encode's channels / filter / chunk_bytes: then the
    PNG is filtered and deflated on the GPU.  .exr = a scene-linear OpenEXR file made on the GPU
    (tracer.exr_encode): `rgba` is then the float32 radiance [H, W, 4], row 0 = top, exr = None or a dict of its
    compression / float32 / layers / chunk_bytes, features = the float32 guides [H, W, 8] its albedo, normal and depth
    layers need."""
    if is_exr_path(path):
        from .tracer import exr_encode
        if getattr(rgba, "dtype", None) != np.float32:
            raise ValueError("write_image: an .exr takes the float32 radiance, not a drawn frame")
        data = exr_encode(rgba, features, device=device, **exr_settings(exr)[0])
        with open(path, "wb") as f:
            f.write(data)
        return
    if is_jpeg_path(path):
        from .tracer import jpeg_encode
        data = jpeg_encode(rgba, device=device, **(jpeg or {}))
        with open(path, "wb") as f:
            f.write(data)
        return
    if png is not None:
        if png != "gpu" and not isinstance(png, dict):
            raise ValueError(f'write_image: png must be None, "gpu" or a dict of png_encode\'s parameters, not {png!r}')
        from .tracer import png_encode
        data = png_encode(rgba, device=device, **({} if png == "gpu" else png))
        with open(path, "wb") as f:
            f.write(data)
        return
    from PIL import Image
    Image.fromarray(rgba[:, :, :3]).save(path)


def write_sample_map(path, counts, max_ticks):
    """Ticks per pixel (PathTracer.sample_counts(), rows bottom-up) as an 8-bit grey PNG, top row first: 255 = max_ticks."""
    import numpy as np
    from PIL import Image
    grey = np.round(counts[::-1].astype(np.float64) * (255.0 / max(int(max_ticks), 1))).clip(0, 255).astype(np.uint8)
    Image.fromarray(grey, mode="L").save(path)


APPEARANCE_FIELDS = ("mat", "uv", "atlas", "env", "bins")


def held_appearance(a):
    """What a scene created from SceneArrays `a` holds of its appearance: mat / uv in a's own (leaf) order, the atlas with
    its shape, the environment with its size, the bins - the record sequence_frame_changes compares later frames with."""
    return dict(n_tris=int(a.n_tris), mat=np.array(a.mat, np.float32).reshape(-1, 12), uv=np.array(a.uv, np.float32).reshape(-1, 6),
                atlas=(int(a.atlas_res), int(a.atlas_layers), None if a.atlas is None else np.array(a.atlas)),
                env=(0, 0, None) if a.env is None else (int(a.env_w), int(a.env_h), np.array(a.env)),
                bins=np.array(a.bins, np.uint32).reshape(-1))


def sequence_frame_changes(held, g, order):
    """render_sequence(bvh="refit")'s classification of a frame, as a pure function.  `held` = held_appearance of what the
    live scene holds now, `g` = the frame's arrays in parse order, `order` = the base tree's leaf order (parse index per leaf
    position).  None: another triangle count - the frame builds a new scene.  Else a dict with the fields of
    APPEARANCE_FIELDS that differ from `held`, each in `held`'s form (mat / uv in the base's leaf order): empty = a plain
    refit, anything else = an "appearance" frame that uploads exactly those."""
    if int(g.n_tris) != held["n_tris"]:
        return None
    order = np.asarray(order)
    new = held_appearance(g)
    new["mat"], new["uv"] = new["mat"][order], new["uv"][order]

    def same(x, y):
        if isinstance(x, tuple):
            return x[:2] == y[:2] and same(x[2], y[2])
        return (x is None and y is None) or (x is not None and y is not None and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)))

    return {k: new[k] for k in APPEARANCE_FIELDS if not same(held[k], new[k])}


POSE_KEYS = ("rotate", "scale", "translate")  # of a prop: what obj_loader.js:19-38 applies to a fixed mesh


def sequence_pose_frame(base_scene, frame_scene):
    """render_sequence(bvh="refit", pose=True)'s classification of a frame, as a pure function of two scene JSONs (dicts): True
    when the frame is the base frame with its props moved rigidly - the two are equal once every prop's rotate / scale /
    translate and the scenes' worldTransforms are removed - and neither has a `normalize` (which rescales by the bounds of
    the moved scene).  Such a frame is fully described by sequence_pose_matrices; its OBJs need not be parsed."""
    def stripped(scene):
        out = {k: v for k, v in scene.items() if k not in ("worldTransforms", "props", "static_props", "animated_props")}
        out["props"] = [{k: v for k, v in p.items() if k not in POSE_KEYS} for p in S.merge_scene_props(scene)]
        return out

    if base_scene.get("normalize") or frame_scene.get("normalize"):
        return False
    return stripped(base_scene) == stripped(frame_scene)


def sequence_pose_matrices(base_scene, frame_scene):
    """float32 [n_props, 12]: per prop (merge_scene_props order) the matrix that takes the BASE frame's triangles to this
    frame's, float32(prop_matrix(frame) @ inverse(prop_matrix(base))) - what Scene.update_transforms is handed when the
    rest mesh is the base frame's."""
    def m4(prop, world):
        m = np.eye(4, dtype=np.float64)
        m[:3] = S.prop_matrix(prop, world)
        return m

    pb, pf = S.merge_scene_props(base_scene), S.merge_scene_props(frame_scene)
    out = [(m4(f, frame_scene.get("worldTransforms")) @ np.linalg.inv(m4(b, base_scene.get("worldTransforms"))))[:3] for b, f in zip(pb, pf)]
    return np.asarray(out, np.float64).reshape(-1, 12).astype(np.float32)


def _obj_split(text):
    """(the OBJ's lines that are not `v` lines, its `v` lines' three numbers as float64 [n, 3]) - obj_loader.js:162-168's split"""
    rest, v = [], []
    for line in text.split("\n"):
        tok = S._js_split_spaces(line)
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:4]])
        else:
            rest.append(line)
    return rest, np.asarray(v, np.float64).reshape(-1, 3)


def sequence_mesh_frame(base_scene, base_objs, frame_scene, frame_objs):
    """render_sequence(bvh="refit", mesh=True)'s classification of a frame, as a pure function of two scene JSONs (dicts) and
    their props' OBJ texts (merge_scene_props order): True when the frame is the base frame with other vertex positions - the
    scenes are equal once every prop's `path` is removed, neither has a `normalize`, and prop by prop the OBJs have the same
    number of `v` lines and are equal in every other line.  Such a frame is fully described by sequence_mesh_positions."""
    def stripped(scene):
        out = {k: v for k, v in scene.items() if k not in ("props", "static_props", "animated_props")}
        out["props"] = [{k: v for k, v in p.items() if k != "path"} for p in S.merge_scene_props(scene)]
        return out

    if base_scene.get("normalize") or frame_scene.get("normalize") or len(base_objs) != len(frame_objs):
        return False
    if stripped(base_scene) != stripped(frame_scene):
        return False
    for a, b in zip(base_objs, frame_objs):
        if a is b or a == b:
            continue
        (ra, va), (rb, vb) = _obj_split(a), _obj_split(b)
        if ra != rb or va.shape != vb.shape:
            return False
    return True


def sequence_mesh_positions(scene, obj_texts):
    """float32 [n_vertices, 3]: every prop's `v` lines (merge_scene_props order, one OBJ after the other: the indices of
    meta["tri_vertex"]) as world positions, float32(prop_matrix(prop) applied in float64) - what Scene.update_vertices is handed.
    (The parse path applies the prop's steps one by one; the composed matrix can differ from it in the last bit.)"""
    out = []
    for prop, text in zip(S.merge_scene_props(scene), obj_texts):
        m = S.prop_matrix(prop, scene.get("worldTransforms"))
        v = _obj_split(text)[1]
        out.append(v @ m[:, :3].T + m[:, 3])
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3), np.float32)


def _parse_order_parts(base):
    """part id per PARSE-order triangle from a base built with keep_order (the inverse of meta["tri_part"]'s gather)"""
    out = np.zeros(base.n_tris, np.uint32)
    out[np.asarray(base.meta["tri_order"], np.int64)] = base.meta["tri_part"]
    return out


def arrays_with_sky(arrays, sun_dir, width=1024, height=512, device=0, **params):
    """`arrays` under a generated sky instead of its environment: scene.sky's bytes and the GPU's bins of them -
    what Scene.update_sky makes of a live scene, for a scene that is yet to be created"""
    import dataclasses
    rgbe, w, h = S.sky(sun_dir, width, height, device=device, **params)
    return dataclasses.replace(arrays, env=rgbe, env_w=w, env_h=h, bins=S.env_bins(rgbe, w, h, device=device))


def _sequence_sky(sky, k, n):
    """frame n's sky (the k-th frame of the sequence): `sky` is a list of parameter dicts, one per frame, or a callable of the
    frame number; a dict holds Scene.update_sky's arguments (sun_dir, width, height and the model's parameters)"""
    d = sky(n) if callable(sky) else sky[k]
    if not isinstance(d, dict) or "sun_dir" not in d:
        raise ValueError(f"render_sequence: the sky of frame {n} must be a dict with a sun_dir, got {d!r}")
    return dict(d)


def render_sequence(scene_pattern, frames, out_pattern, width, height, asset_root=None, bvh="sah", rebuild_above=None,
                    on_frame=None, temporal=None, variance=False, auto_exposure=None, bloom=None, pose=False, camera=None, sky=None, textures="cpu", jpeg=None, png=None, exr=None, mesh=False, matte_samples=8, **kw):
    """frame=N sequencing (main.js:851-866, 966-969): for every N in `frames` load `scene_pattern.format(frame=N)`
    (the per-frame scene JSON the reference's server hands out for `?frame=N`), render it, write
    `out_pattern.format(frame=N)` (the reference POSTs the canvas PNG to /upload/<scene>/<N>), go on to N + 1.
    bvh="gpu" builds every frame's tree on the render device.
    bvh="refit" (DESIGN 8.6): the first frame builds ("sah"); a later frame with the same triangle count keeps scene and
    tracer: its props are parsed without building a tree, the moved triangles go to
    Scene.update_geometry in the first tree's leaf order, the accumulator is cleared and the auto-focus ray is shot
    against the new triangles.  A refitted frame whose Scene.sah_cost() exceeds `rebuild_above` x the cost at the last
    (re)build gets a new tree IN PLACE (Scene.rebuild_geometry, DESIGN 8.7: scene and tracer stay; the tree is the binned
    SAH of bvh="gpu" from then on, which renders 0.94-0.95x as fast as the sweep's); None, the default: never.  A kept frame
    whose materials, uvs, atlas, environment or bins differ from what the live scene holds gets exactly those updated in place
    after its refit (Scene.update_materials / update_environment) and reports "appearance".  A frame with another
    triangle count builds a new scene.
    pose=True (bvh="refit" only): the scene also keeps its triangles as the rest mesh of a pose, one part per
    prop (Scene.set_pose).  A frame that sequence_pose_frame finds to be the rest frame with its props moved rigidly parses
    NO OBJ: its sequence_pose_matrices go to Scene.update_transforms, a kernel poses the triangles and the tree is refitted;
    its auto-focus ray is shot through Scene.intersect on the live scene; it reports "pose".  Any other frame takes the path
    above, and the pose is re-set from what that frame uploaded.  The pictures are NOT bit-equal to the parse path's: there
    the transform is applied in float64 to the OBJ's vertices and rounded once, here a float32 matrix is applied in float32
    to the rest frame's float32 triangles - which is why it is opt-in.
    mesh=True (bvh="refit" only): the scene also keeps its triangles as an indexed mesh (Scene.set_mesh from the
    build's meta).  A frame that sequence_mesh_frame finds to be the build frame with other `v` lines - and whose static
    triangles (no vt, or `normals: "mesh"`) did not move - builds nothing: its OBJs are still read and split line by line in
    Python (to compare the other lines and collect the `v` ones), and its sequence_mesh_positions go to
    Scene.update_vertices, kernels derive the normal frames and the tree is refitted; it reports "mesh".  Any other frame takes
    the path above, and the mesh path then rests until the next frame that builds.  Like pose, NOT bit-equal to the parse
    path: there normals come from the float64 positions, here from their float32 roundings, and the auto-focus ray is shot
    through Scene.intersect in float32 where the parse path asks the builder in float64.
    on_frame(N, "build" | "refit" | "rebuild" | "appearance" | "pose" | "mesh" | "sky") reports what a frame did.
    temporal (bvh="refit" only): True or a dict of PathTracer.temporal_accumulate's parameters, plus "atrous": K
    for K a-trous iterations on the result.  Every frame then follows the protocol motion_begin, update_geometry, clear and
    render, temporal_accumulate, and the picture written is temporal_draw of the result (`denoise`, the firefly filter of
    draw(), does not apply to it; `adaptive` is refused); frame k renders with seed + k, so that the frames' noise is
    independent.  A frame that builds a new scene starts a new history.  "clamp": True or a dict of
    PathTracer.temporal_set_clamp's fast_history / sigma_scale: every tracer gets temporal_set_clamp() before
    its first frame, and every frame's history is clamped into its fast history's box.
    variance (with temporal and "atrous" >= 1): the a-trous iterations are the variance-guided ones - every tracer
    gets temporal_set_moments(), a frame's features() come before its temporal_accumulate (which demodulates by them) and the
    filter is temporal_denoise(iterations=K, variance=True).
    auto_exposure: True or a dict of PathTracer.set_auto_exposure's parameters; every tracer gets
    set_auto_exposure() before its first frame, each frame's one drawing meters what it draws (the accumulator, or under
    temporal the history or its filtered form) and the scene's `exposure` becomes a compensation.  With bvh="refit" the
    tracer lives across the frames and the exposure ADAPTS: adapt_up = adapt_down = SEQUENCE_ADAPT per frame unless the
    dict names one; every other bvh builds a tracer per frame, which meters instantly.  A new scene starts from a first metering.
    bloom: True or a dict of PathTracer.set_bloom's parameters; every tracer gets set_bloom() before its first
    frame, and each frame's one drawing blooms what it draws.
    camera: None or a dict of PathTracer.set_camera_model's arguments; every tracer gets set_camera_model()
    before its first frame (not with temporal or adaptive).
    sky: None, a list of dicts (one per frame) or a callable of the frame number that returns one: Scene.update_sky's
    arguments (sun_dir, width, height, the model's parameters).  Every frame's environment is then that generated sky, whatever
    the scene file names.  With bvh="refit" the kept tracer's scene gets update_sky once per frame - nothing but the light is
    made again, on the GPU - and a kept frame reports "sky"; every other bvh builds each frame's scene under arrays_with_sky.
    textures: "cpu" or "gpu" - where every frame's atlas is resampled.  With "gpu" and bvh="refit" a kept frame
    whose atlas changed sends its decoded images, not the atlas: Scene.update_textures packs them on the device.
    jpeg: an out_pattern that ends in .jpg / .jpeg is written as a JPEG encoded on the GPU (write_image); None
    or a dict of jpeg_encode's quality / subsampling / restart_mcus.
    png: None = every other out_pattern goes through Pillow; "gpu" or a dict of png_encode's channels / filter /
    chunk_bytes = it is written as a PNG encoded on the GPU (write_image).
    exr: an out_pattern that ends in .exr is written as a scene-linear OpenEXR file of the frame's radiance -
    under bvh="refit" by PathTracer.draw_exr (the accumulator, or the temporal result), so that only the file leaves the
    device; None or a dict of its compression / float32 / layers / chunk_bytes.  The albedo, normal and depth layers need
    bvh="refit" (the live tracer's features), and so do "crypto_object" and "crypto_material" (DESIGN 8.25): the ids are set
    once, when the scene is built (Scene.set_default_mattes: the props, and the first frame's materials), follow the
    triangles through every update and rebuild, and each frame's file carries a mattes() pass of matte_samples rays per pixel.
    light_builder (in kw, with lights="emitters"): "gpu" = every scene's emitter light table is built on the
    device (Scene.set_light_builder), so that a kept frame's update reads 8 bytes back for it."""
    as_exr = is_exr_path(out_pattern)
    exr, exr_layers = exr_settings(exr)
    if as_exr and bvh != "refit" and exr_layers & (14 | 48):
        raise ValueError('render_sequence: the albedo, normal, depth and matte layers of an .exr need bvh="refit"')
    if textures not in S.TEXTURE_PACKERS:
        raise ValueError(f"render_sequence: textures must be one of {S.TEXTURE_PACKERS}, not {textures!r}")
    camera = _camera_model_params(camera, kw.get("adaptive"), None if temporal is None or temporal is False else temporal)
    auto_exposure = _auto_exposure_params(auto_exposure, SEQUENCE_ADAPT if bvh == "refit" else None)
    bloom = _bloom_params(bloom)
    written = []
    device = kw.get("device", 0)
    if temporal is not None and temporal is not False:
        if bvh != "refit":
            raise ValueError('render_sequence: temporal needs bvh="refit" (one scene and tracer across the frames)')
        temporal = {} if temporal is True else dict(temporal)
        atrous = int(temporal.pop("atrous", 0))
        clamp = temporal.pop("clamp", None)
        if clamp is not None and clamp is not False:
            from .tracer import _clamp_params
            clamp = {} if clamp is True else dict(clamp)
            if set(clamp) - {"fast_history", "sigma_scale"}:
                raise TypeError(f"unknown clamp parameters {sorted(set(clamp) - {'fast_history', 'sigma_scale'})}")
            _clamp_params(**clamp)
        else:
            clamp = None
        from .tracer import _temporal_params
        _temporal_params(temporal)  # (refuse bad parameters before the first frame renders)
        if kw.get("adaptive") is not None:
            # (tiles retire at different tick counts, the blend weighs every pixel with one n = the accumulator's ticks)
            raise ValueError("render_sequence: temporal cannot be combined with adaptive sampling")
    else:
        temporal = None
    if pose and bvh != "refit":
        raise ValueError('render_sequence: pose needs bvh="refit" (one scene across the frames)')
    if mesh and bvh != "refit":
        raise ValueError('render_sequence: mesh needs bvh="refit" (one scene across the frames)')
    if variance and (temporal is None or atrous < 1):
        raise ValueError('render_sequence: variance needs temporal with "atrous" >= 1 (the variance guides the a-trous filter)')

    def save(n, rgba, data=None):
        out = out_pattern.format(frame=n)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        if data is not None:  # a file made on the device
            with open(out, "wb") as f:
                f.write(data)
        else:
            write_image(out, rgba, jpeg, device, png, exr)
        written.append(out)

    if bvh != "refit":
        for n in frames:
            arrays, settings = load_scene_file(scene_pattern.format(frame=n), asset_root, bvh=bvh, device=device, textures=textures)
            if sky is not None:
                arrays = arrays_with_sky(arrays, device=device, **_sequence_sky(sky, len(written), n))
            rgba, rad = render_frame(arrays, settings, width, height, auto_exposure=auto_exposure, bloom=bloom, camera=camera, **kw)
            if on_frame:
                on_frame(n, "build")
            save(n, np.ascontiguousarray(rad[::-1]) if as_exr else rgba)
        return written

    from .tracer import PathTracer
    opt = dict(samples=None, seed=1, saturation=1.0, denoise=False, max_sigma=3.0, lights=None, emitter_fraction=0.5,
               adaptive=None, sample_map=None)
    bounces = kw.get("bounces", 4)
    opt.update({k: v for k, v in kw.items() if k in opt})
    light_builder = kw.get("light_builder")  #  every scene built here gets it before its first frame
    _light_builder(light_builder, opt["lights"])
    base, pt, cost0, leaf_order = None, None, None, None

    atlas_sent = False
    held = None  # the appearance the live scene holds now (not the base's: a change that persists is uploaded once)
    rest_json = None  # pose=True: the scene JSON of the frame whose triangles are the live scene's rest mesh
    mesh_json, mesh_rest = None, None  # mesh=True: the scene JSON and positions of the frame that built the live scene, while the mesh path is open

    def read_json(p):
        with open(p, "r", encoding="utf-8") as fh:
            return json.load(fh)

    try:
        for n in frames:
            path = scene_pattern.format(frame=n)
            how = "build"
            frame_json = read_json(path) if pose or mesh else None
            mesh_pos = None
            if base is not None and mesh_json is not None:
                root = asset_root or os.path.dirname(os.path.dirname(os.path.abspath(path)))
                texts, frame_objs = {}, []
                for p in S.merge_scene_props(frame_json):
                    if p["path"] not in texts:
                        texts[p["path"]] = _read_text(root, p["path"])
                    frame_objs.append(texts[p["path"]])
                if sequence_mesh_frame(mesh_json, base.meta["obj_texts"], frame_json, frame_objs):
                    mesh_pos = sequence_mesh_positions(frame_json, frame_objs)
                    still = np.unique(base.meta["tri_vertex"][base.meta["tri_static"]])
                    if mesh_pos.shape != mesh_rest.shape or not np.array_equal(mesh_pos[still], mesh_rest[still]):
                        mesh_pos = None  # (a static triangle moved: the parse path)
            if mesh_pos is not None:
                if temporal is not None:
                    pt.scene.motion_begin()
                pt.update_vertices(mesh_pos)
                eye, d = _camera_ray(frame_json)
                t, hit, _, _ = pt.scene.intersect(np.float32([eye + d]))
                dist = float(t[0]) if hit[0] >= 0 else 1e6  # shootAutoFocusRay's maxT (main.js:447-546)
                settings = _settings(frame_json, 1 - 1 / dist)
                how = "mesh"
            elif base is not None and rest_json is not None and sequence_pose_frame(rest_json, frame_json):
                if temporal is not None:
                    pt.scene.motion_begin()
                pt.update_transforms(sequence_pose_matrices(rest_json, frame_json))
                eye, d = _camera_ray(frame_json)
                t, hit, _, _ = pt.scene.intersect(np.float32([eye + d]))
                dist = float(t[0]) if hit[0] >= 0 else 1e6  # shootAutoFocusRay's maxT (main.js:447-546)
                settings = _settings(frame_json, 1 - 1 / dist)
                how = "pose"
            elif base is not None:
                g, settings = load_scene_file(path, asset_root, geometry_only=True, device=device, textures=textures)
                changes = sequence_frame_changes(held, g, base.meta["tri_order"])
                mesh_json = None  # (what the scene holds is no longer the build frame's mesh with other positions)
                if changes is not None:
                    tri, norm = S.geometry_in_leaf_order(leaf_order, g.tri, g.norm)
                    if temporal is not None:
                        pt.scene.motion_begin()
                    pt.update_geometry(tri, norm)
                    how = "refit"
                    if rebuild_above is not None and pt.scene.sah_cost() > rebuild_above * cost0:
                        leaf_order = S.compose_order(leaf_order, pt.rebuild_geometry(tri, norm))
                        cost0 = pt.scene.sah_cost()
                        how = "rebuild"
                    if pose:  # what this frame uploaded is the rest mesh from here on, in the current leaf order
                        rest_json = None if frame_json.get("normalize") else frame_json
                        if rest_json is not None:
                            part = _parse_order_parts(base)[np.asarray(leaf_order, np.int64)]
                            pt.scene.set_pose(part, *S.geometry_in_leaf_order(leaf_order, g.tri, g.norm), n_parts=len(S.merge_scene_props(frame_json)))
                    if sky is not None:  # (the scene file's environment is not this sequence's light)
                        changes = {k: v for k, v in changes.items() if k not in ("env", "bins")}
                    if changes:
                        #  what differs goes to the live scene in place: tracer, history and exposure stay
                        if {"mat", "uv", "atlas"} & set(changes):
                            # the atlas goes along when it changed - and once at the scene's first update, which retains it
                            res, layers, atlas = changes["atlas"] if "atlas" in changes else (None, None, None) if atlas_sent else held["atlas"]
                            atlas_sent = True
                            cur = np.asarray(leaf_order)  # mat / uv go in the CURRENT leaf order (a rebuild composed it)
                            if textures == "gpu" and atlas is not None:  #  the sources go, the device packs them
                                pt.update_textures(g.mat.reshape(-1, 12)[cur], g.uv.reshape(-1, 6)[cur] if "uv" in changes else None, g.meta["packer"])
                            else:
                                pt.update_materials(g.mat.reshape(-1, 12)[cur], g.uv.reshape(-1, 6)[cur] if "uv" in changes else None,
                                                    atlas, res, layers)
                        if {"env", "bins"} & set(changes):
                            pt.update_environment(g.env, g.env_w, g.env_h, g.bins)
                        held.update(changes)
                        how = "appearance"
            if how == "build":
                if pt is not None:
                    pt.close(); pt.scene.close()
                base, settings = load_scene_file(path, asset_root, bvh="sah", device=device, keep_order=True, textures=textures, keep_mesh=mesh)
                pt = PathTracer(base, width, height, device=device, num_bounces=bounces)
                cost0 = pt.scene.sah_cost() if rebuild_above is not None else None
                leaf_order = base.meta["tri_order"]
                held, atlas_sent = held_appearance(base), False
                rest_json = None
                mesh_json = None
                if mesh and not frame_json.get("normalize"):
                    pt.scene.set_mesh()
                    mesh_json, mesh_rest = frame_json, sequence_mesh_positions(frame_json, base.meta["obj_texts"])
                if camera is not None:
                    pt.set_camera_model(**camera)
                if as_exr and exr_layers & 48:
                    pt.scene.set_default_mattes()
                if light_builder is not None:
                    pt.scene.set_light_builder(light_builder)
                if pose and not frame_json.get("normalize"):
                    pt.scene.set_pose(base.meta["tri_part"], n_parts=len(S.merge_scene_props(frame_json)))
                    rest_json = frame_json
                if variance:
                    pt.temporal_set_moments(True)
                if temporal is not None and clamp is not None:
                    pt.temporal_set_clamp(True, **clamp)
                if auto_exposure is not None:
                    pt.set_auto_exposure(True, **auto_exposure)
                if bloom is not None:
                    pt.set_bloom(True, **bloom)
            if sky is not None:
                pt.update_sky(**_sequence_sky(sky, len(written), n))
                how = "sky" if how != "build" else how
            if temporal is None:
                rgba, _ = _render_on(pt, settings, **opt, draw=not as_exr)
            else:
                _render_on(pt, settings, **{**opt, "seed": opt["seed"] + len(written), "denoise": False},
                           draw=auto_exposure is None)  # (its draw is not the frame; under auto-exposure it would adapt twice a frame)
                if variance:
                    pt.features(8, opt["seed"])
                pt.temporal_accumulate(read=False, **temporal)
                if variance:
                    pt.temporal_denoise(iterations=atrous, variance=True)
                elif atrous > 0:
                    pt.features(8, opt["seed"])
                    pt.temporal_denoise(iterations=atrous)
                if not as_exr:
                    rgba = pt.temporal_draw(settings["exposure"], opt["saturation"], denoised=atrous > 0)
            if on_frame:
                on_frame(n, how)
            if as_exr:
                if exr_layers & 14 and not (temporal is not None and (variance or atrous > 0)):
                    pt.features(8, opt["seed"])
                if exr_layers & 48:
                    pt.mattes(matte_samples, opt["seed"])
                save(n, None, pt.draw_exr("accumulator" if temporal is None else "temporal_denoised" if atrous > 0 else "temporal", **exr))
            else:
                save(n, rgba[::-1].copy())
    finally:
        if pt is not None:
            pt.close(); pt.scene.close()
    return written
