"""Render to PNG without a browser: the synthetic BASELINE scene, or a scene JSON / a frame sequence of the
reference's format (scene/<name>.json with props / static_props / animated_props, main.js:869-975).

    python -m fspt_amd.render --out bunny.png --width 960 --height 540 --spp 256 --bounces 8
    python -m fspt_amd.render --scene web/scene/bunny.json --out bunny.png
    python -m fspt_amd.render --scene 'web/scene/anim_{frame}.json' --frames 0:24 --out 'out/{frame}.png'
    python -m fspt_amd.render --out bunny.png --spp 16 --atrous 5 --feature-samples 8   # guided denoiser
    python -m fspt_amd.render --out bunny.png --spp 16 --sampler sobol --sampler-seed 3  # Owen-scrambled Sobol sampler
    python -m fspt_amd.render --scene web/scene/bunny.json --lights --emitter-fraction 0.5  # sample emissive triangles
    python -m fspt_amd.render --scene web/scene/bunny.json --lights --light-builder gpu   # ... their table built on the GPU
    python -m fspt_amd.render --mesh-n 289 --bvh gpu --spp 16 --out c3.png  # binned-SAH tree built on the GPU
    python -m fspt_amd.render --scene 'web/scene/anim_{frame}.json' --frames 0:24 --bvh refit --out 'out/{frame}.png'  # build once, refit
    python -m fspt_amd.render --scene 'web/scene/anim_{frame}.json' --frames 0:24 --bvh refit --pose --out 'out/{frame}.png'  # one matrix per prop per frame
    python -m fspt_amd.render --out bunny.jpg --jpeg-quality 90 --jpeg-444   # drawn and JPEG-encoded on the GPU
    python -m fspt_amd.render --out bunny.png --png-gpu                      # drawn, filtered and deflated on the GPU
    python -m fspt_amd.render --out bunny.exr --exr-layers albedo,normal,depth  # scene-linear OpenEXR with the guides as layers, made on the GPU
    python -m fspt_amd.render --out pano.png --width 1024 --height 512 --camera equirect  # 360-degree panorama (also: ortho, fisheye:180, stereo:0.064)

Path tracing runs in the HIP kernels (fspt_render), tone mapping in the draw.fs kernel (fspt_draw); --atrous K runs
the guided a-trous denoiser (fspt_features + fspt_denoise, K iterations) before tone mapping (fspt_draw_denoised).
"""
import argparse
import time

import numpy as np

from . import PathTracer, scene as S


def parse_camera(spec):
    """--camera pinhole|ortho|fisheye[:DEGREES]|equirect|stereo[:IPD] -> PathTracer.set_camera_model's keyword arguments
    (the fisheye's field of view over the frame height in degrees, in (0, 360]; the stereo pair's ipd in scene units)."""
    name, _, arg = spec.partition(":")
    if name not in ("pinhole", "ortho", "fisheye", "equirect", "stereo"):
        raise ValueError(f"--camera: unknown model {name!r} (pinhole, ortho, fisheye[:DEGREES], equirect, stereo[:IPD])")
    kw = {"model": name}
    if _ and name not in ("fisheye", "stereo"):
        raise ValueError(f"--camera {name} takes no argument")
    if _:
        try:
            v = float(arg)
        except ValueError:
            raise ValueError(f"--camera {name}: {arg!r} is not a number") from None
        if name == "fisheye":
            if not (np.isfinite(v) and 0.0 < v <= 360.0):
                raise ValueError("--camera fisheye:DEGREES must lie in (0, 360]")
            kw["angle"] = min(float(np.float32(np.deg2rad(v))), float(np.float32(2.0 * np.pi)))
        else:
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError("--camera stereo:IPD must be finite and >= 0")
            kw["ipd"] = v
    return kw


def parse_sky(sky, sky_to=None, size="1024x512"):
    """--sky AZIMUTH,ELEVATION[,TURBIDITY] (degrees; azimuth from +x towards +z), --sky-to AZIMUTH,ELEVATION and --sky-size WxH
    as a function of s in [0, 1] - the position in the sequence - that returns Scene.update_sky's arguments; None without --sky"""
    if sky is None:
        return None

    def numbers(text, flag, counts):
        try:
            v = [float(x) for x in text.split(",")]
        except ValueError:
            v = []
        if len(v) not in counts or not all(np.isfinite(v)):
            raise ValueError(f"{flag} takes {' or '.join(str(c) for c in counts)} finite numbers separated by commas, got {text!r}")
        return v

    a = numbers(sky, "--sky", (2, 3))
    b = numbers(sky_to, "--sky-to", (2,)) if sky_to is not None else a[:2]
    try:
        w, h = (int(x) for x in size.lower().split("x"))
    except ValueError:
        raise ValueError(f"--sky-size takes WxH, got {size!r}") from None
    turbidity = a[2] if len(a) == 3 else 1.0

    def at(s):
        az, el = a[0] + (b[0] - a[0]) * s, a[1] + (b[1] - a[1]) * s
        return dict(sun_dir=S.sun_direction(az, el), width=w, height=h, turbidity=turbidity)
    return at


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--camera", default="pinhole", metavar="MODEL",
                    help="camera model (DESIGN 8.15): pinhole | ortho | fisheye[:DEGREES over the frame height, default 180] | equirect | "
                         "stereo[:IPD in scene units, default 0.064; over-under, needs an even --height]")
    ap.add_argument("--out", default="fspt.png")
    ap.add_argument("--jpeg-quality", type=int, default=85, metavar="Q", help="--out *.jpg / *.jpeg: libjpeg quality 1..100 (encoded on the GPU, DESIGN 8.19)")
    ap.add_argument("--jpeg-444", action="store_true", help="--out *.jpg / *.jpeg: no chroma subsampling (default 4:2:0)")
    ap.add_argument("--png-gpu", action="store_true", help="--out *.png: filter and deflate the file on the GPU (DESIGN 8.20; the default is Pillow on the host)")
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--mesh-n", type=int, default=76)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--saturation", type=float, default=1.0)
    ap.add_argument("--denoise", action="store_true", help="draw.fs's 5x5 firefly clamp")
    ap.add_argument("--atrous", type=int, default=0, help="guided a-trous denoiser iterations (0 = off; built-in scene)")
    ap.add_argument("--feature-samples", type=int, default=8, help="camera rays per pixel of the denoiser's guide buffers")
    ap.add_argument("--hdr", default=None, help="also save the RGBA32F radiance buffer: a name that ends in .exr as OpenEXR made on the GPU (DESIGN 8.21), any other as .npy")
    ap.add_argument("--exr-layers", default="", help="--out / --hdr *.exr: layers beside R G B, of albedo,normal,depth,alpha,crypto_object,crypto_material (the last two: Cryptomatte ID mattes, DESIGN 8.25)")
    ap.add_argument("--matte-samples", type=int, default=8, help="camera rays per pixel of the ID mattes (--exr-layers crypto_object,crypto_material), in 1..65535")
    ap.add_argument("--exr-float", action="store_true", help="--out / --hdr *.exr: 32-bit FLOAT channels (the default is HALF; Z is always FLOAT)")
    ap.add_argument("--exr-compression", default="zip", choices=("none", "zips", "zip"), help="--out / --hdr *.exr: blocks of 16 scanlines deflated (zip, the default), of one (zips), or none")
    ap.add_argument("--scene", default=None, help="scene JSON ({frame} is replaced per frame with --frames)")
    ap.add_argument("--assets", default=None, help="web root the JSON's paths are relative to (default: parent of the scene folder)")
    ap.add_argument("--frames", default=None, help="A:B = frames A..B-1 (the reference's ?frame=N loop, main.js:851-866)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bvh", choices=("sah", "gpu", "refit"), default="sah",
                    help="BVH builder: the reference's full-sweep SAH on the CPU, or binned SAH on the GPU (DESIGN 8.4); refit (with "
                         "--frames): build the first frame, then refit the tree for frames that only move triangles (DESIGN 8.6)")
    ap.add_argument("--textures", choices=("cpu", "gpu"), default="cpu",
                    help="with --scene: where the texture atlas is resampled - numpy on the host, or a kernel on the render device "
                         "(DESIGN 8.18); with --bvh refit a changed atlas then reaches the live scene as decoded images")
    ap.add_argument("--rebuild-above", type=float, default=None, metavar="R",
                    help="--bvh refit: rebuild the tree in place on the GPU when a refitted frame's SAH cost exceeds R x the cost at "
                         "the last build (DESIGN 8.7; default: never)")
    ap.add_argument("--mesh", action="store_true",
                    help="--bvh refit --frames: a frame whose OBJs differ from the first frame's only in their `v` lines parses "
                         "only those; one position per vertex goes to the GPU, which derives the normals and refits (DESIGN 8.24; "
                         "normals from float32 positions: not bit-equal to the parse path)")
    ap.add_argument("--pose", action="store_true",
                    help="--bvh refit --frames: a frame that only moves its props rigidly parses no OBJ; one matrix per prop goes to "
                         "the GPU, which poses the first frame's triangles and refits (DESIGN 8.14; float32 matrices: not bit-equal "
                         "to the parse path)")
    ap.add_argument("--temporal", action="store_true",
                    help="--bvh refit --frames: reproject and blend every frame with the frames before it (DESIGN 8.8); with "
                         "--atrous K the a-trous filter runs on the temporal result")
    ap.add_argument("--temporal-clamp", nargs="?", type=float, const=True, default=None, metavar="SIGMA",
                    help="--temporal: a fast history bounds the long one, so that a change of the light is followed within a few "
                         "frames (DESIGN 8.10); SIGMA = the box's half width in standard deviations (default: the library's)")
    ap.add_argument("--auto-exposure", nargs="?", type=float, const=True, default=None, metavar="KEY",
                    help="meter every frame on the GPU and expose its mean log luminance to KEY (default 0.18; DESIGN 8.11); "
                         "--exposure and the scene file's `exposure` then act as compensation")
    ap.add_argument("--bloom", nargs="?", type=float, const=True, default=None, metavar="INTENSITY",
                    help="mix the glow of an HDR pyramid of every drawn frame in before the exposure (DESIGN 8.12); INTENSITY in [0, 1] "
                         "(default 0.05)")
    ap.add_argument("--variance-guided", action="store_true",
                    help="--temporal --atrous K: the K iterations are guided by the per-pixel variance estimate (DESIGN 8.9)")
    ap.add_argument("--sampler", choices=("reference", "sobol"), default="reference",
                    help="the paths' random numbers (fspt_target_set_sampler; built-in scene)")
    ap.add_argument("--sampler-seed", type=int, default=0, help="seed of --sampler sobol, in [0, 2^32)")
    ap.add_argument("--lights", action="store_true", help="next-event estimation of emissive triangles (fspt_target_set_lights)")
    ap.add_argument("--emitter-fraction", type=float, default=0.5,
                    help="with --lights: probability a vertex samples an emitter rather than the environment, in (0, 1]")
    ap.add_argument("--light-builder", choices=("host", "gpu"), default=None,
                    help="with --lights: who builds the emitter light table (fspt_scene_set_light_builder, DESIGN 8.23); gpu = on the "
                         "device, nothing but 8 bytes is read back per build")
    ap.add_argument("--adaptive", type=float, default=None, metavar="REL_MSE",
                    help="adaptive sampling: stop a 32x32 tile once its estimated relative MSE is below REL_MSE (--spp = the most)")
    ap.add_argument("--sample-map", default=None, help="with --adaptive: write the ticks per pixel as a grey PNG")
    ap.add_argument("--sky", default=None, metavar="AZIMUTH,ELEVATION[,TURBIDITY]",
                    help="replace the scene's environment by a sky generated on the GPU (DESIGN 8.17): the sun's azimuth (from +x "
                         "towards +z) and elevation in degrees, and the turbidity (default 1)")
    ap.add_argument("--sky-to", default=None, metavar="AZIMUTH,ELEVATION",
                    help="with --sky and --frames: the sun moves linearly to here over the sequence")
    ap.add_argument("--sky-size", default="1024x512", metavar="WxH", help="texels of the generated sky")
    args = ap.parse_args(argv)
    try:
        sky_at = parse_sky(args.sky, args.sky_to, args.sky_size)
    except ValueError as e:
        ap.error(str(e))
    if not 1 <= args.jpeg_quality <= 100:
        ap.error("--jpeg-quality must lie in 1..100")
    from .scene_file import is_exr_path, is_jpeg_path, write_image
    exr_out, exr_hdr = is_exr_path(args.out), bool(args.hdr) and is_exr_path(args.hdr)
    if (args.exr_layers or args.exr_float or args.exr_compression != "zip") and not (exr_out or exr_hdr):
        ap.error("--exr-layers, --exr-float and --exr-compression need an --out or --hdr that ends in .exr")
    try:
        from .tracer import exr_params
        exr = dict(compression=args.exr_compression, float32=args.exr_float, layers=[x for x in args.exr_layers.split(",") if x])
        exr_guided, exr_mattes = bool(exr_params(**exr).layers & 14), bool(exr_params(**exr).layers & 48)
    except ValueError as e:
        ap.error("--exr-layers: " + str(e))
    if exr_guided and args.scene and not (args.frames and args.bvh == "refit"):
        ap.error("--exr-layers albedo, normal and depth are available for the built-in scene, or with --frames and --bvh refit")
    if exr_mattes and args.scene and not (args.frames and args.bvh == "refit"):
        ap.error("--exr-layers crypto_object and crypto_material are available for the built-in scene, or with --frames and --bvh refit")
    if not 1 <= args.matte_samples <= 65535:
        ap.error("--matte-samples must lie in 1..65535")
    jpeg = dict(quality=args.jpeg_quality, subsampling="444" if args.jpeg_444 else "420")
    if (args.jpeg_quality != 85 or args.jpeg_444) and not is_jpeg_path(args.out):
        ap.error("--jpeg-quality and --jpeg-444 need an --out that ends in .jpg or .jpeg")
    if args.png_gpu and not args.out.lower().endswith(".png"):
        ap.error("--png-gpu needs an --out that ends in .png")
    png = "gpu" if args.png_gpu else None
    if args.sky_to is not None and not (args.sky and args.scene and args.frames):
        ap.error("--sky-to needs --sky, --scene and --frames")
    try:
        camera = parse_camera(args.camera)
    except ValueError as e:
        ap.error(str(e))
    if camera["model"] != "pinhole" and (args.adaptive is not None or args.temporal):
        ap.error("--camera other than pinhole cannot be combined with --adaptive or --temporal")
    if args.bvh == "refit" and not (args.scene and args.frames):
        ap.error("--bvh refit needs --scene and --frames (it reuses one scene across a frame sequence)")
    if args.adaptive is not None:
        if not (np.isfinite(args.adaptive) and args.adaptive >= 0.0):
            ap.error("--adaptive must be a finite relative MSE >= 0")
        if args.spp < 64 or args.spp % 32:
            ap.error("--adaptive needs --spp a multiple of 32, at least 64")
        if args.frames:
            ap.error("--adaptive renders a single frame")
    if args.sample_map and args.adaptive is None:
        ap.error("--sample-map needs --adaptive")
    if not 0.0 < args.emitter_fraction <= 1.0:
        ap.error("--emitter-fraction must lie in (0, 1]")
    if args.emitter_fraction != 0.5 and not args.lights:
        ap.error("--emitter-fraction needs --lights")
    if args.light_builder is not None and not args.lights:
        ap.error("--light-builder needs --lights")
    if args.temporal and args.adaptive is not None:
        ap.error("--temporal cannot be combined with --adaptive")
    if args.temporal and not (args.bvh == "refit" and args.frames):
        ap.error("--temporal needs --bvh refit and --frames")
    if args.pose and not (args.bvh == "refit" and args.frames):
        ap.error("--pose needs --bvh refit and --frames")
    if args.mesh and not (args.bvh == "refit" and args.frames):
        ap.error("--mesh needs --bvh refit and --frames")
    if args.temporal_clamp is not None and not args.temporal:
        ap.error("--temporal-clamp needs --temporal")
    if args.temporal_clamp is not None and args.temporal_clamp is not True and not args.temporal_clamp >= 0.0:
        ap.error("--temporal-clamp SIGMA must be >= 0")
    if args.auto_exposure is not None and args.auto_exposure is not True and not (np.isfinite(args.auto_exposure) and args.auto_exposure > 0.0):
        ap.error("--auto-exposure KEY must be a finite value > 0")
    if args.auto_exposure is not None and args.exposure != 1.0 and args.scene and args.frames:
        ap.error("--auto-exposure with --frames takes its compensation from the scene files' `exposure`, not from --exposure")
    if args.bloom is not None and args.bloom is not True and not (np.isfinite(args.bloom) and 0.0 <= args.bloom <= 1.0):
        ap.error("--bloom INTENSITY must be a finite value in [0, 1]")
    if args.variance_guided and not (args.temporal and args.atrous):
        ap.error("--variance-guided needs --temporal and --atrous K")
    if args.atrous and args.scene and not args.temporal:
        ap.error("--atrous is available for the built-in scene, or with --temporal")
    if args.scene and args.sampler != "reference":
        ap.error("--sampler is available for the built-in scene")
    if not 0 <= args.sampler_seed <= 0xFFFFFFFF:
        ap.error("--sampler-seed must lie in [0, 2^32)")
    if args.scene:
        from . import scene_file as F
        spp = args.spp if "--spp" in " ".join(__import__("sys").argv if argv is None else argv) else None  # default: the scene's `samples`
        kw = dict(samples=spp, bounces=args.bounces, seed=args.seed, saturation=args.saturation, denoise=args.denoise)
        if args.lights:
            kw.update(lights="emitters", emitter_fraction=args.emitter_fraction)
            if args.light_builder is not None:
                kw.update(light_builder=args.light_builder)
        if args.adaptive is not None:
            kw.update(samples=args.spp, adaptive=args.adaptive, sample_map=args.sample_map)
        if args.auto_exposure is not None:
            kw.update(auto_exposure=True if args.auto_exposure is True else {"key": args.auto_exposure})
        if args.bloom is not None:
            kw.update(bloom=True if args.bloom is True else {"intensity": args.bloom})
        if camera["model"] != "pinhole":
            kw.update(camera=camera)
        if args.frames:
            a, b = (int(x) for x in args.frames.split(":"))
            if sky_at is not None:
                kw.update(sky=lambda n: sky_at((n - a) / max(b - 1 - a, 1)))
            t0 = time.perf_counter()
            out = F.render_sequence(args.scene, range(a, b), args.out, args.width, args.height, args.assets, bvh=args.bvh,
                                    rebuild_above=args.rebuild_above,
                                    temporal=({"atrous": args.atrous, "clamp": None if args.temporal_clamp is None else True if args.temporal_clamp is True
                                               else {"sigma_scale": args.temporal_clamp}} if args.temporal else None),
                                    variance=args.variance_guided, pose=args.pose, mesh=args.mesh, textures=args.textures, jpeg=jpeg, png=png, exr=exr,
                                    matte_samples=args.matte_samples, **kw)
            print(f"{len(out)} frames in {time.perf_counter() - t0:.2f} s:", *out)
        else:
            arrays, settings = F.load_scene_file(args.scene, args.assets, bvh=args.bvh, textures=args.textures)
            if sky_at is not None:
                arrays = F.arrays_with_sky(arrays, **sky_at(0.0))
            settings["exposure"] = settings["exposure"] * args.exposure
            rgba, rad = F.render_frame(arrays, settings, args.width, args.height, **kw)
            if exr_hdr:
                write_image(args.hdr, np.ascontiguousarray(rad[::-1]), exr=exr)
            elif args.hdr:
                np.save(args.hdr, rad)
            write_image(args.out, np.ascontiguousarray(rad[::-1]) if exr_out else rgba, jpeg, png=png, exr=exr)
            print("wrote", args.out, f"({arrays.n_tris} triangles, {spp or settings['samples']} spp)")
        return
    t0 = time.perf_counter()
    arrays = S.bunny_scene(n=args.mesh_n, bvh=args.bvh, keep_order=exr_mattes)  # (the mattes' names come from the props)
    print(f"scene: {arrays.n_tris} triangles, {arrays.n_nodes} nodes, depth {arrays.depth} ({args.bvh} tree) in "
          f"{time.perf_counter() - t0:.2f} s")
    pt = PathTracer(arrays, args.width, args.height, num_bounces=args.bounces)
    pt.set_camera(**S.BUNNY_CAMERA)
    if camera["model"] != "pinhole":
        from . import FsptError
        try:
            pt.set_camera_model(**camera)
        except FsptError as e:  # (stereo on an odd --height: the library's message)
            ap.error(str(e))
    if args.sampler != "reference":
        pt.set_sampler(args.sampler, args.sampler_seed)
    if sky_at is not None:
        pt.update_sky(**sky_at(0.0))
        print("sky: {n_bins} bins; generated in {sky_ms:.2f} ms, binned in {bins_ms:.2f} ms, tiled in {tile_ms:.2f} ms".format(**pt.last_sky()))
    if args.lights:
        if args.light_builder is not None:
            pt.scene.set_light_builder(args.light_builder)
        pt.set_lights("emitters", args.emitter_fraction)
    if args.auto_exposure is not None:
        pt.set_auto_exposure(True, **({} if args.auto_exposure is True else {"key": args.auto_exposure}))
    if args.bloom is not None:
        pt.set_bloom(True, **({} if args.bloom is True else {"intensity": args.bloom}))
    t0 = time.perf_counter()
    if args.adaptive is None:
        pt.render(args.spp)
    else:
        pt.render_adaptive(args.adaptive, max_ticks=args.spp)
    pt.sync()
    dt = time.perf_counter() - t0
    samples = args.width * args.height * args.spp
    if args.adaptive is not None:
        samples = pt.adaptive_stats()["samples"]
        print(f"adaptive: {samples / (args.width * args.height):.1f} spp on average (at most {args.spp})")
        if args.sample_map:
            from .scene_file import write_sample_map
            write_sample_map(args.sample_map, pt.sample_counts(), args.spp)
            print("wrote", args.sample_map)
    if args.atrous > 0:
        pt.features(args.feature_samples, args.seed)
        pt.denoise(iterations=args.atrous)
    if exr_guided and args.atrous <= 0:
        pt.features(args.feature_samples, args.seed)
    if exr_mattes:
        pt.scene.set_default_mattes()
        pt.mattes(args.matte_samples, args.seed)
    if exr_out:  # the radiance itself, and the guides, as a file made on the device
        data = pt.draw_exr("denoised" if args.atrous > 0 else "accumulator", **exr)
    elif is_jpeg_path(args.out):  # drawn and encoded on the device: only the file comes back
        data = pt.draw_jpeg("denoised" if args.atrous > 0 else "accumulator", args.exposure, args.saturation, args.denoise, **jpeg)
    elif args.png_gpu:
        data = pt.draw_png("denoised" if args.atrous > 0 else "accumulator", args.exposure, args.saturation, args.denoise)
    elif args.atrous > 0:
        rgba = pt.drawDenoised(args.exposure, args.saturation)
    else:
        rgba = pt.draw(args.exposure, args.saturation, args.denoise)
    print(f"{args.width}x{args.height} x {args.spp} spp in {dt:.3f} s = {samples / dt / 1e6:.0f} Msamples/s")
    if exr_hdr:
        with open(args.hdr, "wb") as f:
            f.write(pt.draw_exr("accumulator", **exr))
    elif args.hdr:
        np.save(args.hdr, pt.readRadiance())
    if exr_out or is_jpeg_path(args.out) or args.png_gpu:
        with open(args.out, "wb") as f:
            f.write(data)
    else:
        from PIL import Image
        Image.fromarray(rgba[::-1, :, :3]).save(args.out)  # radiance rows are bottom-up (GL origin)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
