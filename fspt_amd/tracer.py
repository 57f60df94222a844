"""Host-side mirror of the reference's frame driver (main.js:741-857) on top of
libfspt: same method names, same argument meaning, same call order.

    pt = PathTracer(scene_arrays, width, height)
    pt.eye, pt.dir, pt.fovScale, pt.lensFeatures, pt.envTheta   # main.js:67-74
    pt.drawCamera(randBase); pt.drawTracer(i, randBase)          # one sample
    pt.tick()                                                    # main.js:838-857
    pt.clear()                                                   # main.js:826-836
    pt.readRadiance() -> float32 [H, W, 4], row 0 = bottom       # what draw.fs:87 reads

All compute happens in the HIP kernels; a missing library or device raises
FsptError (there is no CPU path here).
"""
import ctypes as C

import numpy as np

from . import _lib as L


def set_texture_interleave_budget(nbytes):
    """Memory later Scene()s may spend on interleaved material textures (fspt_set_texture_interleave_budget)."""
    L.check(L.lib().fspt_set_texture_interleave_budget(int(nbytes)))

def device_memory(device=0):
    """(free, total) bytes of a device as the HIP runtime reports them (fspt_device_memory): what a host sizes its batches
    against, and how the tests check that dropped tracers give their memory back."""
    f, t = C.c_uint64(), C.c_uint64()
    L.check(L.lib().fspt_device_memory(int(device), C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def sampler_eval(seed, pixel, sample, dim, device=0):
    """FSPT_SAMPLER_SOBOL's device function for the (pixel, sample, dim) triples (fspt_sampler_eval, a test hook):
    float32 values in [0, 1), arrays broadcast against each other."""
    seed = _sampler_seed(seed)
    pixel, sample, dim = (np.ascontiguousarray(a, dtype=np.uint32) for a in np.broadcast_arrays(
        *(_u32_array(a, name) for a, name in ((pixel, "pixel"), (sample, "sample"), (dim, "dim")))))
    out = np.empty(pixel.shape, np.float32)
    L.check(L.lib().fspt_sampler_eval(int(device), seed, L.u32ptr(pixel), L.u32ptr(sample), L.u32ptr(dim), int(pixel.size),
                                      L.fptr(out)))
    return out


def denoise_eval(accum, features, device=0, **params):
    """fspt_denoise's k_atrous launches on host arrays (fspt_denoise_eval, a test hook): accum float32 [H, W, 4], features
    float32 [H, W, 8] (readFeatures' layout) -> the denoised float32 [H, W, 4].  params: iterations, sigma_color,
    sigma_normal, sigma_depth; one left out takes the library's default (DENOISE_DEFAULTS)."""
    unknown = set(params) - set(DENOISE_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown denoise parameters {sorted(unknown)}")
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    features = np.ascontiguousarray(features, dtype=np.float32)
    if accum.ndim != 3 or accum.shape[2] != 4 or features.shape != accum.shape[:2] + (8,):
        raise ValueError(f"need accum [H, W, 4] and features [H, W, 8], got {accum.shape} and {features.shape}")
    H, W = accum.shape[:2]
    v = {**DENOISE_DEFAULTS, **params}
    prm = L.DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]))
    out = np.empty((H, W, 4), np.float32)
    L.check(L.lib().fspt_denoise_eval(int(device), L.fptr(accum), L.fptr(features), W, H, C.byref(prm), L.fptr(out)))
    return out


TEMPORAL_DEFAULTS = {"alpha": 0.0, "max_history": 64.0, "depth_tol": 0.05, "normal_cos": 0.95}  # include/fspt_tuning.h FSPT_TEMPORAL_*


def _temporal_params(params):
    """fspt_temporal_params from keyword arguments (None: all defaults), validated like the library does."""
    unknown = set(params) - set(TEMPORAL_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown temporal parameters {sorted(unknown)}")
    if not params:
        return None
    v = {k: float(x) for k, x in {**TEMPORAL_DEFAULTS, **params}.items()}
    if not (0.0 <= v["alpha"] <= 1.0 and v["max_history"] >= 1.0 and v["depth_tol"] >= 0.0 and -1.0 <= v["normal_cos"] <= 1.0):
        raise ValueError("temporal parameters: need alpha in [0, 1], max_history >= 1, depth_tol >= 0, normal_cos in [-1, 1]")
    return L.TemporalParams(v["alpha"], v["max_history"], v["depth_tol"], v["normal_cos"])


def temporal_eval(accum, motion, g, hist=None, g_prev=None, n=1, device=0, **params):
    """fspt_temporal_accumulate's blend pass on host arrays (fspt_temporal_eval, a test hook): accum, motion, hist float32
    [H, W, 4], g, g_prev float32 [H, W, 8] (temporal_gbuffer's layouts), n = the accumulator's ticks -> the new history
    float32 [H, W, 4] (rgb, length).  hist None: no history.  params: alpha, max_history, depth_tol, normal_cos."""
    prm = _temporal_params(params)
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    if accum.ndim != 3 or accum.shape[2] != 4:
        raise ValueError(f"need accum [H, W, 4], got {accum.shape}")
    H, W = accum.shape[:2]
    arrs = {"motion": (motion, 4), "g": (g, 8)}
    if hist is not None:
        arrs.update({"hist": (hist, 4), "g_prev": (g_prev, 8)})
    a = {}
    for name, (x, c) in arrs.items():
        if x is None or np.shape(x) != (H, W, c):
            raise ValueError(f"need {name} [{H}, {W}, {c}], got {None if x is None else np.shape(x)}")
        a[name] = np.ascontiguousarray(x, dtype=np.float32)
    if int(n) < 1:
        raise ValueError("n must be >= 1")
    out = np.empty((H, W, 4), np.float32)
    L.check(L.lib().fspt_temporal_eval(int(device), L.fptr(accum), L.fptr(a["motion"]), L.fptr(a["g"]),
                                       L.fptr(a["hist"]) if hist is not None else None, L.fptr(a["g_prev"]) if hist is not None else None,
                                       W, H, int(n), C.byref(prm) if prm is not None else None, L.fptr(out)))
    return out


SVGF_DEFAULTS = {"iterations": 4, "sigma_color": 8.0, "sigma_normal": 32.0, "sigma_depth": 0.05}  # include/fspt_tuning.h FSPT_SVGF_* (sigma_color = sigma_l)


def _svgf_params(given):
    """fspt_denoise_params of the variance-guided filter from keyword arguments (None values and an empty dict: the
    library's defaults), validated like the library does."""
    unknown = set(given) - set(SVGF_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown denoise parameters {sorted(unknown)}")
    if all(x is None for x in given.values()):
        return None
    v = {k: SVGF_DEFAULTS[k] if given.get(k) is None else given[k] for k in SVGF_DEFAULTS}
    k, sl, sn, sz = int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"])
    if not (0 <= k <= 16 and k == v["iterations"] and sl >= 0.0 and 0.0 <= sn < float("inf") and sz > 0.0):
        raise ValueError("variance-guided denoise parameters: need iterations <= 16, sigma_color >= 0, sigma_normal in [0, inf), sigma_depth > 0")
    return L.DenoiseParams(k, sl, sn, sz)


def svgf_eval(hist, moments, features, n=1, device=0, **params):
    """k_svgf_variance and the variance-guided a-trous iterations on host arrays (fspt_svgf_eval, a test hook): hist float32
    [H, W, 4] (rgb, history length), moments float32 [H, W, 2] (M1, M2), features float32 [H, W, 8], n = the accumulator's
    ticks -> (filtered float32 [H, W, 4], input variance [H, W], output variance [H, W]).  params: iterations, sigma_color
    (sigma_l, in standard deviations), sigma_normal, sigma_depth (SVGF_DEFAULTS)."""
    prm = _svgf_params(params)
    hist = np.ascontiguousarray(hist, dtype=np.float32)
    if hist.ndim != 3 or hist.shape[2] != 4:
        raise ValueError(f"need hist [H, W, 4], got {hist.shape}")
    H, W = hist.shape[:2]
    if np.shape(moments) != (H, W, 2) or np.shape(features) != (H, W, 8):
        raise ValueError(f"need moments [{H}, {W}, 2] and features [{H}, {W}, 8], got {np.shape(moments)} and {np.shape(features)}")
    moments = np.ascontiguousarray(moments, dtype=np.float32)
    features = np.ascontiguousarray(features, dtype=np.float32)
    if int(n) < 1:
        raise ValueError("n must be >= 1")
    out, vin, vout = np.empty((H, W, 4), np.float32), np.empty((H, W), np.float32), np.empty((H, W), np.float32)
    L.check(L.lib().fspt_svgf_eval(int(device), L.fptr(hist), L.fptr(moments), L.fptr(features), W, H, int(n),
                                   C.byref(prm) if prm is not None else None, L.fptr(out), L.fptr(vin), L.fptr(vout)))
    return out, vin, vout


CLAMP_DEFAULTS = {"fast_history": 32.0, "sigma_scale": 1.0}  # include/fspt_tuning.h FSPT_TEMPORAL_CLAMP_*


def _clamp_params(fast_history=None, sigma_scale=None):
    """(fast_history, sigma_scale) of the history clamp (None: CLAMP_DEFAULTS), validated like the library does."""
    fh = float(CLAMP_DEFAULTS["fast_history"] if fast_history is None else fast_history)
    ss = float(CLAMP_DEFAULTS["sigma_scale"] if sigma_scale is None else sigma_scale)
    if not (1.0 <= fh < float("inf")) or not ss >= 0.0:
        raise ValueError("history clamp: need a finite fast_history >= 1 and sigma_scale >= 0 (+inf: the clamp never binds)")
    return fh, ss


def temporal_clamp_eval(hist, fast, sigma_scale=None, device=0):
    """k_temporal_clamp on host arrays (fspt_temporal_clamp_eval, a test hook): hist, fast float32 [H, W, 4] (rgb, length)
    -> (out, lo, hi) float32 [H, W, 4]: hist.rgb clamped into the box lo..hi of fast's 5 x 5 window, .w of out = hist's,
    of lo / hi = 0.  sigma_scale None: CLAMP_DEFAULTS; +inf: out = hist, the box is -inf..+inf."""
    _, ss = _clamp_params(None, sigma_scale)
    hist = np.ascontiguousarray(hist, dtype=np.float32)
    if hist.ndim != 3 or hist.shape[2] != 4:
        raise ValueError(f"need hist [H, W, 4], got {hist.shape}")
    H, W = hist.shape[:2]
    if np.shape(fast) != (H, W, 4):
        raise ValueError(f"need fast [{H}, {W}, 4], got {np.shape(fast)}")
    fast = np.ascontiguousarray(fast, dtype=np.float32)
    out, lo, hi = (np.empty((H, W, 4), np.float32) for _ in range(3))
    L.check(L.lib().fspt_temporal_clamp_eval(int(device), L.fptr(hist), L.fptr(fast), W, H, ss, L.fptr(out), L.fptr(lo), L.fptr(hi)))
    return out, lo, hi


# include/fspt_tuning.h FSPT_EXPOSURE_*: conventions, not measurements (Reinhard's middle grey, UE4's percentiles)
EXPOSURE_DEFAULTS = {"key": 0.18, "low": 0.10, "high": 0.90, "adapt_up": 1.0, "adapt_down": 1.0, "min_log2": -8.0, "max_log2": 8.0}


def _exposure_params(params):
    """fspt_exposure_params from keyword arguments (missing ones: EXPOSURE_DEFAULTS), validated like the library does."""
    unknown = set(params) - set(EXPOSURE_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown auto-exposure parameters {sorted(unknown)}")
    v = {k: float(np.float32(x)) for k, x in {**EXPOSURE_DEFAULTS, **params}.items()}
    if not (all(np.isfinite(x) for x in v.values()) and v["key"] > 0.0 and 0.0 <= v["low"] < v["high"] <= 1.0
            and 0.0 < v["adapt_up"] <= 1.0 and 0.0 < v["adapt_down"] <= 1.0 and v["min_log2"] <= v["max_log2"]):
        raise ValueError("auto-exposure: need finite parameters with key > 0, 0 <= low < high <= 1, adapt_up and adapt_down in (0, 1], "
                         "min_log2 <= max_log2")
    return L.ExposureParams(*(v[k] for k in EXPOSURE_DEFAULTS))


def exposure_eval(rgba, viewport=None, prev=None, device=0, **params):
    """The two metering kernels on a host array (fspt_exposure_eval, a test hook): rgba float32 [H, W, 4], viewport (vw, vh) or
    None = the whole image, prev = a state dict as returned (None: never metered) -> (hist uint32 [256], state dict with
    exposure (numpy float32), valid, metered, cleared (the histogram was zero after the resolve), log2_exposure, log2_mean)."""
    prm = _exposure_params(params)
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError(f"need rgba [H, W, 4], got {rgba.shape}")
    H, W = rgba.shape[:2]
    vw, vh = (W, H) if viewport is None else (int(viewport[0]), int(viewport[1]))
    if not (1 <= vw <= W and 1 <= vh <= H):
        raise ValueError(f"viewport {vw}x{vh} does not fit the image {W}x{H}")
    st = None
    if prev is not None:
        st = L.ExposureState(float(prev["exposure"]), int(prev["valid"]), int(prev["metered"]), 0, float(prev["log2_exposure"]), float(prev["log2_mean"]))
    hist = np.zeros(256, np.uint32)
    out = L.ExposureState()
    L.check(L.lib().fspt_exposure_eval(int(device), L.fptr(rgba), W, H, vw, vh, C.byref(prm), C.byref(st) if st is not None else None,
                                       hist.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out)))
    return hist, {"exposure": np.float32(out.exposure), "valid": int(out.valid), "metered": int(out.metered), "cleared": out.reserved == 0,
                  "log2_exposure": float(out.log2_exposure), "log2_mean": float(out.log2_mean)}


def exposure_set_form(form):
    """k_exposure_histogram's form, process-wide (fspt_exposure_set_form, a measurement switch): 0 = one LDS atomic per pixel
    (shipped), 1 = same-bin lanes combined by a ballot.  The histogram is the same."""
    L.check(L.lib().fspt_exposure_set_form(int(form)))


# include/fspt_tuning.h FSPT_BLOOM_*: conventions, not measurements (the scatter form of Jimenez / Unity)
BLOOM_DEFAULTS = {"intensity": 0.05, "scatter": 0.7, "levels": 6}
BLOOM_MAX_LEVELS = 8


def _bloom_params(params):
    """fspt_bloom_params from keyword arguments (missing ones: BLOOM_DEFAULTS), validated like the library does."""
    unknown = set(params) - set(BLOOM_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown bloom parameters {sorted(unknown)}")
    v = {**BLOOM_DEFAULTS, **params}
    i, s, n = float(np.float32(v["intensity"])), float(np.float32(v["scatter"])), v["levels"]
    if not (np.isfinite(i) and np.isfinite(s) and 0.0 <= i <= 1.0 and 0.0 <= s <= 1.0 and isinstance(n, (int, np.integer)) and not isinstance(n, bool)
            and 1 <= n <= BLOOM_MAX_LEVELS):
        raise ValueError(f"bloom: need finite intensity and scatter in [0, 1] and an integer levels in [1, {BLOOM_MAX_LEVELS}]")
    return L.BloomParams(i, s, int(n))


def bloom_levels(vw, vh, levels=BLOOM_DEFAULTS["levels"]):
    """[(w_1, h_1), .. (w_n, h_n)] of a vw x vh viewport (the size rule of fspt_tuning.h; n from fspt_bloom_texels, host arithmetic)"""
    n = C.c_uint32()
    L.lib().fspt_bloom_texels(int(vw), int(vh), int(levels), C.byref(n))
    out, w, h = [], int(vw), int(vh)
    for _ in range(n.value):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def bloom_eval(rgba, viewport=None, device=0, **params):
    """The bloom kernels on a host array (fspt_bloom_eval, a test hook): rgba float32 [H, W, 4], viewport (vw, vh) or None = the
    whole image -> (down, up, bloom, mix): down = [D_1 .. D_n] and up = [U_1 .. U_n] as float32 [h_k, w_k, 4] arrays, bloom = B
    [vh, vw, 4], mix = c' [H, W, 4], the float32 a draw with denoise = 0 multiplies by the exposure (n = 0: no levels, the source)."""
    prm = _bloom_params(params)
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError(f"need rgba [H, W, 4], got {rgba.shape}")
    H, W = rgba.shape[:2]
    vw, vh = (W, H) if viewport is None else (int(viewport[0]), int(viewport[1]))
    if not (1 <= vw <= W and 1 <= vh <= H):
        raise ValueError(f"viewport {vw}x{vh} does not fit the image {W}x{H}")
    sizes = bloom_levels(vw, vh, prm.levels)
    total = sum(w * h for w, h in sizes)
    down, up = np.zeros((max(total, 1), 4), np.float32), np.zeros((max(total, 1), 4), np.float32)
    bloom, mix = np.zeros((vh, vw, 4), np.float32), np.zeros((H, W, 4), np.float32)
    n = C.c_uint32()
    L.check(L.lib().fspt_bloom_eval(int(device), L.fptr(rgba), W, H, vw, vh, C.byref(prm), C.byref(n), L.fptr(down), L.fptr(up), L.fptr(bloom), L.fptr(mix)))
    assert n.value == len(sizes)
    ds, us, at = [], [], 0
    for w, h in sizes:
        ds.append(down[at:at + w * h].reshape(h, w, 4).copy())
        us.append(up[at:at + w * h].reshape(h, w, 4).copy())
        at += w * h
    return ds, us, bloom, mix


def skin_set_form(form):
    """Where k_skin_transform reads the joint table from, process-wide (fspt_skin_set_form, a measurement switch): 0 = global
    memory, 1 = staged once per block in LDS.  The bits are the same."""
    L.check(L.lib().fspt_skin_set_form(int(form)))


def logic_set_stash(entries):
    """k_wf_logic's LDS stash of the shaded paths' rows, process-wide (fspt_logic_set_stash, a measurement switch): -1 = the
    library's choice, 0 = none (every listed path is read from memory again), n = at most n entries.  The bits are the same."""
    L.check(L.lib().fspt_logic_set_stash(int(entries)))


def bloom_set_form(form):
    """The pyramid's form, process-wide (fspt_bloom_set_form, a measurement switch): 0 = one launch per level, 1 = the small
    levels in one workgroup (k_bloom_tail).  The bits are the same."""
    L.check(L.lib().fspt_bloom_set_form(int(form)))


def bloom_set_tail_texels(n):
    """Where form 1's tail takes over: the first level with at most n texels (fspt_bloom_set_tail_texels; 0 = the shipped value)"""
    L.check(L.lib().fspt_bloom_set_tail_texels(int(n)))


JPEG_SUBSAMPLING = {"444": 0, "420": 1}
JPEG_SOURCES = {"accumulator": 0, "denoised": 1, "temporal": 2, "temporal_denoised": 3}


def jpeg_params(quality=85, subsampling="420", restart_mcus=0):
    """L.JpegParams of the wrappers' keywords (fspt_jpeg_params); the library checks the ranges"""
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(JPEG_SUBSAMPLING)}")
    return L.JpegParams(int(quality), JPEG_SUBSAMPLING[str(subsampling)], int(restart_mcus))


def jpeg_bound(width, height, quality=85, subsampling="420", restart_mcus=0):
    """Bytes no JPEG file of this size and these settings exceeds (fspt_jpeg_bound; host only)"""
    p, n = jpeg_params(quality, subsampling, restart_mcus), C.c_size_t()
    L.check(L.lib().fspt_jpeg_bound(int(width), int(height), C.byref(p), C.byref(n)))
    return int(n.value)


def _host_image(a, dtype, channels, name):
    a = np.ascontiguousarray(a)
    if a.dtype != np.dtype(dtype) or a.ndim != 3 or a.shape[2] != channels:
        raise ValueError(f"{name} must be a {dtype} [H, W, {channels}] array")
    return a


def _image_arg(a, dtype, channels, name, device, sync=True):
    """(the image, whether it is on the device, the device) of an encoder's input: a `dtype` [H, W, channels] numpy array,
    made contiguous, or a torch tensor on the device, made contiguous, with its device's index and its stream synchronised
    (sync=False: the caller has more tensors to copy and synchronises behind the last one)"""
    if not (hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)):
        return _host_image(a, dtype, channels, name), False, device
    import torch
    if a.dtype != getattr(torch, dtype) or a.dim() != 3 or a.shape[2] != channels:
        raise ValueError(f"{name} must be a {dtype} [H, W, {channels}] tensor")
    a = a.contiguous()
    device = a.device.index or 0
    if sync:
        torch.cuda.current_stream(device).synchronize()  # whatever wrote the tensor, the copy above included, has finished
    return a, True, device


class _FileBuffer:
    """The wrappers' reusable output buffer of one format; bound: the name of its fspt_*_bound.  JPEG and PNG: W*H*4 + 1024
    bytes of the last size, grown to the bound when a call reports a need.  bound_first (OpenEXR): the bound of the call's
    size and settings before the call, kept while it is large enough."""

    def __init__(self, bound, bound_first=False):
        self.bound, self.bound_first = bound, bound_first
        self.size, self.buf = None, np.empty(0, np.uint8)
        self.mattes = None  # OpenEXR with Cryptomatte layers: the call's L.ExrMattes, whose manifests count in the bound

    def grow(self, w, h, p, need=0):
        """at least the bound of (w, h, p) and `need` bytes"""
        b = C.c_size_t()
        if self.mattes is not None:
            L.check(L.lib().fspt_exr_bound_mattes(w, h, C.byref(p), C.byref(self.mattes), C.byref(b)))
        else:
            L.check(getattr(L.lib(), self.bound)(w, h, C.byref(p), C.byref(b)))
        if self.buf.size < max(int(b.value), int(need)):
            self.buf = np.empty(max(int(b.value), int(need)), np.uint8)

    def ready(self, w, h, p):
        """the buffer a call of this size and these settings starts with"""
        if self.bound_first:
            self.grow(w, h, p)
        elif self.size != (w, h):
            self.size, self.buf = (w, h), np.empty(w * h * 4 + 1024, np.uint8)
        return self.buf

    def call(self, w, h, p, fn):
        """The file (bytes) of fn(out pointer, cap, byref(bytes)) -> rc, repeated once with a grown buffer when the first was
        too small"""
        n = C.c_size_t()
        self.ready(w, h, p)
        rc = fn(L.u8ptr(self.buf), self.buf.size, C.byref(n))
        if rc == -1 and n.value > self.buf.size:
            self.grow(w, h, p, n.value)
            rc = fn(L.u8ptr(self.buf), self.buf.size, C.byref(n))
        L.check(rc)
        return self.buf[:int(n.value)].tobytes()


def _last_ms(name):
    """((the three stages' ms), bytes brought to the host) of the last stand-alone encode of a format (fspt_<name>_last_ms)"""
    ms, n = (C.c_float * 3)(), C.c_uint64()
    L.check(getattr(L.lib(), f"fspt_{name}_last_ms")(ms, C.byref(n)))
    return tuple(float(x) for x in ms), int(n.value)


_jpeg_buffer, _png_buffer, _exr_buffer = _FileBuffer("fspt_jpeg_bound"), _FileBuffer("fspt_png_bound"), _FileBuffer("fspt_exr_bound", True)


def _encode_rgba8(buf, host_entry, device_entry, image, p, bottom_up, device):
    """jpeg_encode and png_encode behind their parameters"""
    image, on_dev, device = _image_arg(image, "uint8", 4, "image", device)
    h, w = int(image.shape[0]), int(image.shape[1])
    src = C.c_void_p(image.data_ptr()) if on_dev else L.u8ptr(image)
    entry = getattr(L.lib(), device_entry if on_dev else host_entry)
    return buf.call(w, h, p, lambda o, cap, nb: entry(int(device), src, w, h, 1 if bottom_up else 0, C.byref(p), o, cap, nb))


def jpeg_encode(image, quality=85, subsampling="420", restart_mcus=0, bottom_up=False, device=0):
    """A baseline JPEG file (bytes) of an RGBA8 image [H, W, 4], encoded on the GPU (fspt_jpeg_encode): a numpy
    array, or a torch tensor on the device, which is read where it is (fspt_jpeg_encode_device).  Alpha is ignored;
    bottom_up: row 0 is the bottom, as draw() returns it."""
    return _encode_rgba8(_jpeg_buffer, "fspt_jpeg_encode", "fspt_jpeg_encode_device", image, jpeg_params(quality, subsampling, restart_mcus), bottom_up, device)


def jpeg_coefficients_eval(image, quality=85, subsampling="420", bottom_up=False, device=0):
    """Stage one of the encoder alone (fspt_jpeg_coefficients_eval): int16 [blocks, 64], zig-zag order, MCU-major"""
    p = jpeg_params(quality, subsampling, 0)
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    m = 16 if p.subsampling else 8
    out = np.zeros((((w + m - 1) // m) * ((h + m - 1) // m) * (6 if p.subsampling else 3), 64), np.int16)
    L.check(L.lib().fspt_jpeg_coefficients_eval(int(device), L.u8ptr(image), w, h, 1 if bottom_up else 0, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int16))))
    return out


def jpeg_last_ms():
    """((blocks ms, entropy ms, offsets + pack ms), bytes brought to the host) of the last jpeg_encode (fspt_jpeg_last_ms)"""
    return _last_ms("jpeg")


PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


def png_params(channels=3, filter="adaptive", chunk_bytes=0):
    """L.PngParams of the wrappers' keywords (fspt_png_params); filter: a name of PNG_FILTERS or its number.
    The library checks the ranges."""
    if int(channels) not in (3, 4):
        raise ValueError("channels must be 3 or 4")
    if filter not in PNG_FILTERS and filter not in PNG_FILTERS.values():
        raise ValueError(f"filter must be one of {sorted(PNG_FILTERS)} or 0..5")
    return L.PngParams(int(channels), PNG_FILTERS.get(filter, filter), int(chunk_bytes))


def png_bound(width, height, channels=3, filter="adaptive", chunk_bytes=0):
    """Bytes no PNG file of this size and these settings exceeds (fspt_png_bound; host only)"""
    p, n = png_params(channels, filter, chunk_bytes), C.c_size_t()
    L.check(L.lib().fspt_png_bound(int(width), int(height), C.byref(p), C.byref(n)))
    return int(n.value)


def png_encode(image, channels=3, filter="adaptive", chunk_bytes=0, bottom_up=False, device=0):
    """A PNG file (bytes) of an RGBA8 image [H, W, 4], encoded on the GPU (fspt_png_encode): a numpy array, or
    a torch tensor on the device, which is read where it is (fspt_png_encode_device).  channels 3 drops alpha, 4 keeps it
    (straight); bottom_up: row 0 is the bottom, as draw() returns it."""
    return _encode_rgba8(_png_buffer, "fspt_png_encode", "fspt_png_encode_device", image, png_params(channels, filter, chunk_bytes), bottom_up, device)


def png_filtered_eval(image, channels=3, filter="adaptive", bottom_up=False, device=0):
    """Stage one of the encoder alone (fspt_png_filtered_eval): the filtered stream, uint8 [H, 1 + W * channels]"""
    p = png_params(channels, filter, 0)
    image = _host_image(image, "uint8", 4, "image")
    h, w = image.shape[:2]
    out = np.zeros((h, 1 + w * p.channels), np.uint8)
    L.check(L.lib().fspt_png_filtered_eval(int(device), L.u8ptr(image), w, h, 1 if bottom_up else 0, C.byref(p), L.u8ptr(out)))
    return out


def png_last_ms():
    """((filter ms, deflate ms, offsets + pack ms), bytes brought to the host) of the last png_encode (fspt_png_last_ms)"""
    return _last_ms("png")


EXR_COMPRESSIONS = {"none": 0, "zips": 2, "zip": 3}
EXR_LAYERS = {"alpha": 1, "albedo": 2, "normal": 4, "depth": 8, "crypto_object": 16, "crypto_material": 32}
EXR_GUIDED = 2 | 4 | 8  # the layers that read the features
EXR_CRYPTO = 16 | 32    # the Cryptomatte layers: draw_exr and exr_encode(mattes=...) take them, exr_bound does not
MATTE_KINDS = {"object": 0, "material": 1}


def _matte_kind(kind):
    if kind not in MATTE_KINDS and kind not in MATTE_KINDS.values():
        raise ValueError(f"kind must be one of {sorted(MATTE_KINDS)}")
    return MATTE_KINDS.get(kind, kind)


def matte_hash(name):
    """The 32-bit id of a name (fspt_matte_hash): MurmurHash3_x86_32 of its UTF-8 bytes with seed 0, then
    Cryptomatte's float rule (an exponent field of 0 or 255 has bit 23 flipped)."""
    b = name if isinstance(name, bytes) else str(name).encode("utf-8")
    return int(L.lib().fspt_matte_hash(b, len(b)))


def matte_manifest(names):
    """Cryptomatte's manifest of `names`: JSON {"name":"%08x", ...} in the order given, as bytes"""
    import json
    return ("{" + ",".join("%s:\"%08x\"" % (json.dumps(str(n)), matte_hash(n)) for n in names) + "}").encode("utf-8")


def _exr_mattes(mattes, shape, on_dev):
    """(L.ExrMattes, what it points to) of exr_encode's mattes={kind: ranks or (ranks, manifest bytes)}; ranks float32 [H, W, 12]"""
    m, keep = L.ExrMattes(), []
    for kind, v in (mattes or {}).items():
        k = _matte_kind(kind)
        ranks, manifest = v if isinstance(v, tuple) else (v, b"")
        if on_dev:
            import torch
            if not getattr(ranks, "is_cuda", False) or ranks.dtype != torch.float32 or tuple(ranks.shape) != shape + (12,):
                raise ValueError("matte ranks must be float32 [H, W, 12] tensors on the device of rgba")
            ranks = ranks.contiguous()
            m.ranks[k] = ranks.data_ptr()
        else:
            ranks = np.ascontiguousarray(ranks)
            if ranks.dtype != np.float32 or ranks.shape != shape + (12,):
                raise ValueError("matte ranks must be float32 [H, W, 12] arrays")
            m.ranks[k] = ranks.ctypes.data
        manifest = bytes(manifest or b"")
        m.manifest[k], m.manifest_len[k] = (manifest if manifest else None), len(manifest)
        keep += [ranks, manifest]
    return m, keep


def exr_params(compression="zip", float32=False, layers=(), chunk_bytes=0):
    """L.ExrParams of the wrappers' keywords (fspt_exr_params).  compression: a name of EXR_COMPRESSIONS or its
    number; float32: FLOAT channels, not HALF (Z is always FLOAT); layers: names of EXR_LAYERS (a sequence, or one string
    with commas) or their bit set.  The library checks the ranges."""
    if compression not in EXR_COMPRESSIONS and compression not in EXR_COMPRESSIONS.values():
        raise ValueError(f"compression must be one of {sorted(EXR_COMPRESSIONS)}")
    if isinstance(layers, str):
        layers = [x for x in layers.split(",") if x]
    if not isinstance(layers, int):
        bad = [x for x in layers if x not in EXR_LAYERS]
        if bad:
            raise ValueError(f"layers must be among {sorted(EXR_LAYERS)}, not {bad}")
        bits = 0
        for x in layers:
            bits |= EXR_LAYERS[x]
        layers = bits
    return L.ExrParams(EXR_COMPRESSIONS.get(compression, compression), 2 if float32 else 1, int(layers), int(chunk_bytes))


def exr_bound(width, height, compression="zip", float32=False, layers=(), chunk_bytes=0):
    """Bytes no OpenEXR file of this size and these settings exceeds (fspt_exr_bound; host only)"""
    p, n = exr_params(compression, float32, layers, chunk_bytes), C.c_size_t()
    L.check(L.lib().fspt_exr_bound(int(width), int(height), C.byref(p), C.byref(n)))
    return int(n.value)


def exr_encode(rgba, features=None, compression="zip", float32=False, layers=(), chunk_bytes=0, bottom_up=False, device=0, mattes=None):
    """A scanline OpenEXR file (bytes) of float32 radiance [H, W, 4] and, for the albedo, normal and depth layers, the
    features [H, W, 8] as readFeatures() returns them, encoded on the GPU (fspt_exr_encode): numpy arrays, or
    torch tensors on the device, which are read where they are (fspt_exr_encode_device).  bottom_up: row 0 is the bottom, as
    every buffer of the library; the file's first scanline is the top.  mattes: {"object" / "material":
    ranks [H, W, 12] as fspt_read_mattes returns them, or (ranks, manifest bytes)} for the "crypto_object" /
    "crypto_material" layers (fspt_exr_encode_mattes); arrays or tensors like rgba."""
    p = exr_params(compression, float32, layers, chunk_bytes)
    rgba, on_dev, device = _image_arg(rgba, "float32", 4, "rgba", device, sync=False)
    m, keep = _exr_mattes(mattes, (int(rgba.shape[0]), int(rgba.shape[1])), on_dev) if mattes is not None else (None, None)
    if on_dev:
        import torch
        if features is not None:
            if not getattr(features, "is_cuda", False) or features.dtype != torch.float32 or tuple(features.shape) != (rgba.shape[0], rgba.shape[1], 8) or features.device != rgba.device:
                raise ValueError("features must be a float32 [H, W, 8] tensor on the device of rgba")
            features = features.contiguous()
        torch.cuda.current_stream(device).synchronize()  # whatever wrote the tensors, the copies above included, has finished
    elif features is not None:
        features = np.ascontiguousarray(features)
        if features.dtype != np.float32 or features.shape != (rgba.shape[0], rgba.shape[1], 8):
            raise ValueError("features must be a float32 [H, W, 8] array")
    h, w = int(rgba.shape[0]), int(rgba.shape[1])
    lib, bu = L.lib(), 1 if bottom_up else 0
    if m is not None:
        buf = _FileBuffer("fspt_exr_bound", True)
        buf.mattes = m
        if on_dev:
            f = C.c_void_p(features.data_ptr()) if features is not None else None
            return buf.call(w, h, p, lambda o, cap, nb: lib.fspt_exr_encode_mattes_device(int(device), C.c_void_p(rgba.data_ptr()), f, C.byref(m), w, h, bu, C.byref(p), o, cap, nb))
        f = L.fptr(features) if features is not None else None
        return buf.call(w, h, p, lambda o, cap, nb: lib.fspt_exr_encode_mattes(int(device), L.fptr(rgba), f, C.byref(m), w, h, bu, C.byref(p), o, cap, nb))
    if on_dev:
        f = C.c_void_p(features.data_ptr()) if features is not None else None
        return _exr_buffer.call(w, h, p, lambda o, cap, nb: lib.fspt_exr_encode_device(int(device), C.c_void_p(rgba.data_ptr()), f, w, h, bu, C.byref(p), o, cap, nb))
    f = L.fptr(features) if features is not None else None
    return _exr_buffer.call(w, h, p, lambda o, cap, nb: lib.fspt_exr_encode(int(device), L.fptr(rgba), f, w, h, bu, C.byref(p), o, cap, nb))


def exr_set_form(form):
    """Where a block that falls back to raw takes its bytes from (fspt_exr_set_form): 0 = converted again, 1 = a kept copy"""
    L.check(L.lib().fspt_exr_set_form(int(form)))


def exr_last_ms():
    """((rows ms, deflate ms, offsets + pack ms), bytes brought to the host) of the last exr_encode (fspt_exr_last_ms)"""
    return _last_ms("exr")


def light_alias_table(weights):
    """The Vose alias table (float32 prob, uint32 alias) the light table stores for these weights (fspt_light_alias_table,
    a pure host function: no device needed)."""
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w.size == 0:
        raise ValueError("weights must not be empty")
    prob = np.empty(w.size, np.float32)
    alias = np.empty(w.size, np.uint32)
    L.check(L.lib().fspt_light_alias_table(L.fptr(w), int(w.size), L.fptr(prob), L.u32ptr(alias)))
    return prob, alias


def light_alias_table_gpu(weights, device=0):
    """(prob float32, alias uint32, light_p float32) of the GPU builder's table for these raw weights (finite, >= 0, some
    > 0; fspt_light_alias_table_gpu, a test hook)."""
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w.size == 0:
        raise ValueError("weights must not be empty")
    prob = np.empty(w.size, np.float32)
    alias = np.empty(w.size, np.uint32)
    lp = np.empty(w.size, np.float32)
    L.check(L.lib().fspt_light_alias_table_gpu(int(device), L.fptr(w), int(w.size), L.fptr(prob), L.u32ptr(alias), L.fptr(lp)))
    return prob, alias, lp


def _u32_array(a, name):
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError("%s must be integers, got %s" % (name, a.dtype))
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("%s must lie in [0, 2^32)" % name)
    return a


def _sampler_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("sampler seed must be an integer, got %r" % (seed,))
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("sampler seed must lie in [0, 2^32), got %d" % int(seed))
    return int(seed)


PIPELINES = {"megakernel": 0, "wavefront": 1, "stream": 2}  # fspt_target_set_pipeline codes
SAMPLERS = {"reference": 0, "sobol": 1}  # fspt_target_set_sampler codes
LIGHTS = {"off": 0, "emitters": 1}  # fspt_target_set_lights codes
LIGHT_BUILDERS = {"host": 0, "gpu": 1}  # fspt_scene_set_light_builder codes
CAMERA_MODELS = {"pinhole": 0, "ortho": 1, "fisheye": 2, "equirect": 3, "stereo": 4}  # fspt_target_set_camera_model codes


def camera_model_params(model="pinhole", angle=None, ipd=None):
    """set_camera_model's arguments, checked, as the fspt_camera_model_params the library takes (it checks them again,
    and the target's height for "stereo").  angle (radians) only goes with "fisheye", ipd only with "stereo"."""
    if model is None:
        model = "pinhole"
    if model not in CAMERA_MODELS:
        raise ValueError("camera model must be one of %s, got %r" % (sorted(CAMERA_MODELS), model))
    for name, v, owner in (("angle", angle, "fisheye"), ("ipd", ipd, "stereo")):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("%s must be a number, got %r" % (name, v))
        if model != owner:
            raise ValueError("%s only goes with the %r camera model, got %r" % (name, owner, model))
    a = np.float32(np.pi) if angle is None else np.float32(angle)
    d = np.float32(0.064) if ipd is None else np.float32(ipd)
    if model == "fisheye" and not (np.isfinite(a) and 0.0 < a <= np.float32(2.0 * np.pi)):
        raise ValueError("fisheye angle must lie in (0, 2 pi] radians, got %r" % (angle,))
    if model == "stereo" and not (np.isfinite(d) and d >= 0.0):
        raise ValueError("stereo ipd must be finite and >= 0, got %r" % (ipd,))
    return L.CameraModelParams(CAMERA_MODELS[model], float(a), float(d))
# fspt_denoise's defaults (include/fspt.h FSPT_DENOISE_*; tests/test_denoise_cpu.py pins the two)
DENOISE_DEFAULTS = {"iterations": 4, "sigma_color": 4.0, "sigma_normal": 32.0, "sigma_depth": 0.05}


def _map_side(fn, v):
    """A map's width or height as the uint32 the library takes (it checks the range 1..65535 itself)"""
    if int(v) != v or not 0 <= int(v) < 2 ** 32:
        raise ValueError(f"{fn}: {v!r} is not a map size")
    return int(v)


def _host_geometry(fn, n, tri, norm):
    """(tri, norm) as contiguous float32 host arrays of n x 9 and n x 27 elements (norm may be None)"""
    tri = np.ascontiguousarray(tri, dtype=np.float32)
    if tri.size != n * 9:
        raise ValueError(f"{fn}: tri has {tri.size} elements, the scene needs {n} x 9")
    if norm is not None:
        norm = np.ascontiguousarray(norm, dtype=np.float32)
        if norm.size != n * 27:
            raise ValueError(f"{fn}: norm has {norm.size} elements, the scene needs {n} x 27")
    return tri, norm


class Scene:
    """Device-resident scene (initBVH's texture uploads, main.js:408-437,548-560)."""

    def __init__(self, arrays, device=0):
        self.arrays = arrays
        self.device = device
        self._h = C.c_void_p()
        self.matte_manifests = {}  # kind number -> the manifest bytes set_matte handed the library
        desc = arrays.desc()
        L.check(L.lib().fspt_scene_create(C.byref(desc), device, C.byref(self._h)))

    @property
    def depth(self):
        d = C.c_uint32()
        L.check(L.lib().fspt_scene_depth(self._h, C.byref(d)))
        return d.value

    def intersect(self, rays, two_level=False):
        """intersectScene (tracer.fs:366-404) for rays float32 [n, 6] -> t, index, steps, leaves.  two_level: walk the
        128-byte two-level nodes (include/fspt_tuning.h: fspt_target_set_node_form) - same results, same counts."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        t = np.zeros(n, np.float32); idx = np.zeros(n, np.int32)
        steps = np.zeros(n, np.uint32); leaves = np.zeros(n, np.uint32)
        L.check(L.lib().fspt_intersect_form(self._h, 1 if two_level else 0, L.fptr(rays), n, L.fptr(t),
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), L.u32ptr(steps), L.u32ptr(leaves)))
        return t, idx, steps, leaves

    def light_count(self):
        """Entries of the emitter light table (fspt_scene_light_count; builds the table if no tracer has yet)."""
        n = C.c_uint32()
        L.check(L.lib().fspt_scene_light_count(self._h, C.byref(n)))
        return int(n.value)

    def light_table(self):
        """The emitter light table (fspt_scene_light_table) as a dict of numpy arrays: weights (per triangle),
        prob, alias, tris (per entry), pick, slot_tri (per leaf slot)."""
        nt, nl, ns = C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.check(L.lib().fspt_scene_light_table(self._h, C.byref(nt), C.byref(nl), C.byref(ns), None, None, None, None, None, None))
        r = {"weights": np.zeros(nt.value, np.float32), "prob": np.zeros(nl.value, np.float32),
             "alias": np.zeros(nl.value, np.uint32), "tris": np.zeros(nl.value, np.uint32),
             "pick": np.zeros(ns.value, np.float32), "slot_tri": np.zeros(ns.value, np.uint32)}
        L.check(L.lib().fspt_scene_light_table(self._h, None, None, None, L.fptr(r["weights"]), L.fptr(r["prob"]),
                                               L.u32ptr(r["alias"]), L.u32ptr(r["tris"]), L.fptr(r["pick"]),
                                               L.u32ptr(r["slot_tri"])))
        return r

    def set_light_builder(self, builder):
        """Who builds the emitter light table (fspt_scene_set_light_builder): "host" (default) or "gpu" (nothing
        but 8 bytes crosses the bus per build; the same entries, not the same bytes).  Drops an existing table; rebuilt at
        once when a tracer of the scene has lights on."""
        if builder not in LIGHT_BUILDERS:
            raise ValueError("light builder must be one of %s, got %r" % (sorted(LIGHT_BUILDERS), builder))
        L.check(L.lib().fspt_scene_set_light_builder(self._h, LIGHT_BUILDERS[builder]))

    @property
    def light_builder(self):
        b = C.c_int()
        L.check(L.lib().fspt_scene_get_light_builder(self._h, C.byref(b)))
        return {v: n for n, v in LIGHT_BUILDERS.items()}[b.value]

    def light_build_stats(self):
        """(bytes device -> host, bytes host -> device, GPU ms) of the scene's last light-table build
        (fspt_scene_light_build_stats); zeros before the first.  Blocking."""
        d, h, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        L.check(L.lib().fspt_scene_light_build_stats(self._h, C.byref(d), C.byref(h), C.byref(ms)))
        return int(d.value), int(h.value), float(ms.value)

    def light_sample_eval(self, queries):
        """The device's emitter sample for queries float32 [n, 10] = (ro.xyz, n.xyz, u0, u1, u2, u3; u1 is the
        alias draw v, u0 is unused) (fspt_light_sample_eval, a test hook) -> tri int32 [n], out float32 [n, 8] =
        (point.xyz, pdf_L, Le.rgb, n . w)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 10)
        tri = np.zeros(q.shape[0], np.int32)
        out = np.zeros((q.shape[0], 8), np.float32)
        L.check(L.lib().fspt_light_sample_eval(self._h, L.fptr(q), int(q.shape[0]), tri.ctypes.data_as(C.POINTER(C.c_int32)),
                                               L.fptr(out)))
        return tri, out

    # ---- ID mattes (include/fspt.h fspt_scene_set_matte_ids / _manifest) -------------------------------
    def set_matte(self, kind, tri_label, names):
        """The ids of kind "object" or "material": tri_label [n_tris] = per triangle (the scene's current leaf order) an
        index into `names`, negative = no matte (id 0); a triangle's id is matte_hash of its name, the manifest
        matte_manifest(names).  Two different names with one hash: ValueError.  tri_label None drops the kind."""
        k = _matte_kind(kind)
        lib = L.lib()
        if tri_label is None:
            L.check(lib.fspt_scene_set_matte_ids(self._h, k, None))
            L.check(lib.fspt_scene_set_matte_manifest(self._h, k, None, 0))
            self.matte_manifests.pop(k, None)
            return
        names = [str(n) for n in names]
        hashes, seen = np.array([matte_hash(n) for n in names], np.uint32).reshape(-1), {}
        for n, h in zip(names, hashes):
            if seen.setdefault(int(h), n) != n:
                raise ValueError(f"set_matte: the names {seen[int(h)]!r} and {n!r} have one hash, {int(h):08x}")
        label = np.asarray(tri_label).astype(np.int64).reshape(-1)
        if label.size != int(self.arrays.n_tris):
            raise ValueError(f"set_matte: {label.size} labels, the scene has {int(self.arrays.n_tris)} triangles")
        if label.size and label.max() >= len(names):
            raise ValueError(f"set_matte: label {int(label.max())}, {len(names)} names")
        ids = np.zeros(label.size, np.uint32)
        if len(names):
            ids = np.where(label >= 0, hashes[np.clip(label, 0, len(names) - 1)], np.uint32(0)).astype(np.uint32)
        ids = np.ascontiguousarray(ids)
        manifest = matte_manifest(names)
        L.check(lib.fspt_scene_set_matte_ids(self._h, k, L.u32ptr(ids)))
        L.check(lib.fspt_scene_set_matte_manifest(self._h, k, manifest, len(manifest)))
        self.matte_manifests[k] = manifest

    def set_matte_ids(self, kind, ids):
        """The raw form (fspt_scene_set_matte_ids): one uint32 id per triangle, 0 = no matte; None drops the kind"""
        k = _matte_kind(kind)
        if ids is None:
            L.check(L.lib().fspt_scene_set_matte_ids(self._h, k, None))
            return
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if ids.size != int(self.arrays.n_tris):
            raise ValueError(f"set_matte_ids: {ids.size} ids, the scene has {int(self.arrays.n_tris)} triangles")
        L.check(L.lib().fspt_scene_set_matte_ids(self._h, k, L.u32ptr(ids)))

    def set_default_mattes(self):
        """Objects from meta["tri_part"] and meta["prop_names"] (build_scene(..., keep_order=True)), materials from the
        distinct rows of arrays.mat, named m0000, m0001, ... in order of first appearance."""
        meta = getattr(self.arrays, "meta", None) or {}
        if "tri_part" not in meta or "prop_names" not in meta:
            raise ValueError("set_default_mattes: the arrays carry no meta['tri_part'] / meta['prop_names'] (build_scene(..., keep_order=True))")
        self.set_matte("object", meta["tri_part"], meta["prop_names"])
        rows = np.ascontiguousarray(self.arrays.mat, dtype=np.float32).reshape(-1, 12).view(np.uint32)
        _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))  # a distinct row's number in order of first appearance
        self.set_matte("material", rank[np.asarray(inverse).reshape(-1)], ["m%04d" % i for i in range(len(first))])

    def two_level_nodes(self):
        """(the scene has two-level nodes, their bytes): fspt_scene_create builds them when every box of the tree is the
        exact union of its children's boxes (every tree bvh.js builds)."""
        yes = C.c_int(); b = C.c_uint64()
        L.check(L.lib().fspt_scene_two_level_nodes(self._h, C.byref(yes), C.byref(b)))
        return bool(yes.value), int(b.value)

    def _geometry_args(self, fn, tri, norm):
        """(on device, tri, norm) checked for update_geometry / rebuild_geometry: ctypes pointers of device tensors, or
        contiguous float32 numpy arrays"""
        n = int(self.arrays.n_tris)
        on_dev = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in (tri, norm) if a is not None]
        if any(on_dev):
            if not all(on_dev):
                raise TypeError(f"{fn}: tri and norm must both be device tensors or both host arrays")
            import torch
            ptrs = []
            for name, a, k in (("tri", tri, 9), ("norm", norm, 27)):
                if a is None:
                    ptrs.append(None)
                    continue
                if a.dtype != torch.float32 or not a.is_contiguous():
                    raise TypeError(f"{fn}: {name} must be a contiguous float32 tensor")
                if a.device.index != self.device:
                    raise ValueError(f"{fn}: {name} lives on {a.device}, the scene on device {self.device}")
                if a.numel() != n * k:
                    raise ValueError(f"{fn}: {name} has {a.numel()} elements, the scene needs {n} x {k}")
                ptrs.append(C.c_void_p(a.data_ptr()))
            torch.cuda.current_stream(self.device).synchronize()  # whatever wrote the tensors has finished
            return True, ptrs[0], ptrs[1]
        return (False,) + _host_geometry(fn, n, tri, norm)

    def update_geometry(self, tri, norm=None):
        """New vertices (9 floats per triangle) and, unless norm is None, normTex records (27 per triangle) for the scene's
        n_tris triangles in LEAF order (scene.geometry_in_leaf_order): the tree is refitted on the GPU, nothing else changes
        (fspt_scene_update_geometry).  numpy arrays are uploaded; float32 torch tensors on the scene's device
        are read where they are (the `_device` form, no copy).  Accumulators are not cleared; `self.arrays` is not touched."""
        on_dev, tri, norm = self._geometry_args("update_geometry", tri, norm)
        if on_dev:
            L.check(L.lib().fspt_scene_update_geometry_device(self._h, tri, norm))
        else:
            L.check(L.lib().fspt_scene_update_geometry(self._h, L.fptr(tri), None if norm is None else L.fptr(norm)))
        self._moved = True  # (set_pose's default rest mesh is self.arrays: no longer what the scene holds)

    def rebuild_geometry(self, tri, norm=None):
        """The same input as update_geometry, but the scene gets a NEW tree: the binned-SAH tree of build_scene(bvh="gpu")
        over `tri` in the order given, built on the GPU and installed in this scene - tracers stay valid, accumulators are
        not cleared (fspt_scene_rebuild_geometry).  Returns the permutation `order`: the triangle now at leaf
        position k is input triangle order[k]; "leaf order" means the new order from here on, so the next update_geometry /
        rebuild_geometry takes tri[order] (scene.compose_order keeps a parse-order map current).  numpy in, numpy uint32
        out; float32 torch tensors on the scene's device in, an int64 tensor on that device out.  A scene first built by the
        reference's sweep (bvh="sah") becomes a binned-SAH tree, which renders 0.94-0.95x as fast; rebuilding
        a bvh="gpu" scene with its own triangles changes nothing (order = arange).  Any error leaves the scene as it was."""
        n = int(self.arrays.n_tris)
        on_dev, tri, norm = self._geometry_args("rebuild_geometry", tri, norm)
        self._moved = True
        if on_dev:
            import torch
            order = torch.empty(n, dtype=torch.int32, device=f"cuda:{self.device}")
            L.check(L.lib().fspt_scene_rebuild_geometry_device(self._h, tri, norm, C.c_void_p(order.data_ptr())))
            return order.to(torch.int64)
        order = np.zeros(n, np.uint32)
        L.check(L.lib().fspt_scene_rebuild_geometry(self._h, L.fptr(tri), None if norm is None else L.fptr(norm), L.u32ptr(order)))
        return order

    def set_pose(self, part, tri=None, norm=None, n_parts=None):
        """Hand the scene a pose (fspt_scene_set_pose): `part` = one part id per triangle in the current LEAF
        order (meta["tri_part"] of build_scene(keep_order=True)), tri / norm = the rest mesh in that order.  The default
        is the scene's own arrays - tri AND norm of `self.arrays`; it is refused once update_geometry /
        rebuild_geometry has given the scene other triangles or another order.  With tri given and norm None the pose has no rest normals:
        update_transforms then leaves the normal part of the hit records alone.  part=None drops the pose and frees it.
        n_parts: the number of parts when it is more than max(part) + 1.  Nothing renders differently until update_transforms."""
        if part is None:
            L.check(L.lib().fspt_scene_set_pose(self._h, None, 0, None, None))
            return
        n = int(self.arrays.n_tris)
        if tri is None:
            if norm is not None:
                raise ValueError("set_pose: norm given without tri")
            if getattr(self, "_moved", False):
                raise ValueError("set_pose: the scene's geometry is no longer that of its arrays; pass tri (and norm) in the current leaf order")
            tri, norm = self.arrays.tri, self.arrays.norm
        part = np.ascontiguousarray(_u32_array(part, "part"), dtype=np.uint32).reshape(-1)
        if part.size != n:
            raise ValueError(f"set_pose: part has {part.size} elements, the scene has {n} triangles")
        _, tri, norm = self._geometry_args("set_pose", np.asarray(tri), None if norm is None else np.asarray(norm))
        n_parts = int(n_parts) if n_parts is not None else int(part.max()) + 1 if n else 1
        L.check(L.lib().fspt_scene_set_pose(self._h, L.u32ptr(part), n_parts, L.fptr(tri), None if norm is None else L.fptr(norm)))

    def update_transforms(self, xf):
        """One 3 x 4 matrix per part (float32 [n_parts, 12] or [n_parts, 3, 4], row-major: a00 a01 a02 tx | ...): the rest
        mesh is posed by a kernel - vertices by the matrix, tangents and bitangents by its 3 x 3 part and normals by its
        cofactor matrix, both scaled to the matrix's rms - and the tree refitted exactly as update_geometry on the posed
        arrays would (fspt_scene_update_transforms).  n_parts is set_pose's: max(part) + 1 unless given."""
        xf = np.ascontiguousarray(xf, dtype=np.float32).reshape(-1)
        if xf.size % 12:
            raise ValueError(f"update_transforms: xf has {xf.size} elements, not n_parts x 12")
        L.check(L.lib().fspt_scene_update_transforms(self._h, L.fptr(xf), xf.size // 12))

    def read_pose(self):
        """(tri [n, 9], norm [n, 27] or None) as the most recent update_transforms posed them (fspt_scene_read_pose)."""
        n = int(self.arrays.n_tris)
        tri = np.zeros((n, 9), np.float32)
        norm = np.zeros((n, 27), np.float32)
        if L.lib().fspt_scene_read_pose(self._h, L.fptr(tri), L.fptr(norm)) == 0:
            return tri, norm
        L.check(L.lib().fspt_scene_read_pose(self._h, L.fptr(tri), None))  # (a pose without rest normals)
        return tri, None

    def last_pose_ms(self):
        """The most recent update_transforms as a dict: transform_ms (k_pose_transform), refit_ms, launches."""
        a, b, n = C.c_float(), C.c_float(), C.c_uint32()
        L.check(L.lib().fspt_scene_last_pose_ms(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return dict(transform_ms=float(a.value), refit_ms=float(b.value), launches=int(n.value))

    @staticmethod
    def _skin_desc(fn, n, joints, weights, tri, norm, morph, morph_norm, n_joints):
        """(fspt_skin_desc, the arrays it points into) for n triangles; sizes and types checked here, values by the library"""
        joints = _u32_array(joints, "joints")
        if joints.size and joints.max() > 0xFFFF:
            raise ValueError(f"{fn}: joint ids must lie in [0, 65535], got {int(joints.max())}")
        joints = np.ascontiguousarray(joints, dtype=np.uint16).reshape(-1)
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if joints.size != n * 12 or weights.size != n * 12:
            raise ValueError(f"{fn}: joints has {joints.size} and weights {weights.size} elements, the scene needs {n} x 3 x 4 of each")
        tri, norm = _host_geometry(fn, n, tri, norm)
        n_morph = 0
        if morph is not None:
            morph = np.ascontiguousarray(morph, dtype=np.float32).reshape(-1)
            if n == 0 or morph.size % (n * 9):
                raise ValueError(f"{fn}: morph has {morph.size} elements, not n_morph x {n} x 9")
            n_morph = morph.size // (n * 9)
            if n_morph == 0:
                morph = None
        if morph_norm is not None:
            morph_norm = np.ascontiguousarray(morph_norm, dtype=np.float32).reshape(-1)
            if norm is None:
                raise ValueError(f"{fn}: morph_norm needs a rest norm")
            if n_morph == 0 or morph_norm.size != n_morph * n * 27:
                raise ValueError(f"{fn}: morph_norm has {morph_norm.size} elements, {n_morph} morph targets need {n_morph} x {n} x 27")
        if n_joints is None:
            n_joints = int(joints.max()) + 1 if joints.size else 1
        n_joints = int(n_joints)
        if not 1 <= n_joints <= 65535:
            raise ValueError(f"{fn}: n_joints must lie in [1, 65535], got {n_joints}")
        f = lambda a: None if a is None else L.fptr(a)
        d = L.SkinDesc(joints.ctypes.data_as(C.POINTER(C.c_uint16)), L.fptr(weights), n_joints, L.fptr(tri), f(norm), f(morph), f(morph_norm), n_morph)
        return d, (joints, weights, tri, norm, morph, morph_norm)

    @staticmethod
    def _skin_frame(fn, xf, morph_weights, device):
        """(on device, xf, n_joints, morph weights, n_morph, what to keep alive) for update_skin: contiguous float32 numpy
        arrays, or data pointers of float32 torch tensors on `device` (None: device tensors are refused)"""
        on_dev = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in (xf, morph_weights) if a is not None]
        if any(on_dev):
            if device is None or not all(on_dev):
                raise TypeError(f"{fn}: xf and morph_weights must both be device tensors or both host arrays")
            import torch
            for name, a in (("xf", xf), ("morph_weights", morph_weights)):
                if a is None:
                    continue
                if a.dtype != torch.float32 or not a.is_contiguous():
                    raise TypeError(f"{fn}: {name} must be a contiguous float32 tensor")
                if a.device.index != device:
                    raise ValueError(f"{fn}: {name} lives on {a.device}, the scene on device {device}")
            if xf.numel() == 0 or xf.numel() % 12:
                raise ValueError(f"{fn}: xf has {xf.numel()} elements, not n_joints x 12")
            if xf.data_ptr() % 16:
                raise ValueError(f"{fn}: xf must be 16-byte aligned")
            torch.cuda.current_stream(device).synchronize()  # whatever wrote the tensors has finished
            nm = 0 if morph_weights is None else morph_weights.numel()
            return True, C.c_void_p(xf.data_ptr()), xf.numel() // 12, None if not nm else C.c_void_p(morph_weights.data_ptr()), nm, (xf, morph_weights)
        xf = np.ascontiguousarray(xf, dtype=np.float32).reshape(-1)
        if xf.size == 0 or xf.size % 12:
            raise ValueError(f"{fn}: xf has {xf.size} elements, not n_joints x 12")
        mw = None if morph_weights is None else np.ascontiguousarray(morph_weights, dtype=np.float32).reshape(-1)
        nm = 0 if mw is None else mw.size
        return False, L.fptr(xf), xf.size // 12, None if not nm else L.fptr(mw), nm, (xf, mw)

    def set_skin(self, joints, weights=None, tri=None, norm=None, morph=None, morph_norm=None, n_joints=None):
        """Hand the scene a skin (fspt_scene_set_skin).  Per triangle CORNER in the current LEAF order: joints
        [n, 3, 4] ids (< n_joints <= 65535) and weights [n, 3, 4] float32, used as given (not normalised).  tri / norm = the
        rest mesh in that order; the default is the scene's own arrays - tri AND norm of `self.arrays` - refused once
        update_geometry / rebuild_geometry has given the scene other triangles or another order.  With tri given and norm
        None the skin has no rest normals: update_skin then leaves the normal part of the hit records alone.  morph
        [n_morph, n, 9] / morph_norm [n_morph, n, 27]: morph targets as deltas (at most 64; morph_norm needs norm).
        n_joints: the number of joints when it is more than max(joints) + 1.  joints=None drops the skin and frees it.
        Nothing renders differently until update_skin."""
        if joints is None:
            L.check(L.lib().fspt_scene_set_skin(self._h, None))
            return
        if weights is None:
            raise ValueError("set_skin: joints given without weights")
        if tri is None:
            if norm is not None:
                raise ValueError("set_skin: norm given without tri")
            if getattr(self, "_moved", False):
                raise ValueError("set_skin: the scene's geometry is no longer that of its arrays; pass tri (and norm) in the current leaf order")
            tri, norm = self.arrays.tri, self.arrays.norm
        d, keep = self._skin_desc("set_skin", int(self.arrays.n_tris), joints, weights, tri, norm, morph, morph_norm, n_joints)
        L.check(L.lib().fspt_scene_set_skin(self._h, C.byref(d)))

    def update_skin(self, xf, morph_weights=None):
        """One frame of the skin: xf = one 3 x 4 matrix per joint (float32 [n_joints, 12] or [n_joints, 3, 4], row-major as
        update_transforms takes them), morph_weights = one float32 per morph target (None when the skin has none).  A kernel
        applies the morphs, blends each corner's four matrices by its weights, poses the vertex by the blend, tangent and
        bitangent by its 3 x 3 part and the normal by its cofactor matrix (both scaled to the blend's rms), and the tree is
        refitted exactly as update_geometry on those arrays would (fspt_scene_update_skin).  numpy arrays take
        the host form (checked: a non-finite entry is refused naming the joint / target); float32 torch tensors on the
        scene's device are read where they are (the `_device` form; xf 16-byte aligned; no host check - non-finite results
        are refused by the refit's check).  Any error leaves the scene as it was."""
        on_dev, pxf, nj, pmw, nm, keep = self._skin_frame("update_skin", xf, morph_weights, self.device)
        fn = L.lib().fspt_scene_update_skin_device if on_dev else L.lib().fspt_scene_update_skin
        L.check(fn(self._h, pxf, nj, pmw, nm))

    def read_skin(self):
        """(tri [n, 9], norm [n, 27] or None) as the most recent update_skin wrote them (fspt_scene_read_skin)."""
        n = int(self.arrays.n_tris)
        tri = np.zeros((n, 9), np.float32)
        norm = np.zeros((n, 27), np.float32)
        if L.lib().fspt_scene_read_skin(self._h, L.fptr(tri), L.fptr(norm)) == 0:
            return tri, norm
        L.check(L.lib().fspt_scene_read_skin(self._h, L.fptr(tri), None))  # (a skin without rest normals)
        return tri, None

    @property
    def last_skin(self):
        """The most recent update_skin as a dict: skin_ms (k_skin_transform), refit_ms, launches, and bytes - what the skin
        holds on the device by the library's accounting (fspt_scene_last_skin_ms; 0 without a skin)."""
        a, b, n, by = C.c_float(), C.c_float(), C.c_uint32(), C.c_uint64()
        L.check(L.lib().fspt_scene_last_skin_ms(self._h, C.byref(a), C.byref(b), C.byref(n), C.byref(by)))
        return dict(skin_ms=float(a.value), refit_ms=float(b.value), launches=int(n.value), bytes=int(by.value))

    @staticmethod
    def _mesh_desc(fn, arrays, moved, vertex, uv, n_vertices, smooth, rank, static, tri, norm):
        """(fspt_mesh_desc, the arrays it points into) for the triangles of `arrays`; defaults from its meta
        (build_scene(..., keep_order=True, keep_mesh=True)); sizes and types checked here, values by the library"""
        n, meta = int(arrays.n_tris), arrays.meta
        if vertex is None:
            if "tri_vertex" not in meta:
                raise ValueError(f"{fn}: the arrays carry no meta['tri_vertex'] (build_scene(..., keep_order=True, keep_mesh=True)); pass vertex, uv and n_vertices")
            if moved:
                raise ValueError(f"{fn}: the scene's triangles are no longer in the order of its arrays; pass vertex, uv, ... in the current leaf order")
            vertex, uv = meta["tri_vertex"], (meta["tri_uv64"] if uv is None else uv)
            n_vertices = meta["n_vertices"] if n_vertices is None else n_vertices
            smooth = meta["tri_smooth"] if smooth is None else smooth
            rank = meta["tri_order"] if rank is None else rank
            static = meta["tri_static"] if static is None else static
        if uv is None:
            raise ValueError(f"{fn}: vertex given without uv")
        vertex = np.array(_u32_array(vertex, "vertex"), dtype=np.uint32).reshape(-1)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1)
        if vertex.size != n * 3 or uv.size != n * 6:
            raise ValueError(f"{fn}: vertex has {vertex.size} and uv {uv.size} elements, the scene needs {n} x 3 and {n} x 6")
        if static is not None:
            static = np.asarray(static, dtype=bool).reshape(-1)
            if static.size != n:
                raise ValueError(f"{fn}: static has {static.size} elements, the scene has {n} triangles")
            vertex.reshape(-1, 3)[static] = L.MESH_STATIC
        if n_vertices is None:
            live = vertex[vertex != L.MESH_STATIC]
            n_vertices = int(live.max()) + 1 if live.size else 1
        u8 = lambda a, what: None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
        smooth = u8(smooth, "smooth")
        rank = None if rank is None else np.ascontiguousarray(_u32_array(rank, "rank"), dtype=np.uint32).reshape(-1)
        for name, a in (("smooth", smooth), ("rank", rank)):
            if a is not None and a.size != n:
                raise ValueError(f"{fn}: {name} has {a.size} elements, the scene has {n} triangles")
        if (vertex == L.MESH_STATIC).any():
            if tri is None:
                if norm is not None:
                    raise ValueError(f"{fn}: norm given without tri")
                if moved:
                    raise ValueError(f"{fn}: the scene's geometry is no longer that of its arrays; pass the static triangles' rest tri and norm in the current leaf order")
                tri, norm = arrays.tri, arrays.norm
            tri, norm = _host_geometry(fn, n, tri, norm)
            if norm is None:
                raise ValueError(f"{fn}: static triangles need a rest norm")
        else:
            tri = norm = None
        f = lambda a: None if a is None else L.fptr(a)
        d = L.MeshDesc(L.u32ptr(vertex), int(n_vertices), uv.ctypes.data_as(C.POINTER(C.c_double)),
                       None if smooth is None else smooth.ctypes.data_as(C.POINTER(C.c_uint8)), None if rank is None else L.u32ptr(rank), f(tri), f(norm))
        return d, (vertex, uv, smooth, rank, tri, norm)

    @staticmethod
    def _mesh_frame(fn, pos, device):
        """(on device, pos, n_vertices, what to keep alive) for update_vertices: a contiguous float32 numpy array, or the
        data pointer of a float32 torch tensor on `device` (None: device tensors are refused)"""
        if hasattr(pos, "data_ptr") and getattr(pos, "is_cuda", False):
            import torch
            if device is None:
                raise TypeError(f"{fn}: pos must be a host array here")
            if pos.dtype != torch.float32 or not pos.is_contiguous():
                raise TypeError(f"{fn}: pos must be a contiguous float32 tensor")
            if pos.device.index != device:
                raise ValueError(f"{fn}: pos lives on {pos.device}, the scene on device {device}")
            if pos.numel() == 0 or pos.numel() % 3:
                raise ValueError(f"{fn}: pos has {pos.numel()} elements, not n_vertices x 3")
            torch.cuda.current_stream(device).synchronize()  # whatever wrote the tensor has finished
            return True, C.c_void_p(pos.data_ptr()), pos.numel() // 3, pos
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1)
        if pos.size == 0 or pos.size % 3:
            raise ValueError(f"{fn}: pos has {pos.size} elements, not n_vertices x 3")
        return False, L.fptr(pos), pos.size // 3, pos

    def set_mesh(self, vertex=None, uv=None, n_vertices=None, smooth=None, rank=None, static=None, tri=None, norm=None, drop=False):
        """Hand the scene an indexed mesh (fspt_scene_set_mesh).  Per triangle in the current LEAF order: vertex
        [n, 3] indices < n_vertices, uv [n, 6] float64 raw vt values, smooth [n] 0 / 1 (None: all flat), rank [n] the order a
        face normal is summed in (None: the leaf position), static [n] bool: triangles that keep their rest tri / norm (the
        default rest copy is `self.arrays`).  With vertex=None everything comes from the arrays' meta
        (build_scene(..., keep_order=True, keep_mesh=True)) - refused once the scene has been given another order.
        drop=True drops the mesh and frees it.  Nothing renders differently until update_vertices."""
        if drop:
            L.check(L.lib().fspt_scene_set_mesh(self._h, None))
            return
        d, keep = self._mesh_desc("set_mesh", self.arrays, getattr(self, "_moved", False), vertex, uv, n_vertices, smooth, rank, static, tri, norm)
        L.check(L.lib().fspt_scene_set_mesh(self._h, C.byref(d)))

    def update_vertices(self, pos):
        """One frame of the mesh: pos = one float32 position per vertex [n_vertices, 3].  Kernels derive every meshed
        triangle's vertices and normal frames from them by the reference's rules in float64 (face normals, for smooth
        triangles the mean of the incident face normals, calcTangents) and the tree is refitted exactly as
        update_geometry on those arrays would (fspt_scene_update_vertices).  A numpy array takes the host form
        (checked: a non-finite position is refused); a float32 torch tensor on the scene's device is read where it is
        (the `_device` form; no host check - a collapsed face is refused by the refit's check).  Any error leaves the
        scene as it was."""
        on_dev, p, nv, keep = self._mesh_frame("update_vertices", pos, self.device)
        fn = L.lib().fspt_scene_update_vertices_device if on_dev else L.lib().fspt_scene_update_vertices
        L.check(fn(self._h, p, nv))

    def read_mesh(self):
        """(tri [n, 9], norm [n, 27]) as the most recent update_vertices wrote them (fspt_scene_read_mesh)."""
        n = int(self.arrays.n_tris)
        tri = np.zeros((n, 9), np.float32)
        norm = np.zeros((n, 27), np.float32)
        L.check(L.lib().fspt_scene_read_mesh(self._h, L.fptr(tri), L.fptr(norm)))
        return tri, norm

    @property
    def last_mesh(self):
        """The most recent update_vertices as a dict: derive_ms (the derive kernels), refit_ms, launches, and bytes - what
        the mesh holds on the device by the library's accounting (fspt_scene_last_mesh_ms; 0 without a mesh)."""
        a, b, n, by = C.c_float(), C.c_float(), C.c_uint32(), C.c_uint64()
        L.check(L.lib().fspt_scene_last_mesh_ms(self._h, C.byref(a), C.byref(b), C.byref(n), C.byref(by)))
        ps = np.zeros(3, np.float32)
        L.check(L.lib().fspt_scene_last_mesh_pass_ms(self._h, L.fptr(ps)))
        return dict(derive_ms=float(a.value), refit_ms=float(b.value), launches=int(n.value), bytes=int(by.value), pass_ms=[float(x) for x in ps])

    def _materials_args(self, fn, mat, uv, atlas, atlas_res, atlas_layers):
        n = int(self.arrays.n_tris)
        mat = np.ascontiguousarray(mat, dtype=np.float32)
        if mat.size != n * 12:
            raise ValueError(f"{fn}: mat has {mat.size} elements, the scene needs {n} x 12")
        if uv is not None:
            uv = np.ascontiguousarray(uv, dtype=np.float32)
            if uv.size != n * 6:
                raise ValueError(f"{fn}: uv has {uv.size} elements, the scene needs {n} x 6")
        res = layers = 0
        if atlas is not None:
            atlas = np.ascontiguousarray(atlas, dtype=np.uint8)
            if atlas_res is None or atlas_layers is None:
                raise ValueError(f"{fn}: an atlas needs atlas_res and atlas_layers")
            res, layers = int(atlas_res), int(atlas_layers)
            if res < 0 or layers < 0 or atlas.size != res * res * layers * 4:
                raise ValueError(f"{fn}: atlas has {atlas.size} bytes, {res} x {res} x {layers} RGBA8 texels need {res * res * layers * 4}")
        return (L.fptr(mat), None if uv is None else L.fptr(uv), None if atlas is None else L.u8ptr(atlas), res, layers), (mat, uv, atlas)

    def update_materials(self, mat, uv=None, atlas=None, atlas_res=None, atlas_layers=None):
        """New matTex records (12 floats per triangle) and, unless None, uvs (6 per triangle) in the scene's current LEAF
        order, and a new atlas (RGBA8, atlas_res^2 * atlas_layers texels; any resolution and layer count) - or None: the atlas
        of this scene's most recent update_materials call that carried one.  The texture sets, the tiled and interleaved
        images and the material part of the hit records are laid out again on the GPU; afterwards the scene renders bit for
        bit like a Scene created from the same arrays (fspt_scene_update_materials).  Tracers stay valid and
        keep their accumulators, histories and exposure; `self.arrays` is not touched."""
        args, keep = self._materials_args("update_materials", mat, uv, atlas, atlas_res, atlas_layers)
        L.check(L.lib().fspt_scene_update_materials(self._h, *args))
        if atlas is not None:
            self._retained_atlas_res = args[3]  # (patch_textures' resolution)

    def _textures_mat_uv(self, fn, mat, uv):
        n = int(self.arrays.n_tris)
        mat = np.ascontiguousarray(mat, dtype=np.float32)
        if mat.size != n * 12:
            raise ValueError(f"{fn}: mat has {mat.size} elements, the scene needs {n} x 12")
        if uv is not None:
            uv = np.ascontiguousarray(uv, dtype=np.float32)
            if uv.size != n * 6:
                raise ValueError(f"{fn}: uv has {uv.size} elements, the scene needs {n} x 6")
        return mat, uv

    @staticmethod
    def _patch_args(fn, layer_ids, layers, images, device):
        from . import scene as S
        ids = np.ascontiguousarray(_u32_array(layer_ids, "layer_ids"), dtype=np.uint32).reshape(-1)
        layers = list(layers)
        if ids.size != len(layers):
            raise ValueError(f"{fn}: {ids.size} layer ids for {len(layers)} layers")
        return ids, layers, list(images or [])

    def update_textures(self, mat, uv, packer_or_desc):
        """update_materials with the atlas made on the GPU (fspt_scene_update_textures): packer_or_desc is a
        scene.TexturePacker or its pack_desc() - the decoded sources (numpy arrays, or uint8 torch tensors [h, w, 4] on the
        scene's device, read in place) and the layer list.  Only the sources cross the bus; the kernel resamples them into a
        new raw atlas, and from there on the call is update_materials carrying that atlas: same layouts, same retained
        atlas, same effect on tracers."""
        from . import scene as S
        mat, uv = self._textures_mat_uv("update_textures", mat, uv)
        p, on_dev, _, keep = S.texture_pack_struct(packer_or_desc, getattr(self, "device", None), "update_textures")
        fn = L.lib().fspt_scene_update_textures_device if on_dev else L.lib().fspt_scene_update_textures
        L.check(fn(self._h, L.fptr(mat), None if uv is None else L.fptr(uv), C.byref(p)))
        self._retained_atlas_res = int(p.res)

    def patch_textures(self, layer_ids, layers, images=None, res=None):
        """Replace layers of the retained raw atlas (the one the last update_materials / update_textures call carried) and lay
        the scene out again with its current materials (fspt_scene_patch_textures): layers[k] - a layer dict
        of TexturePacker.pack_desc() whose "image" indexes `images` - becomes layer layer_ids[k]; the resolution is the
        retained atlas's (res=None: what this object's last update_materials / update_textures sent).  images: numpy arrays or
        device tensors as for update_textures.  Without a retained atlas the library refuses (FSPT_E_STATE)."""
        from . import scene as S
        ids, layers, images = self._patch_args("patch_textures", layer_ids, layers, images, getattr(self, "device", None))
        res = int(res) if res is not None else getattr(self, "_retained_atlas_res", None) or 1
        p, on_dev, _, keep = S.texture_pack_struct({"res": res, "images": images, "layers": layers}, getattr(self, "device", None), "patch_textures")
        fn = L.lib().fspt_scene_patch_textures_device if on_dev else L.lib().fspt_scene_patch_textures
        L.check(fn(self._h, L.u32ptr(ids), ids.size, C.byref(p)))

    @staticmethod
    def _environment_args(fn, env, env_w, env_h, bins):
        if bins is None:
            raise ValueError(f"{fn}: bins are required (scene.env_bins)")
        bins = np.ascontiguousarray(_u32_array(bins, "bins"), dtype=np.uint32)
        if bins.size % 4:
            raise ValueError(f"{fn}: bins has {bins.size} elements, not a multiple of 4")
        w = h = 0
        if env is not None:
            env = np.ascontiguousarray(env, dtype=np.uint8)
            w, h = int(env_w), int(env_h)
            if w < 0 or h < 0 or env.size != w * h * 4:
                raise ValueError(f"{fn}: env has {env.size} bytes, {w} x {h} RGBE texels need {w * h * 4}")
        return (None if env is None else L.u8ptr(env), w, h, L.u32ptr(bins), bins.size // 4), (env, bins)

    @staticmethod
    def _environment_auto_args(fn, env, env_w, env_h, device):
        """(on device, pointer, w, h, keep) of an environment whose bins the GPU builds: host RGBE bytes, or - `device` not
        None - a contiguous uint8 tensor on that device"""
        w, h = int(env_w), int(env_h)
        if env is None:
            raise ValueError(f"{fn}: bins are required (scene.env_bins) when there is no map to build them from")
        if not (0 <= w < 2 ** 32 and 0 <= h < 2 ** 32):
            raise ValueError(f"{fn}: {w} x {h} is not a map size")
        if hasattr(env, "data_ptr") and getattr(env, "is_cuda", False):
            import torch
            if device is None:
                raise TypeError(f"{fn}: a device tensor needs a single scene; this host takes host arrays")
            if env.dtype != torch.uint8 or not env.is_contiguous():
                raise TypeError(f"{fn}: env must be a contiguous uint8 tensor")
            if env.device.index != device:
                raise ValueError(f"{fn}: env lives on {env.device}, the scene on device {device}")
            if env.numel() != w * h * 4:
                raise ValueError(f"{fn}: env has {env.numel()} bytes, {w} x {h} RGBE texels need {w * h * 4}")
            torch.cuda.current_stream(device).synchronize()  # whatever wrote the tensor has finished
            return True, C.c_void_p(env.data_ptr()), w, h, env
        env = np.ascontiguousarray(env, dtype=np.uint8)
        if env.size != w * h * 4:
            raise ValueError(f"{fn}: env has {env.size} bytes, {w} x {h} RGBE texels need {w * h * 4}")
        return False, L.u8ptr(env), w, h, env

    def update_environment(self, env, env_w, env_h, bins=None):
        """A new environment map (RGBE in RGBA8, env_w * env_h texels; None = black) and its importance bins (scene.env_bins),
        tiled on the GPU (fspt_scene_update_environment); everything else as update_materials.  bins=None: the
        bins are built on the GPU from the uploaded map (fspt_scene_update_environment_auto), and `env` may be a
        uint8 torch tensor on the scene's device, which is then read in place (fspt_scene_update_environment_device)."""
        if bins is None:
            on_dev, ptr, w, h, keep = self._environment_auto_args("update_environment", env, env_w, env_h, getattr(self, "device", None))
            fn = L.lib().fspt_scene_update_environment_device if on_dev else L.lib().fspt_scene_update_environment_auto
            L.check(fn(self._h, ptr, w, h))
            return
        args, keep = self._environment_args("update_environment", env, env_w, env_h, bins)
        L.check(L.lib().fspt_scene_update_environment(self._h, *args))

    def update_sky(self, sun_dir, width=1024, height=512, **params):
        """Replace the environment by a generated sky (scene.sky's model and parameters) of width x height texels: generated,
        encoded, binned and tiled on the GPU, no texel crosses the bus (fspt_scene_update_sky).  Afterwards the
        scene renders bit for bit like one created from scene.sky's bytes and scene.env_bins of them; everything else as
        update_materials."""
        from . import scene as S
        p = S.sky_params(sun_dir, **params)
        L.check(L.lib().fspt_scene_update_sky(self._h, C.byref(p), _map_side("update_sky", width), _map_side("update_sky", height)))

    def last_sky(self):
        """The most recent update_sky / update_environment(bins=None) as a dict: sky_ms, bins_ms, tile_ms (GPU, HIP events;
        bins_ms includes the read-back of n_bins), launches, readbacks, n_bins (fspt_scene_last_sky_ms)."""
        a, b, c, nl, nr, nb = C.c_float(), C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.check(L.lib().fspt_scene_last_sky_ms(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(nl), C.byref(nr), C.byref(nb)))
        return dict(sky_ms=float(a.value), bins_ms=float(b.value), tile_ms=float(c.value), launches=int(nl.value),
                    readbacks=int(nr.value), n_bins=int(nb.value))

    APPEARANCE = ("tex_sets", "atlas", "atlas4", "env", "bins", "hitrec")  # read_appearance's `what`

    def read_appearance(self, what):
        """The bytes of one of the buffers an appearance update writes, as the device holds them (uint8;
        fspt_scene_read_appearance): 0 texture-set table, 1 single-layer tiled images, 2 interleaved images, 3 environment
        tiles, 4 bins, 5 hit records - or its name in Scene.APPEARANCE."""
        what = self.APPEARANCE.index(what) if isinstance(what, str) else int(what)
        n = C.c_uint64()
        L.check(L.lib().fspt_scene_read_appearance(self._h, what, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if out.size:
            L.check(L.lib().fspt_scene_read_appearance(self._h, what, C.c_void_p(out.ctypes.data), out.size, C.byref(n)))
        return out

    def last_appearance(self):
        """The most recent update_materials / update_environment as a dict: ms (GPU, first kernel to last), launches,
        uploaded (bytes), retained (bytes of the raw atlas kept on the device; 0 for a scene never updated)."""
        ms, nl, up, rt = C.c_float(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().fspt_scene_last_appearance_ms(self._h, C.byref(ms), C.byref(nl), C.byref(up), C.byref(rt)))
        return dict(ms=float(ms.value), launches=int(nl.value), uploaded=int(up.value), retained=int(rt.value))

    def last_rebuild_ms(self):
        """The most recent rebuild_geometry as a dict: build_ms (GPU, the build kernels), install_ms (GPU, gather + refit),
        host_ms (the numbering), launches, readbacks (fspt_scene_last_rebuild_ms)."""
        b, i, h, nl, nr = C.c_float(), C.c_float(), C.c_float(), C.c_uint32(), C.c_uint32()
        L.check(L.lib().fspt_scene_last_rebuild_ms(self._h, C.byref(b), C.byref(i), C.byref(h), C.byref(nl), C.byref(nr)))
        return dict(build_ms=float(b.value), install_ms=float(i.value), host_ms=float(h.value), launches=int(nl.value),
                    readbacks=int(nr.value))

    def sah_cost(self):
        """SAH cost of the tree with the boxes the device holds now, relative to the root's area (fspt_scene_sah_cost): what
        tools/bvh_build_bench.py prints for a built tree; grows as a refitted tree degrades."""
        c = C.c_double()
        L.check(L.lib().fspt_scene_sah_cost(self._h, C.byref(c)))
        return float(c.value)

    def slot_triangles(self):
        """uint32 [n_slots]: the triangle (current leaf order) every leaf slot holds (fspt_scene_slot_triangles); values
        >= n_tris mark empty slots.  What temporal_gbuffer's slot numbers index."""
        n = C.c_uint32()
        L.check(L.lib().fspt_scene_slot_triangles(self._h, C.byref(n), None))
        out = np.zeros(n.value, np.uint32)
        L.check(L.lib().fspt_scene_slot_triangles(self._h, None, L.u32ptr(out)))
        return out

    def motion_begin(self):
        """Motion origin (fspt_scene_motion_begin): snapshot every triangle as it is now; what update_geometry moves
        until the next temporal_accumulate is reprojected from there.  rebuild_geometry keeps the snapshot's slots in step."""
        L.check(L.lib().fspt_scene_motion_begin(self._h))

    def motion_end(self):
        """Drop the motion origin: temporal_accumulate treats the scene as static again (fspt_scene_motion_end)."""
        L.check(L.lib().fspt_scene_motion_end(self._h))

    def last_update_ms(self):
        """(GPU ms first kernel to last, kernels launched) of the most recent update_geometry."""
        ms, n = C.c_float(), C.c_uint32()
        L.check(L.lib().fspt_scene_last_update_ms(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def close(self):
        if self._h:
            L.lib().fspt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PathTracer:
    NUM_BOUNCES = 4  # tracer.fs:9

    def __init__(self, scene, width, height, device=0, num_bounces=None):
        self.scene = scene if isinstance(scene, Scene) else Scene(scene, device)
        self.resolution = (int(width), int(height))
        self._t = C.c_void_p()
        L.check(L.lib().fspt_target_create(self.scene._h, self.resolution[0], self.resolution[1], C.byref(self._t)))
        # main.js:67-74 defaults
        self.fovScale = 0.5
        self.envTheta = 0.0
        self.dir = [0.0, 0.0, -1.0]
        self.eye = [0.0, 0.0, 2.0]
        self.lensFeatures = [1.0 - 1.0 / 2.0, 0.02]
        self.num_bounces = self.NUM_BOUNCES if num_bounces is None else int(num_bounces)
        self.pingpong = 0
        self._rng = C.c_uint64(1)
        self._keep = None
        self._rays_keep = []  # set_rays_device's tensors, held until this tracer's stream has been synchronised
        self._tile = 32  # set_shard's tile (adaptive_stats)

    # ---- configuration -----------------------------------------------------
    def set_camera(self, P, I, fov_scale=0.5, env_theta=0.0, focal_depth=2.0, aperture=0.02, **_):
        self.eye = [float(x) for x in P]
        self.dir = [float(x) for x in I]
        self.fovScale = float(fov_scale)
        self.envTheta = float(env_theta)
        self.lensFeatures = [1.0 - 1.0 / float(focal_depth), float(aperture)]

    def seed(self, s):
        """Seed of the host PRNG that replaces Math.random()*10000 (main.js:748,777)."""
        if int(s) == 0:
            raise ValueError("xorshift seed must be non-zero")
        self._rng = C.c_uint64(int(s))

    def next_rand_base(self):
        return float(L.lib().fspt_rand_base_next(C.byref(self._rng)))

    def set_shard(self, shard, n_shards, tile=32):
        L.check(L.lib().fspt_target_set_shard(self._t, shard, n_shards, tile))
        self._tile = int(tile)

    def set_viewport(self, w=0, h=0):
        """gl.viewport(0, 0, w, h) of drawCamera / drawTracer (main.js:744,761); 0, 0 = the whole target.  The
        reference uses resolution * 0.25 while the camera moves (resScale, main.js:840)."""
        L.check(L.lib().fspt_target_set_viewport(self._t, int(w), int(h)))

    def set_sampler(self, kind="sobol", seed=0):
        """The paths' random numbers (fspt_target_set_sampler): "reference" (the default: rnd(), bit for bit)
        or "sobol" (Owen-scrambled Sobol, seeded by `seed`; rand_base values then no longer affect radiance).  Runs the
        recorded ticks first; does not clear the accumulator."""
        if kind not in SAMPLERS:
            raise ValueError("sampler must be one of %s, got %r" % (sorted(SAMPLERS), kind))
        L.check(L.lib().fspt_target_set_sampler(self._t, SAMPLERS[kind], _sampler_seed(seed)))

    def set_camera_model(self, model="pinhole", angle=None, ipd=None):
        """The camera model (fspt_target_set_camera_model): "pinhole" (the default, or None), "ortho", "fisheye"
        (angle: the full field of view over the frame height in radians, in (0, 2 pi], default pi), "equirect" or "stereo"
        (over-under, the upper half is the left eye; ipd in scene units, >= 0, default 0.064; the height must be even).
        Runs the recorded ticks first; does not clear the accumulator."""
        L.check(L.lib().fspt_target_set_camera_model(self._t, camera_model_params(model, angle, ipd)))

    @property
    def camera_model(self):
        """{"model", "angle", "ipd"} of fspt_target_get_camera_model."""
        p = L.CameraModelParams()
        L.check(L.lib().fspt_target_get_camera_model(self._t, C.byref(p)))
        return {"model": {v: n for n, v in CAMERA_MODELS.items()}[p.model], "angle": float(p.angle), "ipd": float(p.ipd)}

    def set_lights(self, mode="emitters", emitter_fraction=0.5):
        """Next-event estimation of emissive triangles (fspt_target_set_lights): "emitters" lets a shading
        vertex spend its shadow ray on an emitter with probability emitter_fraction (1 when the scene has no environment
        map), MIS-weighted; "off" (the default) is the reference bit for bit.  emitter_fraction in (0, 1].  Runs the
        recorded ticks first; does not clear the accumulator."""
        if mode not in LIGHTS:
            raise ValueError("lights mode must be one of %s, got %r" % (sorted(LIGHTS), mode))
        if isinstance(emitter_fraction, bool) or not isinstance(emitter_fraction, (int, float, np.integer, np.floating)):
            raise TypeError("emitter_fraction must be a number, got %r" % (emitter_fraction,))
        f = float(emitter_fraction)
        if not 0.0 < f <= 1.0:
            raise ValueError("emitter_fraction must lie in (0, 1], got %r" % (emitter_fraction,))
        L.check(L.lib().fspt_target_set_lights(self._t, LIGHTS[mode], f))

    def get_lights(self):
        """(mode, emitter_fraction) of fspt_target_get_lights."""
        m, f = C.c_int(), C.c_float()
        L.check(L.lib().fspt_target_get_lights(self._t, C.byref(m), C.byref(f)))
        return {v: n for n, v in LIGHTS.items()}[m.value], float(f.value)

    def get_sampler(self):
        """(kind, seed) of fspt_target_get_sampler."""
        k, s = C.c_int(), C.c_uint32()
        L.check(L.lib().fspt_target_get_sampler(self._t, C.byref(k), C.byref(s)))
        return {v: n for n, v in SAMPLERS.items()}[k.value], int(s.value)

    def bind_accumulator(self, device_ptr, keep=None):
        """Accumulate into caller-owned device memory (e.g. a torch tensor) so a
        collective can run on it in place; `keep` is held to keep it alive."""
        self._keep = keep
        L.check(L.lib().fspt_target_bind_accumulator(self._t, C.c_void_p(device_ptr)))
        self.bound_ptr = int(device_ptr)  # what pack_tiles / unpack_tiles read and write (distributed.TileGather checks it)

    # ---- the two ends of a one-process-per-GPU read-out exchange (include/fspt.h) -----------------------------
    def shard_slots(self, shard, n_shards):
        """Entries of shard `shard`'s packed pixel array: owned tiles x tile^2."""
        n = C.c_uint64()
        L.check(L.lib().fspt_target_shard_slots(self._t, int(shard), int(n_shards), C.byref(n)))
        return int(n.value)

    def pack_tiles(self, packed_ptr, channels=4):
        """This target's own pixels -> packed[slots][channels] (device pointer).  Blocking."""
        L.check(L.lib().fspt_target_pack_tiles(self._t, C.c_void_p(packed_ptr), int(channels)))

    def unpack_tiles(self, packed_ptr, shard, n_shards, channels=4):
        """Packed pixels of shard `shard` of `n_shards` -> the accumulator (channels 3: alpha = 1).  Blocking."""
        L.check(L.lib().fspt_target_unpack_tiles(self._t, C.c_void_p(packed_ptr), int(shard), int(n_shards), int(channels)))

    def set_pipeline(self, pipeline, batch_ticks=0):
        """'wavefront' (batches), 'stream' (fixed pool of live paths) or 'megakernel'; results are bit-identical
        (include/fspt_tuning.h)."""
        code = PIPELINES.get(pipeline, pipeline)
        L.check(L.lib().fspt_target_set_pipeline(self._t, int(code), int(batch_ticks)))

    def set_pool(self, paths=0, drain=-1, max_iterations=0, overlap=-1):
        """Stream scheduler: live paths per state set (0 = default), drain iterations (-1 = default), iteration cap
        (0 = none; test hook), second HIP stream for plan / primary / resolve (-1 = default).  include/fspt_tuning.h:
        fspt_target_set_pool."""
        L.check(L.lib().fspt_target_set_pool(self._t, int(paths), int(drain), int(max_iterations), int(overlap)))

    def set_primary_form(self, form=0):
        """k_wf_primary's traversal phase: 1 one ray per lane, 2 per-lane refill, 0 (default) measured and chosen by the
        library per batch size (include/fspt_tuning.h)."""
        L.check(L.lib().fspt_target_set_primary_form(self._t, int(form)))

    def primary_form(self, batch_ticks):
        """(form the next batch of that size uses, [ms per sample of form 1, form 2] measured so far or -1)."""
        f = C.c_int()
        ms = (C.c_double * 2)()
        L.check(L.lib().fspt_target_get_primary_form(self._t, int(batch_ticks), C.byref(f), ms))
        return int(f.value), [float(ms[0]), float(ms[1])]

    def set_node_form(self, primary=-1, trace=-1, tail=-1, trace_below=-1):
        """Node form per kernel class: -1 the library's choice, 0 the 64-byte nodes, 1 the two-level nodes (two traversal
        steps per memory round trip; bit-identical results); tail also 2 = adaptive (two-level once a wave's list is used up).  trace_below: the library's choice for a trace launch is
        two-level when it expects fewer paths than this (include/fspt_tuning.h)."""
        L.check(L.lib().fspt_target_set_node_form(self._t, int(primary), int(trace), int(tail), int(trace_below)))

    def set_trace_budget(self, steps):
        """Traversal steps a starved trace wave walks on before it suspends its rays (0 = never; include/fspt_tuning.h)."""
        L.check(L.lib().fspt_target_set_trace_budget(self._t, int(steps)))

    def prepare(self):
        """Allocate the pipeline's path-state buffers now (not lazily inside the first render)."""
        L.check(L.lib().fspt_target_prepare(self._t))

    def set_memory_limit(self, nbytes):
        """Cap the wavefront path state of this target (bytes, 0 = none); a batch that does not fit is halved."""
        L.check(L.lib().fspt_target_set_memory_limit(self._t, int(nbytes)))

    def path_state_bytes(self):
        """(bytes of path state currently allocated, batch size in use)."""
        b = C.c_uint64(); n = C.c_uint32()
        L.check(L.lib().fspt_target_path_state_bytes(self._t, C.byref(b), C.byref(n)))
        return b.value, n.value

    def set_stage_timing(self, on=True):
        """HIP event pairs around every launch (what last_stage_ms reads); off: ~1.3 % faster 20-tick regions, zeros there."""
        L.check(L.lib().fspt_target_set_stage_timing(self._t, 1 if on else 0))

    def last_stage_ms(self):
        ms = (C.c_float * 5)(); n = (C.c_uint32 * 5)()
        L.check(L.lib().fspt_last_stage_ms(self._t, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(("primary", "trace", "logic", "resolve", "tail"))}

    def set_deferred(self, on=True):
        """Two-call ticks (drawCamera + drawTracer) are recorded and run in batches at the next read-out (default);
        False: every drawTracer executes at once."""
        L.check(L.lib().fspt_target_set_deferred(self._t, 1 if on else 0))

    def live_paths(self, n_rounds=12):
        """Fraction of the batch's samples still alive after round r (index r; r = 1 is the primary launch)."""
        f = (C.c_double * n_rounds)()
        L.check(L.lib().fspt_target_live_paths(self._t, f, n_rounds))
        return list(f)

    def set_tail(self, round=-1):
        """-1: adaptive (default), 0: never, r >= 1: the tail kernel takes over after wavefront round r."""
        L.check(L.lib().fspt_target_set_tail(self._t, int(round)))

    def enable_counters(self, on=True):
        """0 / False: off.  1 / True: count the reference algorithm's work (equals the oracle's counters).
        2: count what the production kernels really do (NEE shadow rays stop at the first hit)."""
        L.check(L.lib().fspt_enable_counters(self._t, int(on)))

    # ---- the reference's draw calls ------------------------------------------
    def drawCamera(self, randBase):
        P = (C.c_float * 3)(*self.eye); I = (C.c_float * 3)(*self.dir); lens = (C.c_float * 2)(*self.lensFeatures)
        L.check(L.lib().fspt_camera(self._t, P, I, self.fovScale, lens, float(randBase)))

    def drawTracer(self, i, randBase):
        L.check(L.lib().fspt_trace(self._t, int(i), float(randBase), self.envTheta, self.num_bounces))

    def drawTracerTest(self, i):
        """drawTracer with bvh_test.fs (`mode=test`, main.js:879-883): traversal-step heat map."""
        L.check(L.lib().fspt_trace_test(self._t, int(i)))

    def tick(self):
        """One iteration of main.js:838-857 (camera draw, trace draw, pingpong++)."""
        self.drawCamera(self.next_rand_base())
        self.drawTracer(self.pingpong, self.next_rand_base())
        self.pingpong += 1

    def render(self, n_ticks):
        """n_ticks fused ticks (ray generation inside the path kernel), same
        randBase stream and results as n_ticks x tick()."""
        cp = L.CameraParams()
        cp.P = (C.c_float * 3)(*self.eye); cp.I = (C.c_float * 3)(*self.dir)
        cp.fov_scale = self.fovScale; cp.lens = (C.c_float * 2)(*self.lensFeatures)
        cp.env_theta = self.envTheta; cp.num_bounces = self.num_bounces
        L.check(L.lib().fspt_render(self._t, C.byref(cp), self.pingpong, int(n_ticks), self._rng.value))
        for _ in range(2 * int(n_ticks)):  # advance the host stream like the kernel did
            self.next_rand_base()
        self.pingpong += int(n_ticks)

    def _camera_params(self):
        cp = L.CameraParams()
        cp.P = (C.c_float * 3)(*self.eye); cp.I = (C.c_float * 3)(*self.dir)
        cp.fov_scale = self.fovScale; cp.lens = (C.c_float * 2)(*self.lensFeatures)
        cp.env_theta = self.envTheta; cp.num_bounces = self.num_bounces
        return cp

    def render_adaptive(self, target_rel_mse, max_ticks=1024, min_ticks=64, round_ticks=32):
        """Adaptive sampling (fspt_render_adaptive): clear, then rounds of round_ticks ticks over the tiles whose
        estimated relative MSE is still >= target_rel_mse (each tile at least min_ticks, at most max_ticks ticks).  A tile
        retired after n ticks holds render(n)'s pixels of a cleared tracer bit for bit.  Returns the largest count run;
        pingpong and the host randBase stream then stand where render(that count) after clear() leaves them."""
        for name, v in (("max_ticks", max_ticks), ("min_ticks", min_ticks), ("round_ticks", round_ticks)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"render_adaptive: {name} must be an int")
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"render_adaptive: {name} out of range")
        if isinstance(target_rel_mse, bool) or not isinstance(target_rel_mse, (int, float, np.floating, np.integer)):
            raise TypeError("render_adaptive: target_rel_mse must be a number")
        if not (np.isfinite(target_rel_mse) and target_rel_mse >= 0):
            raise ValueError("render_adaptive: target_rel_mse must be finite and >= 0")
        prm = L.AdaptiveParams(float(target_rel_mse), int(max_ticks), int(min_ticks), int(round_ticks))
        L.check(L.lib().fspt_render_adaptive(self._t, C.byref(self._camera_params()), C.byref(prm), self._rng.value))
        rounds = C.c_uint32()
        L.check(L.lib().fspt_adaptive_last_stats(self._t, C.byref(rounds), None, None, None, 0))
        n = int(rounds.value) * int(round_ticks)
        for _ in range(2 * n):  # the host stream advances like fspt_render's for the largest count
            self.next_rand_base()
        self.pingpong = n
        return n

    def sample_counts(self):
        """The last render_adaptive()'s ticks per pixel: uint32 [H, W], row 0 = bottom, 0 outside its viewport."""
        W, H = self.resolution
        out = np.zeros((H, W), np.uint32)
        L.check(L.lib().fspt_read_sample_counts(self._t, L.u32ptr(out)))
        return out

    def adaptive_stats(self):
        """The last render_adaptive(): {"rounds", "samples", "tile_ticks" [tiles_y, tiles_x] uint32, "tile_err" (the E_T that
        retired each tile) float64}, tiles row-major from the bottom row (fspt_adaptive_last_stats)."""
        W, H = self.resolution
        tile = self._tile
        tx, ty = (W + tile - 1) // tile, (H + tile - 1) // tile
        rounds, samples = C.c_uint32(), C.c_uint64()
        ticks = np.zeros((ty, tx), np.uint32); err = np.zeros((ty, tx), np.float64)
        L.check(L.lib().fspt_adaptive_last_stats(self._t, C.byref(rounds), C.byref(samples), err.ctypes.data_as(C.POINTER(C.c_double)),
                                                 L.u32ptr(ticks), tx * ty))
        return {"rounds": int(rounds.value), "samples": int(samples.value), "tile_ticks": ticks, "tile_err": err}

    def update_geometry(self, tri, norm=None):
        """Scene.update_geometry on this tracer's scene (every tracer of the scene sees it); call clear() to restart the mean."""
        self.scene.update_geometry(tri, norm)

    def set_pose(self, part, tri=None, norm=None):
        """Scene.set_pose on this tracer's scene."""
        self.scene.set_pose(part, tri, norm)

    def update_transforms(self, xf):
        """Scene.update_transforms on this tracer's scene (every tracer of the scene sees it); call clear() to restart the mean."""
        self.scene.update_transforms(xf)

    def set_skin(self, joints, weights=None, tri=None, norm=None, morph=None, morph_norm=None, n_joints=None):
        """Scene.set_skin on this tracer's scene."""
        self.scene.set_skin(joints, weights, tri, norm, morph, morph_norm, n_joints)

    def update_skin(self, xf, morph_weights=None):
        """Scene.update_skin on this tracer's scene (every tracer of the scene sees it); call clear() to restart the mean."""
        self.scene.update_skin(xf, morph_weights)

    def read_skin(self):
        """Scene.read_skin of this tracer's scene."""
        return self.scene.read_skin()

    @property
    def last_skin(self):
        """Scene.last_skin of this tracer's scene."""
        return self.scene.last_skin

    def set_mesh(self, *args, **kwargs):
        """Scene.set_mesh on this tracer's scene."""
        self.scene.set_mesh(*args, **kwargs)

    def update_vertices(self, pos):
        """Scene.update_vertices on this tracer's scene (every tracer of the scene sees it); call clear() to restart the mean."""
        self.scene.update_vertices(pos)

    def read_mesh(self):
        """Scene.read_mesh of this tracer's scene."""
        return self.scene.read_mesh()

    @property
    def last_mesh(self):
        """Scene.last_mesh of this tracer's scene."""
        return self.scene.last_mesh

    def update_materials(self, mat, uv=None, atlas=None, atlas_res=None, atlas_layers=None):
        """Scene.update_materials on this tracer's scene (every tracer of the scene sees it); the accumulator, the temporal
        history, the exposure and the bloom state stay - call clear() to restart the mean."""
        self.scene.update_materials(mat, uv, atlas, atlas_res, atlas_layers)

    def update_textures(self, mat, uv, packer_or_desc):
        """Scene.update_textures on this tracer's scene; state stays as for update_materials."""
        self.scene.update_textures(mat, uv, packer_or_desc)

    def patch_textures(self, layer_ids, layers, images=None, res=None):
        """Scene.patch_textures on this tracer's scene; state stays as for update_materials."""
        self.scene.patch_textures(layer_ids, layers, images, res)

    def update_environment(self, env, env_w, env_h, bins=None):
        """Scene.update_environment on this tracer's scene (bins=None: built on the GPU); state stays as for update_materials."""
        self.scene.update_environment(env, env_w, env_h, bins)

    def update_sky(self, sun_dir, width=1024, height=512, **params):
        """Scene.update_sky on this tracer's scene; state stays as for update_materials."""
        self.scene.update_sky(sun_dir, width, height, **params)

    def last_sky(self):
        """Scene.last_sky of this tracer's scene"""
        return self.scene.last_sky()

    def rebuild_geometry(self, tri, norm=None):
        """Scene.rebuild_geometry on this tracer's scene: a new tree in place; returns the new leaf order."""
        return self.scene.rebuild_geometry(tri, norm)

    def clear(self):
        L.check(L.lib().fspt_clear(self._t))
        self.pingpong = 0
        L.check(L.lib().fspt_counters_reset(self._t))

    def sync(self):
        L.check(L.lib().fspt_sync(self._t))
        self._rays_keep = []

    # ---- read-back -------------------------------------------------------------
    def setRays(self, pos, dir):
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1)
        dir = np.ascontiguousarray(dir, dtype=np.float32).reshape(-1)
        n = self.resolution[0] * self.resolution[1] * 4
        if pos.size != n or dir.size != n:
            raise ValueError("ray buffers must be W*H*4 floats")
        L.check(L.lib().fspt_set_rays(self._t, L.fptr(pos), L.fptr(dir)))

    def set_rays_device(self, pos, dir):
        """setRays with torch tensors on the tracer's device (fspt_set_rays_device): float32, contiguous, W*H*4 elements
        each; copied on the tracer's stream without a host synchronisation.  The tensors' producer must have finished
        (e.g. torch.cuda.synchronize()) before the call, and their memory must stay unmodified until the copy has run: the
        tracer holds a reference to both until its next sync() or readRadiance(), so that dropping them is safe; writing
        new rays into the SAME tensors needs a sync() first."""
        n = self.resolution[0] * self.resolution[1] * 4
        for name, a in (("pos", pos), ("dir", dir)):
            if not (hasattr(a, "data_ptr") and hasattr(a, "is_cuda")):
                raise TypeError(f"set_rays_device: {name} must be a torch tensor")
            if not a.is_cuda or a.device.index != self.scene.device:
                raise ValueError(f"set_rays_device: {name} must live on device {self.scene.device}, got {a.device}")
            if str(a.dtype) != "torch.float32" or not a.is_contiguous() or a.numel() != n:
                raise ValueError(f"set_rays_device: {name} must be a contiguous float32 tensor of W*H*4 elements")
        L.check(L.lib().fspt_set_rays_device(self._t, C.c_void_p(pos.data_ptr()), C.c_void_p(dir.data_ptr())))
        self._rays_keep.append((pos, dir))

    def readRays(self):
        W, H = self.resolution
        pos = np.zeros((H, W, 4), np.float32); d = np.zeros((H, W, 4), np.float32)
        L.check(L.lib().fspt_read_rays(self._t, L.fptr(pos), L.fptr(d)))
        return pos, d

    def readRadiance(self):
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32)
        L.check(L.lib().fspt_read_radiance(self._t, L.fptr(out)))
        self._rays_keep = []  # (the read waited for the stream)
        return out

    def draw(self, exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0, scale=1.0):
        """drawQuad (main.js:809-824) / draw.fs: tonemapped RGBA8 [H, W, 4], row 0 = bottom.  scale = draw.fs's
        `scale` uniform (resScale: 0.25 while the camera moves, main.js:819,840)."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.uint8)
        L.check(L.lib().fspt_draw_scaled(self._t, float(exposure), float(saturation), 1 if denoise else 0,
                                         float(max_sigma), float(scale), L.u8ptr(out)))
        return out

    def present(self, exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0, scale=1.0, out=None):
        """drawQuad inside tick() (main.js:838-857), pipelined with one frame of latency (fspt_present): enqueues
        the ticks recorded since the last call and their frame, and returns (the PREVIOUS call's frame, its sample count =
        1 + its newest tick index).  (None, 0) when there is nothing to present yet (first call after any other call on
        this tracer but tick()).  `out`: an optional uint8 [H, W, 4] array the frame is written to."""
        W, H = self.resolution
        if out is None:
            out = np.zeros((H, W, 4), np.uint8)
        elif out.dtype != np.uint8 or out.size != W * H * 4 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint8 array of W*H*4 elements")
        ticks = C.c_uint32()
        L.check(L.lib().fspt_present(self._t, float(exposure), float(saturation), 1 if denoise else 0,
                                     float(max_sigma), float(scale), L.u8ptr(out), C.byref(ticks)))
        return (out if ticks.value else None), int(ticks.value)

    # ---- JPEG output (include/fspt.h fspt_draw_jpeg / fspt_present_jpeg) ----------------------------
    def _file_buffer(self, fmt, bound_first=False):
        if getattr(self, f"_{fmt}_buf", None) is None:
            setattr(self, f"_{fmt}_buf", _FileBuffer(f"fspt_{fmt}_bound", bound_first))
        return getattr(self, f"_{fmt}_buf")

    def draw_jpeg(self, source="accumulator", exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0, scale=1.0,
                  quality=85, subsampling="420", restart_mcus=0):
        """draw() ("accumulator"), draw_denoised() ("denoised") or temporal_draw() ("temporal", "temporal_denoised") of the
        same arguments as a JPEG file (bytes), encoded on the GPU: the frame never leaves the device (fspt_draw_jpeg)."""
        if source not in JPEG_SOURCES:
            raise ValueError(f"source must be one of {sorted(JPEG_SOURCES)}")
        p, lib = jpeg_params(quality, subsampling, restart_mcus), L.lib()
        return self._file_buffer("jpeg").call(*self.resolution, p, lambda o, cap, nb: lib.fspt_draw_jpeg(
            self._t, JPEG_SOURCES[source], float(exposure), float(saturation), 1 if denoise else 0, float(max_sigma), float(scale), C.byref(p), o, cap, nb))

    def draw_png(self, source="accumulator", exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0, scale=1.0,
                 channels=3, filter="adaptive", chunk_bytes=0):
        """draw() ("accumulator"), draw_denoised() ("denoised") or temporal_draw() ("temporal", "temporal_denoised") of the
        same arguments as a lossless PNG file (bytes), filtered and deflated on the GPU: only the file comes back
        (fspt_draw_png)."""
        if source not in JPEG_SOURCES:
            raise ValueError(f"source must be one of {sorted(JPEG_SOURCES)}")
        p, lib = png_params(channels, filter, chunk_bytes), L.lib()
        return self._file_buffer("png").call(*self.resolution, p, lambda o, cap, nb: lib.fspt_draw_png(
            self._t, JPEG_SOURCES[source], float(exposure), float(saturation), 1 if denoise else 0, float(max_sigma), float(scale), C.byref(p), o, cap, nb))

    def draw_exr(self, source="accumulator", compression="zip", float32=False, layers=(), chunk_bytes=0):
        """The HDR buffer itself - read_radiance()'s ("accumulator"), denoise()'s ("denoised"), temporal_accumulate()'s
        ("temporal") or temporal_denoise()'s ("temporal_denoised") - as a scene-linear OpenEXR file (bytes), with the
        first-hit guides of features() as layers ("albedo", "normal", "depth"; "alpha" is the buffer's fourth float),
        made on the GPU: only the file comes back (fspt_draw_exr).  No exposure, bloom or tone map."""
        if source not in JPEG_SOURCES:
            raise ValueError(f"source must be one of {sorted(JPEG_SOURCES)}")
        p, lib = exr_params(compression, float32, layers, chunk_bytes), L.lib()
        buf = self._file_buffer("exr", True)
        buf.mattes = None
        if p.layers & EXR_CRYPTO:  # the scene's manifests count in the bound ("crypto_object", "crypto_material": DESIGN 8.25)
            buf.mattes = L.ExrMattes()
            for k, manifest in self.scene.matte_manifests.items():
                buf.mattes.manifest[k], buf.mattes.manifest_len[k] = manifest, len(manifest)
        return buf.call(*self.resolution, p, lambda o, cap, nb: lib.fspt_draw_exr(self._t, JPEG_SOURCES[source], C.byref(p), o, cap, nb))

    def present_jpeg(self, exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0, scale=1.0, quality=85, subsampling="420", restart_mcus=0):
        """present() with the frame encoded on the GPU behind its draw (fspt_present_jpeg): (the PREVIOUS call's JPEG file as
        bytes, its sample count), or (None, 0) when there is nothing to present.  A file that outgrows the buffer is dropped
        by the library; the buffer is grown for the next one."""
        p, buf, lib = jpeg_params(quality, subsampling, restart_mcus), self._file_buffer("jpeg"), L.lib()
        n, ticks = C.c_size_t(), C.c_uint32()
        buf.ready(*self.resolution, p)
        rc = lib.fspt_present_jpeg(self._t, float(exposure), float(saturation), 1 if denoise else 0, float(max_sigma), float(scale), C.byref(p),
                                   L.u8ptr(buf.buf), buf.buf.size, C.byref(n), C.byref(ticks))
        if rc == -1 and n.value > buf.buf.size:
            buf.grow(*self.resolution, p, n.value)
            return None, 0
        L.check(rc)
        return (buf.buf[:n.value].tobytes() if ticks.value else None), int(ticks.value)

    # ---- guided denoiser (include/fspt.h fspt_features / fspt_denoise) --------------------------------
    def features(self, samples=8, seed=1):
        """Guide buffers of the set_camera() view: `samples` camera rays per pixel to their first hit (fspt_features)."""
        cp = L.CameraParams()
        cp.P = (C.c_float * 3)(*self.eye); cp.I = (C.c_float * 3)(*self.dir)
        cp.fov_scale = self.fovScale; cp.lens = (C.c_float * 2)(*self.lensFeatures)
        cp.env_theta = self.envTheta; cp.num_bounces = self.num_bounces
        L.check(L.lib().fspt_features(self._t, C.byref(cp), int(samples), int(seed)))

    # ---- ID mattes (include/fspt.h fspt_mattes) -------------------------------------------------------
    def mattes(self, samples=8, seed=1):
        """Object and material coverage of the set_camera() view: features()' rays, the ids of the scene's kinds ranked per
        pixel (fspt_mattes).  The scene needs ids (Scene.set_matte / set_default_mattes)."""
        cp = L.CameraParams()
        cp.P = (C.c_float * 3)(*self.eye); cp.I = (C.c_float * 3)(*self.dir)
        cp.fov_scale = self.fovScale; cp.lens = (C.c_float * 2)(*self.lensFeatures)
        cp.env_theta = self.envTheta; cp.num_bounces = self.num_bounces
        L.check(L.lib().fspt_mattes(self._t, C.byref(cp), int(samples), int(seed)))

    def read_mattes(self, kind, raw=False):
        """(ids uint32 [H, W, 6], coverage float32 [H, W, 6]) of the last mattes(), row 0 = bottom, rank 0 first; raw: the
        float32 [H, W, 12] buffer itself (id0 c0 .. id5 c5), what exr_encode(mattes=...) takes"""
        W, H = self.resolution
        out = np.zeros((H, W, 12), np.float32)
        L.check(L.lib().fspt_read_mattes(self._t, _matte_kind(kind), L.fptr(out)))
        if raw:
            return out
        return np.ascontiguousarray(out.view(np.uint32)[..., 0::2]), np.ascontiguousarray(out[..., 1::2])

    def mattes_lost(self, kind):
        """Samples the last mattes() dropped because a pixel's six slots were taken (fspt_mattes_lost)"""
        n = C.c_uint64()
        L.check(L.lib().fspt_mattes_lost(self._t, _matte_kind(kind), C.byref(n)))
        return int(n.value)

    def readFeatures(self):
        """float32 [H, W, 8], row 0 = bottom: albedo.rgb, depth, normal.xyz, coverage (sample means)."""
        W, H = self.resolution
        out = np.zeros((H, W, 8), np.float32)
        L.check(L.lib().fspt_read_features(self._t, L.fptr(out)))
        return out

    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None):
        """Edge-avoiding a-trous filter of the current accumulator guided by the last features() -> float32 [H, W, 4].
        None = the library's default (DENOISE_DEFAULTS = include/fspt.h FSPT_DENOISE_*)."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32)
        given = {"iterations": iterations, "sigma_color": sigma_color, "sigma_normal": sigma_normal, "sigma_depth": sigma_depth}
        prm = None
        if any(v is not None for v in given.values()):
            v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
            prm = L.DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]))
        L.check(L.lib().fspt_denoise(self._t, C.byref(prm) if prm is not None else None, L.fptr(out)))
        return out

    def drawDenoised(self, exposure=1.0, saturation=1.0):
        """draw() of the last denoise() result (fspt_draw_denoised): tonemapped RGBA8 [H, W, 4], row 0 = bottom."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.uint8)
        L.check(L.lib().fspt_draw_denoised(self._t, float(exposure), float(saturation), L.u8ptr(out)))
        return out

    # ---- temporal accumulation (include/fspt.h fspt_temporal_*) ------------------------------------
    def temporal_accumulate(self, read=True, **params):
        """One frame of temporal accumulation: the previous call's result, reprojected through the first hit of every pixel's
        centre ray of the set_camera() view, blended with the current accumulator (which is only read).  Returns the new
        history float32 [H, W, 4] (rgb, history length), or None with read=False.  params: alpha, max_history, depth_tol,
        normal_cos (TEMPORAL_DEFAULTS)."""
        prm = _temporal_params(params)
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32) if read else None
        cp = self._camera_params()
        L.check(L.lib().fspt_temporal_accumulate(self._t, C.byref(cp), C.byref(prm) if prm is not None else None,
                                                 L.fptr(out) if read else None))
        return out

    def temporal_reset(self):
        """Drop the history: the next temporal_accumulate behaves as the first (fspt_temporal_reset)."""
        L.check(L.lib().fspt_temporal_reset(self._t))

    def temporal_denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, variance=False):
        """denoise() with the temporal result in the accumulator's place (fspt_temporal_denoise) -> float32 [H, W, 4].
        variance=True (after temporal_set_moments()): the variance-guided filter (fspt_temporal_denoise_variance, DESIGN 8.9;
        sigma_color is sigma_l, in standard deviations; SVGF_DEFAULTS)."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32)
        given = {"iterations": iterations, "sigma_color": sigma_color, "sigma_normal": sigma_normal, "sigma_depth": sigma_depth}
        if variance:
            prm = _svgf_params(given)
            L.check(L.lib().fspt_temporal_denoise_variance(self._t, C.byref(prm) if prm is not None else None, L.fptr(out)))
            return out
        prm = None
        if any(v is not None for v in given.values()):
            v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
            prm = L.DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]))
        L.check(L.lib().fspt_temporal_denoise(self._t, C.byref(prm) if prm is not None else None, L.fptr(out)))
        return out

    def temporal_set_moments(self, on=True):
        """SVGF variance guidance (fspt_temporal_set_moments): temporal_accumulate() also carries two luminance
        moments of the demodulated input (it then needs features() first); what temporal_denoise(variance=True) reads."""
        L.check(L.lib().fspt_temporal_set_moments(self._t, 1 if on else 0))

    def temporal_variance(self, variance=True):
        """(v float32 [H, W], moments float32 [H, W, 2]) (fspt_temporal_read_variance): the variance estimate of the last
        temporal_denoise(variance=True) - None with variance=False, which needs no such call - and (M1, M2) of the last
        temporal_accumulate."""
        W, H = self.resolution
        v = np.zeros((H, W), np.float32) if variance else None
        m = np.zeros((H, W, 2), np.float32)
        L.check(L.lib().fspt_temporal_read_variance(self._t, L.fptr(v) if variance else None, L.fptr(m)))
        return v, m

    def svgf_last_ms(self):
        """(k_svgf_variance ms, guided iterations ms) of the last temporal_denoise(variance=True), from HIP events."""
        ms = (C.c_float * 2)()
        L.check(L.lib().fspt_svgf_last_ms(self._t, ms))
        return float(ms[0]), float(ms[1])

    def temporal_set_clamp(self, on=True, fast_history=None, sigma_scale=None):
        """History clamp (fspt_temporal_set_clamp): temporal_accumulate() also carries a fast history capped at
        fast_history samples and clamps the long one into mean +- sigma_scale spread of its 5 x 5 window, so that a change of
        the light is not averaged over max_history samples.  None: CLAMP_DEFAULTS; sigma_scale inf: the clamp never binds.
        Switching it on drops an existing history; a call that changes only the parameters keeps it."""
        fh, ss = _clamp_params(fast_history, sigma_scale) if on else (0.0, 0.0)
        L.check(L.lib().fspt_temporal_set_clamp(self._t, 1 if on else 0, fh, ss))

    def temporal_fast(self):
        """The fast history of the last temporal_accumulate with the clamp on (fspt_temporal_read_fast): float32 [H, W, 4]
        (rgb, length)."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32)
        L.check(L.lib().fspt_temporal_read_fast(self._t, L.fptr(out)))
        return out

    def temporal_clamp_last_ms(self):
        """k_temporal_clamp ms of the last temporal_accumulate with the clamp on, from HIP events."""
        ms = C.c_float()
        L.check(L.lib().fspt_temporal_clamp_last_ms(self._t, C.byref(ms)))
        return float(ms.value)

    # ---- auto-exposure (include/fspt.h fspt_target_set_auto_exposure) --------------------------------
    def set_auto_exposure(self, on=True, **params):
        """Auto-exposure (fspt_target_set_auto_exposure): every draw(), present(), drawDenoised() and temporal_draw() first meters
        the buffer it draws on the GPU, and its `exposure` argument becomes a compensation of the metered value.  params: key,
        low, high, adapt_up, adapt_down, min_log2, max_log2 (missing ones: EXPOSURE_DEFAULTS).  A call that changes only the
        parameters keeps the adapted state; off frees it."""
        prm = _exposure_params(params) if on else None
        L.check(L.lib().fspt_target_set_auto_exposure(self._t, 1 if on else 0, C.byref(prm) if on else None))

    def exposure(self):
        """(exposure, log2_mean, metered) of the last metering (fspt_exposure_get): the float32 factor the draws multiply by,
        the mean log2 luminance of the kept pixels, the pixels counted.  Blocking; joins a present."""
        e, m, n = C.c_float(), C.c_float(), C.c_uint32()
        L.check(L.lib().fspt_exposure_get(self._t, C.byref(e), C.byref(m), C.byref(n)))
        return np.float32(e.value), float(m.value), int(n.value)

    def exposure_reset(self):
        """The next metering is a first one: no adaptation from the state so far (fspt_exposure_reset)."""
        L.check(L.lib().fspt_exposure_reset(self._t))

    def exposure_last_ms(self):
        """(histogram ms, resolve ms, k_draw_auto ms) of the last metered draw, from HIP events (fspt_exposure_last_ms,
        fspt_exposure_last_draw_ms)."""
        ms, d = (C.c_float * 2)(), C.c_float()
        L.check(L.lib().fspt_exposure_last_ms(self._t, ms))
        L.check(L.lib().fspt_exposure_last_draw_ms(self._t, C.byref(d)))
        return float(ms[0]), float(ms[1]), float(d.value)

    # ---- bloom (include/fspt.h fspt_target_set_bloom) -------------------------------------------------
    def set_bloom(self, on=True, **params):
        """Bloom (fspt_target_set_bloom): every draw(), present(), drawDenoised() and temporal_draw() first builds an HDR pyramid of
        the buffer it draws, on the GPU, and mixes its glow into every texel in front of the exposure.  params: intensity, scatter,
        levels (missing ones: BLOOM_DEFAULTS).  A call that changes only the parameters keeps the allocation; off frees it."""
        prm = _bloom_params(params) if on else None
        L.check(L.lib().fspt_target_set_bloom(self._t, 1 if on else 0, C.byref(prm) if on else None))

    @property
    def bloom(self):
        """None (off) or {"intensity", "scatter", "levels"} as the library holds them (fspt_target_get_bloom)"""
        on, p = C.c_int(), L.BloomParams()
        L.check(L.lib().fspt_target_get_bloom(self._t, C.byref(on), C.byref(p)))
        return {"intensity": float(p.intensity), "scatter": float(p.scatter), "levels": int(p.levels)} if on.value else None

    def bloom_last_ms(self):
        """(down chain ms, tail ms, up chain ms, k_draw_bloom ms) of the last bloomed draw, from HIP events (fspt_bloom_last_ms)"""
        ms = (C.c_float * 4)()
        L.check(L.lib().fspt_bloom_last_ms(self._t, ms))
        return tuple(float(x) for x in ms)

    def temporal_draw(self, exposure=1.0, saturation=1.0, denoised=False):
        """draw() of the temporal result, or of the last temporal_denoise() (fspt_temporal_draw): RGBA8 [H, W, 4]."""
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.uint8)
        L.check(L.lib().fspt_temporal_draw(self._t, float(exposure), float(saturation), 1 if denoised else 0, L.u8ptr(out)))
        return out

    def temporal_gbuffer(self):
        """(G float32 [H, W, 8], M float32 [H, W, 4]) of the last temporal_accumulate (fspt_temporal_read_gbuffer): G = t, leaf
        slot (int32 bits), bv, bw, macroNormal.xyz, hit; M = sx, sy, distance, kind (0 none / behind, 1 hit, 2 miss)."""
        W, H = self.resolution
        g, m = np.zeros((H, W, 8), np.float32), np.zeros((H, W, 4), np.float32)
        L.check(L.lib().fspt_temporal_read_gbuffer(self._t, L.fptr(g), L.fptr(m)))
        return g, m

    def temporal_last_ms(self):
        """(G-buffer and motion pass ms, blend pass ms) of the last temporal_accumulate, from HIP events."""
        ms = (C.c_float * 2)()
        L.check(L.lib().fspt_temporal_last_ms(self._t, ms))
        return float(ms[0]), float(ms[1])

    def counters(self):
        c = L.Counters()
        L.check(L.lib().fspt_get_counters(self._t, C.byref(c)))
        return c.as_dict()

    def last_kernel_ms(self):
        ms = C.c_float(); n = C.c_uint32()
        L.check(L.lib().fspt_last_kernel_ms(self._t, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        """Destroy the target.  Recorded (deferred) ticks are executed first: fspt_target_destroy itself drops them - it
        never writes to a caller-owned accumulator, which may be gone by then - but here `_keep` still holds the bound
        buffer, so a host that binds a tensor, ticks and closes finds every tick in its tensor."""
        if self._t:
            L.lib().fspt_sync(self._t)  # (an error here must not keep the target alive: destroy follows regardless)
            L.lib().fspt_target_destroy(self._t)
            self._t = C.c_void_p()
            self._keep = None
            self._rays_keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiPathTracer:
    """PathTracer's frame driver over several GPUs from ONE host thread (include/fspt.h: fspt_multi_*): every device
    traces every len(devices)-th 32x32 tile of the same frame, nothing moves between devices while rendering, and
    readRadiance() / draw() gather the tiles onto devices[0] with peer-to-peer copies.  Same attribute and method
    names as PathTracer; the result is bit-identical to a single-GPU render."""
    NUM_BOUNCES = PathTracer.NUM_BOUNCES

    def __init__(self, arrays, width, height, devices=(0,), num_bounces=None):
        self.arrays = arrays
        self.devices = [int(d) for d in devices]
        self.resolution = (int(width), int(height))
        self._m = C.c_void_p()
        desc = arrays.desc()
        devs = (C.c_int * len(self.devices))(*self.devices)
        L.check(L.lib().fspt_multi_create(C.byref(desc), devs, len(self.devices), self.resolution[0], self.resolution[1],
                                          C.byref(self._m)))
        self.fovScale = 0.5
        self.envTheta = 0.0
        self.dir = [0.0, 0.0, -1.0]
        self.eye = [0.0, 0.0, 2.0]
        self.lensFeatures = [1.0 - 1.0 / 2.0, 0.02]
        self.num_bounces = self.NUM_BOUNCES if num_bounces is None else int(num_bounces)
        self.pingpong = 0
        self._rng = C.c_uint64(1)

    set_camera = PathTracer.set_camera
    seed = PathTracer.seed
    next_rand_base = PathTracer.next_rand_base

    def _targets(self):
        for i in range(len(self.devices)):
            t = C.c_void_p()
            L.check(L.lib().fspt_multi_target(self._m, i, C.byref(t)))
            yield t

    def set_pipeline(self, pipeline, batch_ticks=0):
        code = PIPELINES.get(pipeline, pipeline)
        for t in self._targets():
            L.check(L.lib().fspt_target_set_pipeline(t, int(code), int(batch_ticks)))

    def set_tail(self, round=-1):
        for t in self._targets():
            L.check(L.lib().fspt_target_set_tail(t, int(round)))

    def set_camera_model(self, model="pinhole", angle=None, ipd=None):
        """PathTracer.set_camera_model on every device's target (a ray depends on its pixel only: DESIGN 9)."""
        p = camera_model_params(model, angle, ipd)
        for t in self._targets():
            L.check(L.lib().fspt_target_set_camera_model(t, p))

    def prepare(self):
        for t in self._targets():
            L.check(L.lib().fspt_target_prepare(t))

    def drawCamera(self, randBase):
        P = (C.c_float * 3)(*self.eye); I = (C.c_float * 3)(*self.dir); lens = (C.c_float * 2)(*self.lensFeatures)
        L.check(L.lib().fspt_multi_camera(self._m, P, I, self.fovScale, lens, float(randBase)))

    def drawTracer(self, i, randBase):
        L.check(L.lib().fspt_multi_trace(self._m, int(i), float(randBase), self.envTheta, self.num_bounces))

    tick = PathTracer.tick

    def render(self, n_ticks):
        cp = L.CameraParams()
        cp.P = (C.c_float * 3)(*self.eye); cp.I = (C.c_float * 3)(*self.dir)
        cp.fov_scale = self.fovScale; cp.lens = (C.c_float * 2)(*self.lensFeatures)
        cp.env_theta = self.envTheta; cp.num_bounces = self.num_bounces
        L.check(L.lib().fspt_multi_render(self._m, C.byref(cp), self.pingpong, int(n_ticks), self._rng.value))
        for _ in range(2 * int(n_ticks)):
            self.next_rand_base()
        self.pingpong += int(n_ticks)

    def update_geometry(self, tri, norm=None):
        """Scene.update_geometry (host arrays) on every device's copy of the scene (fspt_multi_update_geometry)."""
        n = int(self.arrays.n_tris)
        tri, norm = _host_geometry("update_geometry", n, tri, norm)
        L.check(L.lib().fspt_multi_update_geometry(self._m, L.fptr(tri), None if norm is None else L.fptr(norm)))

    def set_pose(self, part, tri=None, norm=None):
        """Scene.set_pose on every device's copy of the scene (fspt_multi_set_pose); tri is required once the scene has moved."""
        if part is None:
            L.check(L.lib().fspt_multi_set_pose(self._m, None, 0, None, None))
            return
        n = int(self.arrays.n_tris)
        if tri is None:
            if norm is not None:
                raise ValueError("set_pose: norm given without tri")
            tri, norm = self.arrays.tri, self.arrays.norm
        part = np.ascontiguousarray(_u32_array(part, "part"), dtype=np.uint32).reshape(-1)
        if part.size != n:
            raise ValueError(f"set_pose: part has {part.size} elements, the scene has {n} triangles")
        tri, norm = _host_geometry("set_pose", n, tri, norm)
        L.check(L.lib().fspt_multi_set_pose(self._m, L.u32ptr(part), int(part.max()) + 1 if n else 1, L.fptr(tri),
                                            None if norm is None else L.fptr(norm)))

    def update_transforms(self, xf):
        """Scene.update_transforms on every device's copy of the scene (fspt_multi_update_transforms)."""
        xf = np.ascontiguousarray(xf, dtype=np.float32).reshape(-1)
        if xf.size % 12:
            raise ValueError(f"update_transforms: xf has {xf.size} elements, not n_parts x 12")
        L.check(L.lib().fspt_multi_update_transforms(self._m, L.fptr(xf), xf.size // 12))

    def set_skin(self, joints, weights=None, tri=None, norm=None, morph=None, morph_norm=None, n_joints=None):
        """Scene.set_skin on every device's copy of the scene (fspt_multi_set_skin); tri is required once the scene has moved."""
        if joints is None:
            L.check(L.lib().fspt_multi_set_skin(self._m, None))
            return
        if weights is None:
            raise ValueError("set_skin: joints given without weights")
        if tri is None:
            if norm is not None:
                raise ValueError("set_skin: norm given without tri")
            tri, norm = self.arrays.tri, self.arrays.norm
        d, keep = Scene._skin_desc("set_skin", int(self.arrays.n_tris), joints, weights, tri, norm, morph, morph_norm, n_joints)
        L.check(L.lib().fspt_multi_set_skin(self._m, C.byref(d)))

    def update_skin(self, xf, morph_weights=None):
        """Scene.update_skin (host arrays) on every device's copy of the scene (fspt_multi_update_skin)."""
        _, pxf, nj, pmw, nm, keep = Scene._skin_frame("update_skin", xf, morph_weights, None)
        L.check(L.lib().fspt_multi_update_skin(self._m, pxf, nj, pmw, nm))

    def set_mesh(self, vertex=None, uv=None, n_vertices=None, smooth=None, rank=None, static=None, tri=None, norm=None, drop=False):
        """Scene.set_mesh on every device's copy of the scene (fspt_multi_set_mesh)."""
        if drop:
            L.check(L.lib().fspt_multi_set_mesh(self._m, None))
            return
        d, keep = Scene._mesh_desc("set_mesh", self.arrays, getattr(self, "_moved", False), vertex, uv, n_vertices, smooth, rank, static, tri, norm)
        L.check(L.lib().fspt_multi_set_mesh(self._m, C.byref(d)))

    def update_vertices(self, pos):
        """Scene.update_vertices (a host array) on every device's copy of the scene (fspt_multi_update_vertices)."""
        _, p, nv, keep = Scene._mesh_frame("update_vertices", pos, None)
        L.check(L.lib().fspt_multi_update_vertices(self._m, p, nv))

    def update_materials(self, mat, uv=None, atlas=None, atlas_res=None, atlas_layers=None):
        """Scene.update_materials (host arrays) on every device's copy of the scene (fspt_multi_update_materials)."""
        args, keep = Scene._materials_args(self, "update_materials", mat, uv, atlas, atlas_res, atlas_layers)
        L.check(L.lib().fspt_multi_update_materials(self._m, *args))
        if atlas is not None:
            self._retained_atlas_res = args[3]

    def update_textures(self, mat, uv, packer_or_desc):
        """Scene.update_textures (host arrays) on every device's copy of the scene (fspt_multi_update_textures)."""
        from . import scene as S
        mat, uv = Scene._textures_mat_uv(self, "update_textures", mat, uv)
        p, _, _, keep = S.texture_pack_struct(packer_or_desc, None, "update_textures")
        L.check(L.lib().fspt_multi_update_textures(self._m, L.fptr(mat), None if uv is None else L.fptr(uv), C.byref(p)))
        self._retained_atlas_res = int(p.res)

    def patch_textures(self, layer_ids, layers, images=None, res=None):
        """Scene.patch_textures (host arrays) on every device's copy of the scene (fspt_multi_patch_textures)."""
        from . import scene as S
        ids, layers, images = Scene._patch_args("patch_textures", layer_ids, layers, images, None)
        res = int(res) if res is not None else getattr(self, "_retained_atlas_res", None) or 1
        p, _, _, keep = S.texture_pack_struct({"res": res, "images": images, "layers": layers}, None, "patch_textures")
        L.check(L.lib().fspt_multi_patch_textures(self._m, L.u32ptr(ids), ids.size, C.byref(p)))

    def update_environment(self, env, env_w, env_h, bins=None):
        """Scene.update_environment on every device's copy of the scene (fspt_multi_update_environment; bins=None: each
        device builds them from its copy of the map, fspt_multi_update_environment_auto - host arrays only)."""
        if bins is None:
            _, ptr, w, h, keep = Scene._environment_auto_args("update_environment", env, env_w, env_h, None)
            L.check(L.lib().fspt_multi_update_environment_auto(self._m, ptr, w, h))
            return
        args, keep = Scene._environment_args("update_environment", env, env_w, env_h, bins)
        L.check(L.lib().fspt_multi_update_environment(self._m, *args))

    def update_sky(self, sun_dir, width=1024, height=512, **params):
        """Scene.update_sky on every device's copy of the scene: each device generates its own map (fspt_multi_update_sky)."""
        from . import scene as S
        p = S.sky_params(sun_dir, **params)
        L.check(L.lib().fspt_multi_update_sky(self._m, C.byref(p), _map_side("update_sky", width), _map_side("update_sky", height)))

    def rebuild_geometry(self, tri, norm=None):
        """Scene.rebuild_geometry (host arrays) on every device's copy of the scene (fspt_multi_rebuild_geometry); every
        device builds the same tree, the one order is returned."""
        n = int(self.arrays.n_tris)
        tri, norm = _host_geometry("rebuild_geometry", n, tri, norm)
        order = np.zeros(n, np.uint32)
        L.check(L.lib().fspt_multi_rebuild_geometry(self._m, L.fptr(tri), None if norm is None else L.fptr(norm), L.u32ptr(order)))
        return order

    def clear(self):
        L.check(L.lib().fspt_multi_clear(self._m))
        self.pingpong = 0

    def sync(self):
        L.check(L.lib().fspt_multi_sync(self._m))

    def readRadiance(self):
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.float32)
        L.check(L.lib().fspt_multi_read_radiance(self._m, L.fptr(out)))
        return out

    def draw(self, exposure=1.0, saturation=1.0, denoise=False, max_sigma=3.0):
        W, H = self.resolution
        out = np.zeros((H, W, 4), np.uint8)
        L.check(L.lib().fspt_multi_draw(self._m, float(exposure), float(saturation), 1 if denoise else 0, float(max_sigma),
                                        L.u8ptr(out)))
        return out

    def peer_access(self, i):
        """How target i's tiles reach devices[0]: bit 0 = its device can write devices[0]'s memory directly (the
        direction the gather copy runs), bit 1 = the reverse; 0 = staged through the host."""
        m = C.c_int()
        L.check(L.lib().fspt_multi_peer_access(self._m, int(i), C.byref(m)))
        return m.value

    EXCHANGES = {"peer": 0, "rccl_gather": 1, "rccl_reduce": 2}

    def set_exchange(self, mode):
        """Read-out exchange: 'peer' (hipMemcpyPeerAsync of packed tiles, default), 'rccl_gather' (ncclSend / ncclRecv of
        the same tiles) or 'rccl_reduce' (ncclReduce(SUM) of own-tiles-only frames); RCCL needs distinct devices."""
        L.check(L.lib().fspt_multi_set_exchange(self._m, int(self.EXCHANGES.get(mode, mode))))

    def exchange(self):
        """(mode code, RCCL version or 0 when RCCL is not loaded)."""
        m = C.c_int(); v = C.c_int()
        L.check(L.lib().fspt_multi_get_exchange(self._m, C.byref(m), C.byref(v)))
        return m.value, v.value

    def stage_ms(self):
        """Per device [render, pack, transfer, scatter] milliseconds of the most recent render + read-out
        (fspt_multi_last_stage_ms; -1 = the stage did not run on that device).  Blocking."""
        import numpy as np
        n = len(self.devices)
        out = np.zeros((n, 4), np.float32)
        L.check(L.lib().fspt_multi_last_stage_ms(self._m, L.fptr(out), n))
        return out

    def last_gather_bytes(self):
        b = C.c_uint64()
        L.check(L.lib().fspt_multi_last_gather_bytes(self._m, C.byref(b)))
        return b.value

    def close(self):
        if self._m:
            L.lib().fspt_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bytes_per_sample(counters):
    """Algorithmic bytes per sample on the REFERENCE layout:
    60 B per traversal step (12 B header + 2x24 B child boxes, tracer.fs:374-378),
    144 B per leaf visit (4 x 36 B, tracer.fs:355-364), 280 B per shading event
    (tracer.fs:447-460), 16 B per environment lookup (tracer.fs:410-419), 64 B of
    ray + accumulator traffic per sample (tracer.fs:439,516-517)."""
    s = max(1, counters["samples"])
    return (60.0 * counters["steps"] + 144.0 * counters["leaves"] + 280.0 * counters["shades"]
            + 16.0 * counters["env_lookups"]) / s + 64.0
