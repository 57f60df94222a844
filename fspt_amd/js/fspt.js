'use strict';
/**
 * fspt.js — JavaScript host of libfspt (Node, CommonJS).
 *
 * Mirrors the reference's own host code so that main.js can switch from WebGL2
 * to the MI355X kernels with the same call order (INTEGRATION.md):
 *   buildScene's material step    drives the reference's own TexturePacker / getMaterial / ParseMaterials when the
 *                                 caller passes them (opts.host), a table-driven resolver with the same layer
 *                                 numbering otherwise (AtlasLayers / readMtl / resolveMaterial; images: decoded RGBA8)
 *   packReferenceScene            main.js:355-392 + maskBVHBuffer 272-282, fed with the
 *                                 reference's own BVH / Triangle objects (bvh.js, obj_loader.js)
 *   buildScene                    native obj_loader.js + bvh.js (same decisions, float64) for
 *                                 scenes too large for the JS builder
 *   PathTracer                    drawCamera / drawTracer / tick / clear (main.js:741-857)
 * All compute happens in the HIP kernels behind fspt_napi.node; errors surface as JS Errors.
 */
const addon = require('./fspt_napi.node');
const ABI_VERSION = 4;   // include/fspt.h FSPT_ABI_VERSION this module was written against
if (addon.abiVersion() !== ABI_VERSION) {
  throw new Error('libfspt.so has ABI version ' + addon.abiVersion() + ', fspt.js needs ' + ABI_VERSION + ': stale build (python -c "import __graft_entry__ as g; g.build()")');
}

function jsNum(v) { return String(Number(v)); }

const f = Math.fround;

/** WebGLTextureWriter.setAndDrawTexture + its shader (texture_packer.js:103-121,159-175) on the CPU, float32:
 *  bilinear (S = REPEAT, T = CLAMP_TO_EDGE) resample of a decoded image {width, height, data: RGBA8, row 0 = top}
 *  to res x res at uv = (x+.5, res-(y+.5))/res, sRGB -> linear before filtering when `corrected`, channel swizzle,
 *  rgb premultiplied by alpha, alpha = 1.  Output row 0 = bottom (readPixels).  Same arithmetic as scene.py. */
function resampleImage(img, res, corrected, swizzle) {
  const w = img.width, h = img.height, sw = swizzle || [0, 1, 2, 3];
  const lut = new Float32Array(256), lin = new Float32Array(256);
  for (let i = 0; i < 256; i++) {
    const c = f(i / 255);
    lin[i] = c;
    lut[i] = c <= 0.04045 ? f(c / 12.92) : f(Math.pow(f(f(c + 0.055) / 1.055), 2.4));
  }
  const out = new Uint8Array(res * res * 4);
  const i0 = new Int32Array(res), i1 = new Int32Array(res), ax = new Float32Array(res);
  for (let x = 0; x < res; x++) {
    const px = f(f(x + 0.5) / res), u = f(f(px * w) - 0.5), fl = Math.floor(u);
    ax[x] = f(u - fl);
    i0[x] = ((fl % w) + w) % w; i1[x] = (((fl + 1) % w) + w) % w;
  }
  const c = new Float32Array(4);
  for (let y = 0; y < res; y++) {
    const py = f(f(y + 0.5) / res), v = f(f(f(1 - py) * h) - 0.5), fl = Math.floor(v), by = f(v - fl);
    const j0 = Math.min(Math.max(fl, 0), h - 1), j1 = Math.min(Math.max(fl + 1, 0), h - 1);
    for (let x = 0; x < res; x++) {
      const a = ax[x], na = f(1 - a), nb = f(1 - by);
      for (let k = 0; k < 4; k++) {
        const t = (k < 3 && corrected) ? lut : lin;
        const p00 = t[img.data[(j0 * w + i0[x]) * 4 + k]], p01 = t[img.data[(j0 * w + i1[x]) * 4 + k]];
        const p10 = t[img.data[(j1 * w + i0[x]) * 4 + k]], p11 = t[img.data[(j1 * w + i1[x]) * 4 + k]];
        const top = f(f(p00 * na) + f(p01 * a)), bot = f(f(p10 * na) + f(p11 * a));
        c[k] = f(f(top * nb) + f(bot * by));
      }
      const al = c[sw[3]], o = (y * res + x) * 4;
      for (let k = 0; k < 3; k++) {
        const q = Math.floor(f(f(f(c[sw[k]] * al) * 255) + 0.5));
        out[o + k] = Math.min(Math.max(q, 0), 255);
      }
      out[o + 3] = 255;
    }
  }
  return out;
}

/* ---------------------------------------------------------------------------------------------------------------
 * Material resolution for buildScene.  In the reference this is host code that STAYS in the reference
 * (INTEGRATION.md 2: TexturePacker texture_packer.js:5-63, ParseMaterials mtl_loader.js:3-43, getMaterial
 * main.js:206-270): a caller that has those modules passes them in (`opts.host = {TexturePacker, getMaterial,
 * ParseMaterials}`) and buildScene drives them unchanged.  Without them - Node scripts, the tests on the GPU box -
 * the table-driven resolver below gives the same layer numbering (pinned to the reference's JS by the 'mtl' golden,
 * tests/test_node_host.py::test_js_full_scene_build_matches_reference_js).
 * ------------------------------------------------------------------------------------------------------------- */

/** The atlas layer list: one entry per distinct image (by URL) or flat colour (by its components), in first-use
 *  order.  Like the reference's packer an entry that landed at index 0 is never found again (its lookup tests the
 *  stored index for truthiness), so the first layer may appear twice - the layer ids in `mat` depend on it. */
class AtlasLayers {
  constructor(limit) { this.res = limit || 2048; this.entries = []; this.index = new Map(); this.tallest = 1; }
  _intern(key, entry) {
    const at = this.index.get(key);
    if (at) return at;
    this.entries.push(entry);
    this.index.set(key, this.entries.length - 1);
    return this.entries.length - 1;
  }
  image(img, corrected) {
    const known = this.index.get(img.currentSrc);
    if (known) return known;
    if (img.height > this.tallest) this.tallest = img.height;
    img.corrected = corrected;
    return this._intern(img.currentSrc, img);
  }
  colour(rgb) { return this._intern(rgb.join(' '), rgb); }
  resolution() { this.res = Math.min(this.res, this.tallest); return this.res; }
  /** RGBA8 texels of every layer, res x res each: flat colours as gl.clearColor + readPixels would store them, images
   *  through resampleImage */
  pixels(opts) {
    if (opts && opts.device != null) return atlasPackGpu(this.packDesc(), opts.device);   // (DESIGN 8.18) resampled on that HIP device
    const res = this.resolution(), n = res * res * 4;
    const out = new Uint8Array(n * this.entries.length);
    this.entries.forEach((e, i) => {
      if (!Array.isArray(e)) { out.set(resampleImage(e, res, !!e.corrected, e.swizzle), i * n); return; }
      const px = [0, 1, 2].map((k) => Math.floor(Math.min(Math.max(Number(e[k]), 0), 1) * 255 + 0.5));
      for (let t = i * n; t < (i + 1) * n; t += 4) { out[t] = px[0]; out[t + 1] = px[1]; out[t + 2] = px[2]; out[t + 3] = 255; }
    });
    return out;
  }
  /** the atlas as a description for the GPU packer (fspt_texture_pack, DESIGN 8.18): {res, images, layers} - the distinct
   *  images (an image that is layer 0 and a later layer too goes once) and per entry {kind: 'color', color} or
   *  {kind: 'image', image, corrected, swizzle}, with the flags the images carry now, as pixels() reads them */
  packDesc() {
    const res = this.resolution(), images = [], at = new Map();
    const layers = this.entries.map((e) => {
      if (Array.isArray(e)) return { kind: 'color', color: [0, 1, 2].map((k) => Number(e[k])) };
      if (!at.has(e)) { at.set(e, images.length); images.push(e); }
      return { kind: 'image', image: at.get(e), corrected: !!e.corrected, swizzle: e.swizzle ? Array.from(e.swizzle, Number) : [0, 1, 2, 3] };
    });
    return { res, images, layers };
  }
  describe() {
    return this.entries.map((e) => (Array.isArray(e) ? { color: e.map(Number) } :
      { src: e.currentSrc, corrected: !!e.corrected, swizzle: e.swizzle ? Array.from(e.swizzle, Number) : null }));
  }
}

/** MTL statements the pipeline reads: s = one number, v = a list of numbers, u = a file name relative to the OBJ. */
const MTL_FIELDS = { ns: 's', ni: 's', d: 's', illum: 's', dielectric: 's', ior: 's',
  ka: 'v', kd: 'v', kem: 'v', ks: 'v', ke: 'v', pr: 'v', pm: 'v', pmr: 'v', pmr_swizzle: 'v',
  map_bump: 'u', map_kd: 'u', map_kem: 'u', map_ks: 'u', map_d: 'u', map_ns: 'u', map_pmr: 'u' };
/** MTL text -> {materials: {name: {field: value}}, urls: Set}.  Statements before the first `newmtl` are ignored; a
 *  statement whose value is falsy (a scalar 0, an unparsable number) is dropped, as in the reference's loader. */
function readMtl(text, basePath) {
  const materials = {}, urls = new Set();
  let cur = null;
  for (const raw of text.split('\n')) {
    const [word, ...rest] = raw.trim().split(/[ ]+/);
    const field = word.toLowerCase();
    if (field === 'newmtl') { cur = materials[rest[0]] = {}; continue; }
    const kind = MTL_FIELDS[field];
    if (!cur || !kind) continue;
    const value = kind === 's' ? parseFloat(rest[0]) : (kind === 'v' ? rest.map(parseFloat) : rest[0]);
    if (!value) continue;
    if (kind === 'u') urls.add(basePath + '/' + value);
    cur[field] = value;
  }
  return { materials, urls };
}

/** The four atlas layers of a material, in the order their ids are handed out.  Per layer, first match wins:
 *  the group's MTL image map, the group's MTL colour, the prop's scene-JSON field (an image URL, or - where `propColour` -
 *  a colour), the default colour. */
const MATERIAL_LAYERS = [
  { id: 'diffuseIndex', map: 'map_kd', colour: 'kd', prop: 'diffuse', propColour: true, fallback: [0.5, 0.5, 0.5], corrected: true },
  { id: 'roughnessIndex', map: 'map_pmr', colour: 'pmr', prop: 'metallicRoughness', propColour: true, fallback: [0.0, 0.3, 0],
    mapSwizzle: 'pmr_swizzle', propSwizzle: 'mrSwizzle' },
  { id: 'specularIndex', map: 'map_kem', colour: 'kem', prop: 'emission', propColour: false, fallback: [0, 0, 0] },
  { id: 'normalIndex', map: 'map_bump', colour: null, prop: 'normal', propColour: false, anyTruthyProp: true, fallback: [0.5, 0.5, 1] },
];
function resolveMaterial(prop, group, layers, assets, basePath) {
  const mtl = (group && group.material) || {};
  const decoded = (url) => {
    const img = assets && assets[url];
    if (!img) throw new Error('texture ' + url + ' is not in assets');
    if (!img.currentSrc) img.currentSrc = url;
    return img;
  };
  const out = {};
  for (const L of MATERIAL_LAYERS) {
    const pv = prop[L.prop];
    let img = null, swizzle;
    if (mtl[L.map]) { img = decoded(basePath + '/' + mtl[L.map]); swizzle = mtl[L.mapSwizzle]; }
    else if (L.colour && mtl[L.colour]) { out[L.id] = layers.colour(mtl[L.colour]); continue; }
    else if (typeof pv === 'string' || (L.anyTruthyProp && pv)) { img = decoded(pv); swizzle = prop[L.propSwizzle]; }
    else if (L.propColour && pv && typeof pv === 'object') { out[L.id] = layers.colour(pv); continue; }
    else { out[L.id] = layers.colour(L.fallback); continue; }
    // the swizzle lives on the shared decoded image and is (re)set before de-duplication: the last use decides
    if (L.mapSwizzle) img.swizzle = swizzle;
    out[L.id] = L.corrected ? layers.image(img, true) : layers.image(img);
  }
  out.ior = Number(mtl.ior || prop.ior || 1.4);
  out.dielectric = Number(mtl.dielectric || prop.dielectric || -1);
  out.emittance = prop.emittance || [0, 0, 0];
  return out;
}

/** mergeSceneProps (main.js:869-871) */
function mergeSceneProps(scene) {
  return [].concat((scene.props || []), (scene.static_props || []), Object.values(scene.animated_props || []));
}

/** main.js:355-392 for a reference `BVH` instance whose triangles carry `.material`. */
function packReferenceScene(bvh) {
  const bvhArray = bvh.serializeTree();
  const bvhBuffer = [], tri = [], mat = [], norm = [], uv = [];
  for (let i = 0; i < bvhArray.length; i++) {
    const e = bvhArray[i], node = e.node;
    const triIndex = node.leaf ? tri.length / 9 : -1;
    if (node.leaf) {
      for (const t of node.getTriangles()) {
        tri.push(...t.verts[0], ...t.verts[1], ...t.verts[2]);
        const m = t.material;
        mat.push(m.diffuseIndex, m.specularIndex, m.normalIndex, m.roughnessIndex, 0, 0, ...m.emittance, m.ior, m.dielectric, 0);
        for (let k = 0; k < 3; k++) norm.push(...t.normals[k], ...t.tangents[k], ...t.bitangents[k]);
        uv.push(...t.uvs[0], ...t.uvs[1], ...t.uvs[2]);
      }
    }
    bvhBuffer.push(e.left, e.right, triIndex, ...node.boundingBox.min, ...node.boundingBox.max);
  }
  const masked = new Float32Array(new Int32Array(bvhBuffer).buffer);   // maskBVHBuffer
  for (let i = 0; i < bvhBuffer.length; i += 9) for (let j = 3; j < 9; j++) masked[i + j] = bvhBuffer[i + j];
  return { bvh: masked, tri: new Float32Array(tri), mat: new Float32Array(mat), norm: new Float32Array(norm),
           uv: new Float32Array(uv), depth: bvh.depth };
}

/** initBVH (main.js:284-445) through the native builder (same decisions, float64).
 *  sceneOrProps: the scene JSON (props / static_props / animated_props, worldTransforms, normalize, atlasRes) or a
 *  bare props array; objTexts: {path: OBJ text}; env: {rgbe, width, height} | null;
 *  opts: {mtlTexts: {url: MTL text}, assets: {url: decoded image}, focusRays: [[eye, dir], ...],
 *         host: {TexturePacker, getMaterial, ParseMaterials} (the reference's modules) + atlasPixels(packer),
 *         bvh: 'sah' (default: the reference's tree) | 'gpu' (binned SAH built on HIP device opts.device, DESIGN 8.4)}. */
function buildScene(sceneOrProps, objTexts, env, leafSize, opts) {
  opts = opts || {};
  const bvh = opts.bvh === undefined ? 'sah' : opts.bvh;
  if (bvh !== 'sah' && bvh !== 'gpu') throw new RangeError("buildScene: opts.bvh must be 'sah' or 'gpu'");
  const textures = opts.textures === undefined ? 'cpu' : opts.textures;   // 'gpu': the atlas is resampled on HIP device opts.device (DESIGN 8.18)
  if (textures !== 'cpu' && textures !== 'gpu') throw new RangeError("buildScene: opts.textures must be 'cpu' or 'gpu'");
  if (textures === 'gpu' && opts.host) throw new RangeError("buildScene: opts.textures 'gpu' packs this host's AtlasLayers, not opts.host's packer");
  const scene = Array.isArray(sceneOrProps) ? { props: sceneOrProps } : sceneOrProps;
  const props = mergeSceneProps(scene);
  // the reference's own host modules when the caller has them (INTEGRATION.md), the resolver above otherwise
  const host = opts.host || null;
  const packer = host ? new host.TexturePacker(scene.atlasRes || 2048, props.length) : new AtlasLayers(scene.atlasRes || 2048);
  const mtlOf = host ? host.ParseMaterials : readMtl;
  const materialOf = host ? host.getMaterial : resolveMaterial;
  const b = addon.builderCreate();
  let s;
  try {
    for (const p of props) {
      const basePath = p.path.split('/').slice(0, -1).join('/');
      const groups = addon.builderParseObj(b, objTexts[p.path], { rotate: p.rotate || [], scale: p.scale === undefined ? 1 : p.scale,
        translate: p.translate || [0, 0, 0], normals: p.normals || 'flat' }, scene.worldTransforms || null, p.skips || null);
      const libs = {};
      const mats = groups.map((g) => {
        let material = {};
        if (g.mtllib !== null) {
          const url = basePath + '/' + g.mtllib;
          if (!libs[url]) {
            if (!opts.mtlTexts || opts.mtlTexts[url] === undefined) throw new Error('mtllib ' + url + ' is not in opts.mtlTexts');
            libs[url] = mtlOf(opts.mtlTexts[url], basePath).materials;
          }
          material = libs[url][g.name] || {};
        }
        return materialOf(p, { material }, packer, opts.assets, basePath);
      });
      addon.builderCommit(b, mats);
    }
    if (scene.normalize) addon.builderNormalize(b, scene.normalize);
    s = bvh === 'gpu' ? addon.builderBuildGpu(b, leafSize || 4, opts.device || 0) : addon.builderBuild(b, leafSize || 4);
    s.focus = (opts.focusRays || []).map(([eye, dir]) => 1 - 1 / addon.builderAutofocus(b, eye, dir));   // main.js:544
  } finally {
    addon.builderDestroy(b);
  }
  if (host) {
    // the reference's packer renders the atlas with a WebGL context of its own (texture_packer.js:103-175): its pixels
    // are the caller's to fetch (opts.atlasPixels(packer) -> Uint8Array of res*res*4*layers); the layer ids are in `mat`
    if (typeof opts.atlasPixels !== 'function') throw new Error('buildScene: opts.host needs opts.atlasPixels(packer)');
    s.atlasRes = packer.setAndGetResolution(); s.atlasLayers = packer.imageSet.length;
    s.atlas = opts.atlasPixels(packer);
    s.layers = null;
  } else {
    s.atlas = packer.pixels(textures === 'gpu' ? { device: opts.device || 0 } : undefined); s.atlasRes = packer.res; s.atlasLayers = packer.entries.length;
    Object.defineProperty(s, 'packer', { value: packer, enumerable: false });   // (updateTextures takes it; not a part of the arrays)
    s.layers = packer.describe();
  }
  if (env) { s.env = env.rgbe; s.envW = env.width; s.envH = env.height; s.bins = addon.envBins(env.rgbe, env.width, env.height); }
  else { s.env = null; s.envW = 0; s.envH = 0; s.bins = new Uint32Array([0, 0, 1, 2048]); }   // main.js:292
  s.leafSize = leafSize || 4;
  s.bvhBuilder = bvh;
  return s;
}

/** `.fspt` scene blob (layout: fspt_amd/blob.py). */
const fs = require('fs');
const DT = [Float32Array, Uint8Array, Uint32Array];
function saveBlob(path, s) {
  const secs = [['bvh', s.bvh], ['tri', s.tri], ['mat', s.mat], ['norm', s.norm], ['uv', s.uv], ['atlas', s.atlas],
    ['bins', s.bins], ['meta', new Uint32Array([s.atlasRes, s.atlasLayers, s.env ? s.envW : 0, s.env ? s.envH : 0, s.leafSize, s.depth || 0])]];
  if (s.env) secs.push(['env', s.env]);
  const parts = [Buffer.from('FSPT'), Buffer.alloc(8)];
  parts[1].writeUInt32LE(1, 0); parts[1].writeUInt32LE(secs.length, 4);
  for (const [name, arr] of secs) {
    const h = Buffer.alloc(24);
    h.write(name, 0, 'ascii');
    h.writeUInt32LE(DT.findIndex((T) => arr instanceof T), 8);
    h.writeBigUInt64LE(BigInt(arr.length), 16);
    const raw = Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength);
    parts.push(h, raw, Buffer.alloc((16 - (raw.length % 16)) % 16));
  }
  fs.writeFileSync(path, Buffer.concat(parts));
}
function loadBlob(path) {
  const buf = fs.readFileSync(path);
  if (buf.toString('ascii', 0, 4) !== 'FSPT' || buf.readUInt32LE(4) !== 1) throw new Error('not a version-1 .fspt blob');
  const n = buf.readUInt32LE(8), secs = {};
  let off = 12;
  for (let i = 0; i < n; i++) {
    const name = buf.toString('ascii', off, off + 8).replace(/\0+$/, '');
    const T = DT[buf.readUInt32LE(off + 8)], count = Number(buf.readBigUInt64LE(off + 16));
    off += 24;
    const nbytes = count * T.BYTES_PER_ELEMENT;
    secs[name] = new T(buf.buffer.slice(buf.byteOffset + off, buf.byteOffset + off + nbytes));
    off += nbytes + ((16 - (nbytes % 16)) % 16);
  }
  const m = secs.meta;
  return { bvh: secs.bvh, tri: secs.tri, mat: secs.mat, norm: secs.norm, uv: secs.uv, atlas: secs.atlas, atlasRes: m[0],
    atlasLayers: m[1], env: secs.env || null, envW: m[2], envH: m[3], bins: secs.bins, leafSize: m[4], depth: m[5] };
}

const PIPELINE_CODES = { megakernel: 0, wavefront: 1, stream: 2 };

// a pipeline name (or a code of include/fspt_tuning.h's fspt_target_set_pipeline); anything else is an error, as in the Python host
const CAMERA_MODELS = ['pinhole', 'ortho', 'fisheye', 'equirect', 'stereo'];  // include/fspt.h FSPT_CAMERA_*
/** setCameraModel's { model, angle, ipd } checked -> [code, angle, ipd] for the addon (which checks them again) */
function cameraModelArgs(params) {
  const p = params === undefined || params === null ? {} : params;
  if (typeof p !== 'object') throw new TypeError('setCameraModel: expects { model, angle, ipd }');
  const name = p.model === undefined || p.model === null ? 'pinhole' : p.model;
  const code = CAMERA_MODELS.indexOf(name);
  if (code < 0) throw new RangeError("setCameraModel: model must be one of 'pinhole', 'ortho', 'fisheye', 'equirect', 'stereo'");
  if (p.angle !== undefined && name !== 'fisheye') throw new RangeError("setCameraModel: angle only goes with 'fisheye'");
  if (p.ipd !== undefined && name !== 'stereo') throw new RangeError("setCameraModel: ipd only goes with 'stereo'");
  const angle = p.angle === undefined ? f(Math.PI) : p.angle, ipd = p.ipd === undefined ? f(0.064) : p.ipd;
  if (typeof angle !== 'number' || !(f(angle) > 0 && f(angle) <= f(2 * Math.PI))) throw new RangeError('setCameraModel: angle must be a number in (0, 2 pi] radians');
  if (typeof ipd !== 'number' || !(f(ipd) >= 0 && Number.isFinite(f(ipd)))) throw new RangeError('setCameraModel: ipd must be a finite number >= 0');
  return [code, angle, ipd];
}
/** fspt_tuning.h FSPT_SKY_*: the defaults of the sky model (DESIGN 8.17) */
const SKY_DEFAULTS = { turbidity: 1, sunIntensity: 20, sunRadius: 0.02, gain: 1, groundAlbedo: 0.3, viewSamples: 16, lightSamples: 8, width: 1024, height: 512 };
/** {sunDir, ...} -> what the addon takes: the ten floats of fspt_sky_params, the two counts and the size (ranges: the library's) */
function skyArgs(fn, o) {
  if (o == null || typeof o !== 'object' || !Array.isArray(o.sunDir) && !(o.sunDir instanceof Float32Array) || o.sunDir.length !== 3) throw new TypeError(fn + ': expected {sunDir: [x, y, z], ...}');
  for (const key of Object.keys(o)) if (key !== 'sunDir' && !(key in SKY_DEFAULTS)) throw new TypeError(fn + ': unknown parameter ' + key);
  const p = Object.assign({}, SKY_DEFAULTS, o);
  const alb = typeof p.groundAlbedo === 'number' ? [p.groundAlbedo, p.groundAlbedo, p.groundAlbedo] : p.groundAlbedo;
  if (!alb || alb.length !== 3) throw new RangeError(fn + ': groundAlbedo must be a number or [r, g, b]');
  for (const key of ['viewSamples', 'lightSamples', 'width', 'height']) if (!Number.isInteger(p[key]) || p[key] < 0 || p[key] > 0xFFFFFFFF) throw new RangeError(fn + ': ' + key + ' must be a count');
  const params = Float32Array.of(p.sunDir[0], p.sunDir[1], p.sunDir[2], p.turbidity, p.sunIntensity, p.sunRadius, p.gain, alb[0], alb[1], alb[2]);
  return { params, viewSamples: p.viewSamples, lightSamples: p.lightSamples, width: p.width, height: p.height };
}
const PNG_FILTERS = { none: 0, sub: 1, up: 2, average: 3, paeth: 4, adaptive: 5 };
/** {channels (3 | 4), filter (a name of PNG_FILTERS, 'adaptive'), chunkBytes (0 = the library's default)} -> the addon's three numbers */
function pngArgs(o, fn) {
  const ch = o.channels === undefined ? 3 : o.channels, f = PNG_FILTERS[o.filter === undefined ? 'adaptive' : String(o.filter)];
  const cb = o.chunkBytes === undefined ? 0 : o.chunkBytes;
  if (ch !== 3 && ch !== 4) throw new RangeError(fn + ': channels must be 3 or 4');
  if (f === undefined) throw new RangeError(fn + ": filter must be 'none', 'sub', 'up', 'average', 'paeth' or 'adaptive'");
  if (!Number.isInteger(cb) || (cb !== 0 && (cb < 256 || cb > 32768))) throw new RangeError(fn + ': chunkBytes must be 0 or an integer in 256..32768');
  return [ch, f, cb];
}
/** An RGBA8 image (Uint8Array of width*height*4; bottomUp: row 0 is the bottom, as drawQuad returns it) as a lossless PNG file,
 *  filtered and deflated on the GPU (include/fspt.h fspt_png_encode, DESIGN.md 8.20) -> Buffer.
 *  opts: {channels (3 = RGB, 4 = RGBA), filter ('adaptive'), chunkBytes (0), bottomUp (false), device (0)}. */
function pngEncode(rgba, width, height, opts) {
  const o = opts || {}, enc = pngArgs(o, 'pngEncode');
  if (!(rgba instanceof Uint8Array) || rgba.length !== width * height * 4) throw new RangeError('pngEncode: need a Uint8Array of width*height*4 bytes');
  let out = new Uint8Array(width * height * 4 + 1024);
  let n = addon.pngEncode(o.device || 0, rgba, width, height, !!o.bottomUp, ...enc, out);
  if (n < 0) { out = new Uint8Array(Math.max(-n, addon.pngBound(width, height, ...enc))); n = addon.pngEncode(o.device || 0, rgba, width, height, !!o.bottomUp, ...enc, out); }
  if (n < 0) throw new Error('pngEncode: the file outgrew the bound');
  return Buffer.from(out.subarray(0, n));
}
/** stage one of pngEncode alone (fspt_png_filtered_eval): the filtered stream, height rows of 1 + width * channels bytes */
function pngFilteredEval(rgba, width, height, opts) {
  const o = opts || {}, enc = pngArgs(o, 'pngFilteredEval');
  if (!(rgba instanceof Uint8Array) || rgba.length !== width * height * 4) throw new RangeError('pngFilteredEval: need a Uint8Array of width*height*4 bytes');
  const out = new Uint8Array(height * (1 + width * enc[0]));
  addon.pngFilteredEval(o.device || 0, rgba, width, height, !!o.bottomUp, ...enc, out);
  return out;
}
const EXR_COMPRESSIONS = { none: 0, zips: 2, zip: 3 };
const EXR_LAYERS = { alpha: 1, albedo: 2, normal: 4, depth: 8, crypto_object: 16, crypto_material: 32 }; // (the last two: the Cryptomatte ID mattes of DESIGN.md 8.25)
const EXR_CRYPTO = 16 | 32;
const MATTE_KINDS = { object: 0, material: 1 };
function matteKind(kind, fn) {
  const k = MATTE_KINDS[kind];
  if (k === undefined) throw new RangeError(fn + ": kind must be 'object' or 'material'");
  return k;
}
/** The 32-bit id of a name (include/fspt.h fspt_matte_hash, DESIGN.md 8.25): MurmurHash3_x86_32 of its UTF-8 bytes, seed 0, then Cryptomatte's float rule */
function matteHash(name) { return addon.matteHash(String(name)); }
/** Cryptomatte's manifest of `names`: JSON {"name":"%08x", ...} in the order given (non-ASCII characters escaped, as the Python host writes them) */
function matteManifest(names) {
  const esc = (s) => JSON.stringify(String(s)).replace(/[\u007f-\uffff]/g, (c) => '\\u' + c.charCodeAt(0).toString(16).padStart(4, '0'));
  return '{' + names.map((n) => esc(n) + ':"' + matteHash(n).toString(16).padStart(8, '0') + '"').join(',') + '}';
}
/** {compression ('zip' | 'zips' | 'none'), float32 (false: HALF; Z is always FLOAT), layers (names of EXR_LAYERS: an array, or one string with
 *  commas), chunkBytes (0 = the library's default)} -> the addon's four numbers */
function exrArgs(o, fn) {
  const c = EXR_COMPRESSIONS[o.compression === undefined ? 'zip' : String(o.compression)];
  const names = o.layers === undefined ? [] : Array.isArray(o.layers) ? o.layers : String(o.layers).split(',').filter((x) => x);
  const cb = o.chunkBytes === undefined ? 0 : o.chunkBytes;
  if (c === undefined) throw new RangeError(fn + ": compression must be 'none', 'zips' or 'zip'");
  let bits = 0;
  for (const n of names) {
    if (EXR_LAYERS[n] === undefined) throw new RangeError(fn + ": layers must be among 'alpha', 'albedo', 'normal' and 'depth'");
    bits |= EXR_LAYERS[n];
  }
  if (!Number.isInteger(cb) || (cb !== 0 && (cb < 256 || cb > 32768))) throw new RangeError(fn + ': chunkBytes must be 0 or an integer in 256..32768');
  return [c, o.float32 ? 2 : 1, bits, cb];
}
/** Scene-linear radiance (Float32Array of width*height*4; bottomUp: row 0 is the bottom, as readRadiance returns it) and, for the albedo,
 *  normal and depth layers, the features (Float32Array of width*height*8, as readFeatures returns them) as a scanline OpenEXR file made
 *  on the GPU (include/fspt.h fspt_exr_encode, DESIGN.md 8.21) -> Buffer.
 *  opts: {compression ('zip'), float32 (false), layers ([]), chunkBytes (0), bottomUp (false), device (0)}. */
function exrEncode(rgba, features, width, height, opts) {
  const o = opts || {}, enc = exrArgs(o, 'exrEncode');
  if (o.mattes != null) return exrEncodeMattes(rgba, features, width, height, o, enc);
  if (!(rgba instanceof Float32Array) || rgba.length !== width * height * 4) throw new RangeError('exrEncode: need a Float32Array of width*height*4 floats');
  if (enc[2] & 14 ? !(features instanceof Float32Array) || features.length !== width * height * 8 : features != null && !(features instanceof Float32Array && features.length === width * height * 8)) {
    throw new RangeError('exrEncode: the albedo, normal and depth layers need features, a Float32Array of width*height*8 floats');
  }
  const out = new Uint8Array(addon.exrBound(width, height, ...enc));
  const n = addon.exrEncode(o.device || 0, rgba, features || null, width, height, !!o.bottomUp, ...enc, out);
  if (n < 0) throw new Error('exrEncode: the file outgrew the bound');
  return Buffer.from(out.subarray(0, n));
}
/** exrEncode with opts.mattes = { object, material }: each a Float32Array of width*height*12 floats as readMattes(kind, true) returns
 *  it, or { ranks, manifest (a string) }, for the 'crypto_object' / 'crypto_material' layers (fspt_exr_encode_mattes, DESIGN.md 8.25) */
function exrEncodeMattes(rgba, features, width, height, o, enc) {
  if (!(rgba instanceof Float32Array) || rgba.length !== width * height * 4) throw new RangeError('exrEncode: need a Float32Array of width*height*4 floats');
  const ranks = [null, null], manifest = [null, null];
  for (const kind of Object.keys(o.mattes)) {
    const k = matteKind(kind, 'exrEncode'), v = o.mattes[kind];
    ranks[k] = v instanceof Float32Array ? v : v.ranks;
    manifest[k] = v instanceof Float32Array || v.manifest == null || v.manifest === '' ? null : String(v.manifest);
    if (!(ranks[k] instanceof Float32Array) || ranks[k].length !== width * height * 12) throw new RangeError('exrEncode: matte ranks must be a Float32Array of width*height*12 floats');
  }
  const out = new Uint8Array(addon.exrBoundMattes(width, height, ...enc, manifest[0], manifest[1]));
  const n = addon.exrEncodeMattes(o.device || 0, rgba, features || null, ranks[0], ranks[1], manifest[0], manifest[1], width, height, !!o.bottomUp, ...enc, out);
  if (n < 0) throw new Error('exrEncode: the file outgrew the bound');
  return Buffer.from(out.subarray(0, n));
}
const JPEG_SUBSAMPLING = { '444': 0, '420': 1 };
const JPEG_SOURCES = { accumulator: 0, denoised: 1, temporal: 2, temporalDenoised: 3 };
/** An RGBA8 image (Uint8Array of width*height*4, alpha ignored; bottomUp: row 0 is the bottom, as drawQuad returns it) as a
 *  baseline JPEG file, encoded on the GPU (include/fspt.h fspt_jpeg_encode, DESIGN.md 8.19) -> Buffer.
 *  opts: {quality (85), subsampling ('420' | '444'), restartMcus (0 = one MCU row), bottomUp (false), device (0)}. */
function jpegEncode(rgba, width, height, opts) {
  const o = opts || {};
  const sub = JPEG_SUBSAMPLING[o.subsampling === undefined ? '420' : String(o.subsampling)];
  if (sub === undefined) throw new RangeError("jpegEncode: subsampling must be '444' or '420'");
  if (!(rgba instanceof Uint8Array) || rgba.length !== width * height * 4) throw new RangeError('jpegEncode: need a Uint8Array of width*height*4 bytes');
  const q = o.quality === undefined ? 85 : o.quality, ri = o.restartMcus === undefined ? 0 : o.restartMcus;
  let out = new Uint8Array(width * height * 4 + 1024);
  let n = addon.jpegEncode(o.device || 0, rgba, width, height, !!o.bottomUp, q, sub, ri, out);
  if (n < 0) { out = new Uint8Array(Math.max(-n, addon.jpegBound(width, height, q, sub, ri))); n = addon.jpegEncode(o.device || 0, rgba, width, height, !!o.bottomUp, q, sub, ri, out); }
  if (n < 0) throw new Error('jpegEncode: the file outgrew the bound');
  return Buffer.from(out.subarray(0, n));
}

/** a generated sky as {rgbe Uint8Array, width, height} on HIP device `device` (fspt_sky_generate): what buildScene takes as env */
function skyGenerate(o, device) {
  const k = skyArgs('skyGenerate', o);
  return { rgbe: addon.skyGenerate(device || 0, k.params, k.viewSamples, k.lightSamples, k.width, k.height), width: k.width, height: k.height };
}
/** env_sampler.js's bins of an RGBE map, built on HIP device `device` (fspt_env_bins_gpu; addon.envBins is the CPU's) */
/* Texture packing on the GPU (DESIGN 8.18).  A description is {res, images: [{width, height, data}], layers: [{kind: 'color',
 * color} | {kind: 'image', image, corrected, swizzle} | {kind: 'pixels', image}]} (AtlasLayers.packDesc()); it crosses to the
 * addon as typed arrays.  Sizes are checked here, values by the library. */
const TEX_KINDS = { color: 0, image: 1, pixels: 2 };
function texDescArgs(fn, d) {
  if (d instanceof AtlasLayers) d = d.packDesc();
  if (d == null || typeof d !== 'object' || !Array.isArray(d.images) || !Array.isArray(d.layers)) throw new TypeError(fn + ': expected a texture description {res, images, layers}');
  if (!Number.isInteger(d.res) || d.res < 0 || d.res > 0xFFFFFFFF) throw new RangeError(fn + ': res must be an integer');
  const dims = new Uint32Array(d.images.length * 2);
  const images = d.images.map((im, i) => {
    if (im == null || !Number.isInteger(im.width) || !Number.isInteger(im.height) || im.width < 0 || im.height < 0 || im.width > 0xFFFFFFFF || im.height > 0xFFFFFFFF ||
        im.data == null || !ArrayBuffer.isView(im.data) || im.data.BYTES_PER_ELEMENT !== 1 || im.data.length !== im.width * im.height * 4) {
      throw new RangeError(fn + ': images[' + i + '] must be {width, height, data: width x height x 4 bytes}');
    }
    dims[2 * i] = im.width; dims[2 * i + 1] = im.height;
    return im.data instanceof Uint8Array ? im.data : new Uint8Array(im.data.buffer, im.data.byteOffset, im.data.length);
  });
  const layers = new Float32Array(d.layers.length * 10);
  d.layers.forEach((y, l) => {
    if (y == null || typeof y !== 'object') throw new TypeError(fn + ': layers[' + l + '] must be an object');
    const o = l * 10;
    layers[o] = y.kind in TEX_KINDS ? TEX_KINDS[y.kind] : Number(y.kind);
    if (y.kind === 'color') {
      if (!y.color || y.color.length < 3) throw new RangeError(fn + ': layers[' + l + '].color must hold 3 numbers');
      // the ABI carries float32: a colour goes as the float64 quantisation pixels() makes of it, byte / 255 (non-finite: as given, refused)
      for (let k = 0; k < 3; k++) { const c = Number(y.color[k]); layers[o + 1 + k] = Number.isFinite(c) ? Math.floor(Math.min(Math.max(c, 0), 1) * 255 + 0.5) / 255 : c; }
      return;
    }
    if (!Number.isInteger(y.image) || y.image < 0) throw new RangeError(fn + ': layers[' + l + '].image must be an index into images');
    layers[o + 4] = y.image; layers[o + 5] = y.corrected ? 1 : 0;
    const sw = y.swizzle == null ? [0, 1, 2, 3] : y.swizzle;
    if (sw.length !== 4) throw new RangeError(fn + ': layers[' + l + '].swizzle must hold 4 channel indices');
    for (let k = 0; k < 4; k++) layers[o + 6 + k] = Number(sw[k]);
  });
  return { images, dims, layers, res: d.res };
}
/** the raw atlas (Uint8Array, res^2 * layers RGBA8 texels, GL rows) of a description or an AtlasLayers, packed on HIP device
 *  `device` (fspt_atlas_pack_gpu, DESIGN 8.18) */
function atlasPackGpu(desc, device) {
  const k = texDescArgs('atlasPackGpu', desc);
  return addon.atlasPackGpu(device || 0, k.images, k.dims, k.layers, k.res);
}
function envBinsGpu(rgbe, w, h, device) { return addon.envBinsGpu(rgbe, w, h, device || 0); }

function pipelineCode(name) {
  if (PIPELINE_CODES[name] !== undefined) return PIPELINE_CODES[name];
  if (Number.isInteger(name) && name >= 0 && name <= 2) return name;
  throw new Error("unknown pipeline '" + name + "' (want " + Object.keys(PIPELINE_CODES).join(', ') + ')');
}

class PathTracer {
  /** scene: {bvh,tri,mat,norm,uv,atlas,atlasRes,atlasLayers,env,envW,envH,bins,leafSize} */
  constructor(scene, width, height, device) {
    this.resolution = [width, height];
    this._scene = addon.sceneCreate(scene, device || 0);
    this._nTris = scene.tri.length / 9;       // updateGeometry checks its arrays against it
    this._manifests = [null, null];            // setMatte's manifests by kind (drawExr's bound counts them)
    this._target = addon.targetCreate(this._scene, width, height);
    // main.js:67-74
    this.fovScale = 0.5; this.envTheta = 0; this.dir = [0, 0, -1]; this.eye = [0, 0, 2];
    this.lensFeatures = [1 - 1 / 2.0, 0.02];
    this.numBounces = 4;                       // tracer.fs:9
    this.pingpong = 0;
    this._rng = new BigUint64Array([1n]);      // replaces Math.random()*10000 (main.js:748,777)
  }
  seed(s) { this._rng[0] = BigInt(s); }
  _randBase() { return addon.randBaseNext(this._rng); }
  drawCamera(randBase) { addon.camera(this._target, this.eye, this.dir, this.fovScale, this.lensFeatures, randBase === undefined ? this._randBase() : randBase); }
  drawTracer(i, randBase) { addon.trace(this._target, i, randBase === undefined ? this._randBase() : randBase, this.envTheta, this.numBounces); }
  drawTracerTest(i) { addon.traceTest(this._target, i); }   // mode=test: bvh_test.fs (main.js:879-883)
  tick() { this.drawCamera(); this.drawTracer(this.pingpong); this.pingpong++; }            // main.js:838-857
  render(nTicks) {
    addon.render(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, this.pingpong, nTicks, this._rng[0]);
    for (let k = 0; k < 2 * nTicks; k++) this._randBase();
    this.pingpong += nTicks;
  }
  /** render(nTicks) on a worker thread (napi_async_work): resolves when the ticks are on the device's accumulator.
   *  Until it settles every other call on this tracer throws Error('render in flight') (enforced by the addon: the
   *  library's contract is one thread at a time per target, like the reference's single-threaded tick(),
   *  main.js:838-857); close() waits for it. */
  renderAsync(nTicks) {
    const p = addon.renderAsync(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, this.pingpong, nTicks, this._rng[0]);
    for (let k = 0; k < 2 * nTicks; k++) this._randBase();
    this.pingpong += nTicks;
    const settled = p.then(() => {}, () => {});
    this._inflight = settled;
    settled.then(() => { if (this._inflight === settled) this._inflight = null; });
    return p;
  }
  clear() { addon.clear(this._target); this.pingpong = 0; }                                  // main.js:826-836
  /** Adaptive sampling (include/fspt.h fspt_render_adaptive, DESIGN 8.5): clear, then rounds of roundTicks ticks over the
   *  32x32 tiles whose estimated relative MSE is still >= targetRelMse, each at least minTicks and at most maxTicks ticks.
   *  Returns the largest count run; pingpong and the randBase stream then stand where render(that count) leaves them. */
  renderAdaptive(opts) {
    const o = opts || {};
    const t = o.targetRelMse, maxT = o.maxTicks === undefined ? 1024 : o.maxTicks;
    const minT = o.minTicks === undefined ? 64 : o.minTicks, r = o.roundTicks === undefined ? 32 : o.roundTicks;
    if (typeof t !== 'number' || !Number.isFinite(t) || t < 0) throw new RangeError('renderAdaptive: targetRelMse must be a finite number >= 0');
    for (const [name, v] of [['maxTicks', maxT], ['minTicks', minT], ['roundTicks', r]]) {
      if (!Number.isInteger(v) || v < 0 || v > 0xFFFFFFFF) throw new RangeError(`renderAdaptive: ${name} must be an integer in [0, 2^32)`);
    }
    const n = addon.renderAdaptive(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, t, maxT, minT, r, this._rng[0]);
    for (let k = 0; k < 2 * n; k++) this._randBase();
    this.pingpong = n;
    return n;
  }
  /** the last renderAdaptive()'s ticks per pixel: Uint32Array(W*H), rows bottom-up, 0 outside its viewport */
  readSampleCounts(out) {
    out = out || new Uint32Array(this.resolution[0] * this.resolution[1]);
    if (!(out instanceof Uint32Array) || out.length !== this.resolution[0] * this.resolution[1]) throw new RangeError('readSampleCounts: need a Uint32Array of W*H counts');
    return addon.readSampleCounts(this._target, out);
  }
  /** wait until every enqueued (and recorded) tick is on the accumulator (gl.finish) */
  sync() { addon.sync(this._target); }
  readRadiance(out) {
    out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('readRadiance: need W*H*4 floats');
    return addon.readRadiance(this._target, out);
  }
  /** drawQuad (main.js:809-824) -> draw.fs: tonemapped RGBA8 as the canvas would hold it (row 0 = bottom). */
  drawQuad(exposure, saturation, denoise, maxSigma, out, resScale) {
    out = out || new Uint8Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('drawQuad: need W*H*4 bytes');
    return addon.draw(this._target, exposure === undefined ? 1 : exposure, saturation === undefined ? 1 : saturation,
      !!denoise, maxSigma === undefined ? 3 : maxSigma, out, resScale === undefined ? 1 : resScale);   // draw.fs `scale`
  }
  /** drawQuad inside tick() (main.js:838-857), pipelined with one frame of latency (include/fspt.h fspt_present,
   *  DESIGN.md 4.3): enqueues the ticks recorded since the last call and their frame, writes the PREVIOUS call's frame
   *  into `out` and returns its sample count (1 + its newest tick index; 0 = nothing presented yet, `out` untouched). */
  present(exposure, saturation, denoise, maxSigma, out, resScale) {
    if (!out || out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('present: need W*H*4 bytes');
    return addon.present(this._target, exposure === undefined ? 1 : exposure, saturation === undefined ? 1 : saturation,
      !!denoise, maxSigma === undefined ? 3 : maxSigma, out, resScale === undefined ? 1 : resScale);
  }
  /** JPEG output (include/fspt.h fspt_draw_jpeg / fspt_present_jpeg, DESIGN.md 8.19): the frame is drawn AND encoded on the GPU -
   *  a baseline JFIF file, byte for byte libjpeg's - and only the file crosses the bus.  opts: {source: 'accumulator' | 'denoised' |
   *  'temporal' | 'temporalDenoised', exposure, saturation, denoise, maxSigma, scale, quality (85), subsampling ('420' | '444'),
   *  restartMcus (0 = one MCU row)}.  drawJpeg -> Buffer.  presentJpeg -> {jpeg: Buffer | null, ticks}: the PREVIOUS call's file
   *  (present()'s one frame of latency; null with ticks 0 when there is nothing to present).  One reusable buffer of W*H*4 + 1024
   *  bytes, grown to the library's bound when a file needs more (a present frame that did is dropped by the library). */
  _jpegArgs(o, fn) {
    o = o || {};
    const sub = JPEG_SUBSAMPLING[o.subsampling === undefined ? '420' : String(o.subsampling)];
    if (sub === undefined) throw new RangeError(fn + ": subsampling must be '444' or '420'");
    const q = o.quality === undefined ? 85 : o.quality, ri = o.restartMcus === undefined ? 0 : o.restartMcus;
    if (!Number.isInteger(q) || q < 1 || q > 100) throw new RangeError(fn + ': quality must be an integer in 1..100');
    if (!Number.isInteger(ri) || ri < 0 || ri > 65535) throw new RangeError(fn + ': restartMcus must be an integer in 0..65535');
    if (!this._jpegBuf) this._jpegBuf = new Uint8Array(this.resolution[0] * this.resolution[1] * 4 + 1024);
    return { o, enc: [q, sub, ri], draw: [o.exposure === undefined ? 1 : o.exposure, o.saturation === undefined ? 1 : o.saturation, !!o.denoise,
      o.maxSigma === undefined ? 3 : o.maxSigma, o.scale === undefined ? 1 : o.scale] };
  }
  _jpegGrow(need, enc) {
    this._jpegBuf = new Uint8Array(Math.max(need, addon.jpegBound(this.resolution[0], this.resolution[1], enc[0], enc[1], enc[2])));
  }
  drawJpeg(opts) {
    const a = this._jpegArgs(opts, 'drawJpeg');
    const src = JPEG_SOURCES[a.o.source === undefined ? 'accumulator' : a.o.source];
    if (src === undefined) throw new RangeError("drawJpeg: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'");
    let n = addon.drawJpeg(this._target, src, ...a.draw, ...a.enc, this._jpegBuf);
    if (n < 0) { this._jpegGrow(-n, a.enc); n = addon.drawJpeg(this._target, src, ...a.draw, ...a.enc, this._jpegBuf); }
    if (n < 0) throw new Error('drawJpeg: the file outgrew the bound');
    return Buffer.from(this._jpegBuf.subarray(0, n));
  }
  /** drawJpeg's lossless sibling (include/fspt.h fspt_draw_png, DESIGN.md 8.20): the frame is drawn, filtered and deflated on the
   *  GPU and only the PNG file crosses the bus -> Buffer.  opts: drawJpeg's source and draw settings, pngEncode's channels / filter /
   *  chunkBytes.  Its own reusable buffer, grown to the library's bound when a file needs more. */
  drawPng(opts) {
    const o = opts || {}, enc = pngArgs(o, 'drawPng');
    const src = JPEG_SOURCES[o.source === undefined ? 'accumulator' : o.source];
    if (src === undefined) throw new RangeError("drawPng: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'");
    const draw = [o.exposure === undefined ? 1 : o.exposure, o.saturation === undefined ? 1 : o.saturation, !!o.denoise,
      o.maxSigma === undefined ? 3 : o.maxSigma, o.scale === undefined ? 1 : o.scale];
    if (!this._pngBuf) this._pngBuf = new Uint8Array(this.resolution[0] * this.resolution[1] * 4 + 1024);
    let n = addon.drawPng(this._target, src, ...draw, ...enc, this._pngBuf);
    if (n < 0) {
      this._pngBuf = new Uint8Array(Math.max(-n, addon.pngBound(this.resolution[0], this.resolution[1], ...enc)));
      n = addon.drawPng(this._target, src, ...draw, ...enc, this._pngBuf);
    }
    if (n < 0) throw new Error('drawPng: the file outgrew the bound');
    return Buffer.from(this._pngBuf.subarray(0, n));
  }
  /** The HDR buffer itself as a scene-linear OpenEXR file (include/fspt.h fspt_draw_exr, DESIGN.md 8.21): readRadiance's ('accumulator'),
   *  denoise's, temporalAccumulate's or temporalDenoise's buffer, with the guides of features() as layers; made on the GPU, only the file
   *  crosses the bus -> Buffer.  opts: {source, compression, float32, layers, chunkBytes} as exrEncode's.  No exposure, bloom or tone map. */
  drawExr(opts) {
    const o = opts || {}, enc = exrArgs(o, 'drawExr');
    const src = JPEG_SOURCES[o.source === undefined ? 'accumulator' : o.source];
    if (src === undefined) throw new RangeError("drawExr: source must be 'accumulator', 'denoised', 'temporal' or 'temporalDenoised'");
    const need = enc[2] & EXR_CRYPTO ? addon.exrBoundMattes(this.resolution[0], this.resolution[1], ...enc, this._manifests[0], this._manifests[1])
      : addon.exrBound(this.resolution[0], this.resolution[1], ...enc);
    if (!this._exrBuf || this._exrBuf.length < need) this._exrBuf = new Uint8Array(need);
    let n = addon.drawExr(this._target, src, ...enc, this._exrBuf);
    if (n < 0) { this._exrBuf = new Uint8Array(-n); n = addon.drawExr(this._target, src, ...enc, this._exrBuf); }
    if (n < 0) throw new Error('drawExr: the file outgrew the bound');
    return Buffer.from(this._exrBuf.subarray(0, n));
  }
  presentJpeg(opts) {
    const a = this._jpegArgs(opts, 'presentJpeg');
    const [n, ticks] = addon.presentJpeg(this._target, ...a.draw, ...a.enc, this._jpegBuf);
    if (n < 0) { this._jpegGrow(-n, a.enc); return { jpeg: null, ticks: 0 }; }
    return { jpeg: ticks ? Buffer.from(this._jpegBuf.subarray(0, n)) : null, ticks };
  }
  /** Guided denoiser (include/fspt.h, DESIGN.md 8).  features(): guide buffers of the current view - `samples` camera rays
   *  per pixel to their first hit; denoise(): the edge-avoiding a-trous filter of the accumulator, {iterations, sigmaColor,
   *  sigmaNormal, sigmaDepth} (omitted = the library's defaults) -> Float32Array(W*H*4); drawDenoised(): drawQuad of that
   *  frame (call it in place of drawQuad). */
  features(samples, seed) {
    addon.features(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, samples === undefined ? 8 : samples, seed === undefined ? 1 : seed);
  }
  /** ID mattes (include/fspt.h fspt_scene_set_matte_ids / _manifest, fspt_mattes; DESIGN.md 8.25).  setMatte(kind, triLabel, names):
   *  kind 'object' | 'material'; triLabel = per triangle (current leaf order) an index into names, negative = no matte; a triangle's id
   *  is matteHash of its name, the manifest matteManifest(names); two names with one hash throw.  setMatte(kind, null) drops the kind.
   *  mattes(samples, seed): features()' rays, the ids ranked per pixel.  readMattes(kind) -> { ids: Uint32Array(W*H*6), coverage:
   *  Float32Array(W*H*6) }, rows bottom-up, rank 0 first (raw = true: the Float32Array(W*H*12) itself, what exrEncode's mattes take).
   *  mattesLost(kind): the samples the last pass dropped.  drawExr takes the layers 'crypto_object' and 'crypto_material'.
   *  Every one of them throws Error('render in flight') during a renderAsync. */
  setMatte(kind, triLabel, names) {
    const k = matteKind(kind, 'setMatte');
    if (triLabel == null) { addon.sceneSetMatte(this._scene, this._nTris, k, null, null); this._manifests[k] = null; return; }
    if (triLabel.length !== this._nTris) throw new RangeError('setMatte: triLabel must hold ' + this._nTris + ' labels');
    const hashes = names.map((n) => matteHash(n)), seen = new Map();
    names.forEach((n, i) => {
      if (seen.has(hashes[i]) && seen.get(hashes[i]) !== String(n)) throw new RangeError('setMatte: the names ' + JSON.stringify(seen.get(hashes[i])) + ' and ' + JSON.stringify(String(n)) + ' have one hash');
      seen.set(hashes[i], String(n));
    });
    const ids = new Uint32Array(this._nTris);
    for (let i = 0; i < ids.length; i++) {
      const l = triLabel[i];
      if (l >= names.length) throw new RangeError('setMatte: label ' + l + ', ' + names.length + ' names');
      ids[i] = l >= 0 ? hashes[l] : 0;
    }
    const manifest = matteManifest(names);
    addon.sceneSetMatte(this._scene, this._nTris, k, ids, manifest);
    this._manifests[k] = manifest;
  }
  mattes(samples, seed) {
    addon.mattes(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, samples === undefined ? 8 : samples, seed === undefined ? 1 : seed);
  }
  readMattes(kind, raw) {
    const px = this.resolution[0] * this.resolution[1];
    const out = addon.readMattes(this._target, matteKind(kind, 'readMattes'), new Float32Array(px * 12));
    if (raw) return out;
    const bits = new Uint32Array(out.buffer), ids = new Uint32Array(px * 6), coverage = new Float32Array(px * 6);
    for (let i = 0; i < px * 6; i++) { ids[i] = bits[2 * i]; coverage[i] = out[2 * i + 1]; }
    return { ids, coverage };
  }
  mattesLost(kind) { return addon.mattesLost(this._target, matteKind(kind, 'mattesLost')); }
  denoise(opts, out) {
    out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('denoise: need W*H*4 floats');
    return addon.denoise(this._target, opts || null, out);
  }
  drawDenoised(exposure, saturation, out) {
    out = out || new Uint8Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('drawDenoised: need W*H*4 bytes');
    return addon.drawDenoised(this._target, exposure === undefined ? 1 : exposure, saturation === undefined ? 1 : saturation, out);
  }
  /** Temporal accumulation (include/fspt.h fspt_temporal_*, DESIGN.md 8.8), one call per frame after the frame's ticks:
   *  temporalAccumulate(): the previous call's result reprojected through every pixel's first hit and blended with the
   *  accumulator, {alpha, maxHistory, depthTol, normalCos} (omitted = the library's defaults) -> Float32Array(W*H*4) (rgb,
   *  history length; out === null: nothing is read back); temporalReset(): the next call is a first one; temporalDenoise() / temporalDraw(): denoise() /
   *  drawQuad() of the temporal result (denoised: of the last temporalDenoise); motionBegin(): snapshot the triangles -
   *  what updateGeometry moves until the next temporalAccumulate is reprojected from there; motionEnd(): drop it. */
  temporalAccumulate(opts, out) {
    if (opts != null) {
      const d = { alpha: 0, maxHistory: 64, depthTol: 0.05, normalCos: 0.95 };  // include/fspt_tuning.h FSPT_TEMPORAL_* (tests/test_temporal_cpu.py ties them)
      for (const k of Object.keys(opts)) if (!(k in d)) throw new RangeError('temporalAccumulate: unknown parameter ' + k);
      const v = Object.assign(d, opts);
      if (!(v.alpha >= 0 && v.alpha <= 1 && v.maxHistory >= 1 && v.depthTol >= 0 && v.normalCos >= -1 && v.normalCos <= 1))
        throw new RangeError('temporalAccumulate: need alpha in [0, 1], maxHistory >= 1, depthTol >= 0, normalCos in [-1, 1]');
    }
    if (out !== null) {  // (null: keep the result on the device, nothing is read back)
      out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
      if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('temporalAccumulate: need W*H*4 floats');
    }
    return addon.temporalAccumulate(this._target, { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures,
      envTheta: this.envTheta, numBounces: this.numBounces }, opts || null, out);
  }
  temporalReset() { addon.temporalReset(this._target); }
  temporalDenoise(opts, out) {
    out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('temporalDenoise: need W*H*4 floats');
    return addon.temporalDenoise(this._target, opts || null, out);
  }
  /** SVGF variance guidance (include/fspt.h, DESIGN.md 8.9): temporalSetMoments(true) makes temporalAccumulate() carry two
   *  luminance moments (it then needs features() first); temporalDenoiseVariance() is temporalDenoise() guided by the variance
   *  estimate ({iterations, sigmaColor = sigma_l in standard deviations, sigmaNormal, sigmaDepth}; omitted = the library's defaults). */
  temporalSetMoments(on) { addon.temporalSetMoments(this._target, on === undefined ? true : !!on); }
  temporalDenoiseVariance(opts, out) {
    out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('temporalDenoiseVariance: need W*H*4 floats');
    return addon.temporalDenoiseVariance(this._target, opts || null, out);
  }
  /** History clamp (include/fspt.h, DESIGN.md 8.10): temporalSetClamp(true, {fastHistory, sigmaScale}) makes temporalAccumulate() carry a
   *  fast history and clamp the long one into mean +- sigmaScale spread of its 5 x 5 window (omitted = the library's defaults; sigmaScale
   *  Infinity: never binds).  Switching it on drops an existing history; a call that changes only the parameters keeps it. */
  temporalSetClamp(on, opts) {
    const d = { fastHistory: 32, sigmaScale: 1 };  // include/fspt_tuning.h FSPT_TEMPORAL_CLAMP_* (tests/test_clamp_cpu.py ties them)
    if (opts != null) {
      for (const k of Object.keys(opts)) if (!(k in d)) throw new RangeError('temporalSetClamp: unknown parameter ' + k);
      Object.assign(d, opts);
    }
    if (typeof d.fastHistory !== 'number' || typeof d.sigmaScale !== 'number') throw new TypeError('temporalSetClamp: fastHistory and sigmaScale must be numbers');
    addon.temporalSetClamp(this._target, on === undefined ? true : !!on, d.fastHistory, d.sigmaScale);
  }
  /** Auto-exposure (include/fspt.h, DESIGN.md 8.11): setAutoExposure(true, {key, low, high, adaptUp, adaptDown, minLog2, maxLog2}) makes every
   *  drawQuad(), present(), drawDenoised() and temporalDraw() meter the buffer it draws on the GPU; their exposure argument becomes a compensation
   *  (omitted parameters = the library's defaults).  A call that changes only the parameters keeps the adapted state.  exposure(): {exposure,
   *  log2Mean, metered} of the last metering (blocking); exposureReset(): the next metering is a first one. */
  setAutoExposure(on, opts) {
    const d = { key: 0.18, low: 0.10, high: 0.90, adaptUp: 1, adaptDown: 1, minLog2: -8, maxLog2: 8 };  // include/fspt_tuning.h FSPT_EXPOSURE_*
    if (opts != null) {
      for (const k of Object.keys(opts)) if (!(k in d)) throw new RangeError('setAutoExposure: unknown parameter ' + k);
      Object.assign(d, opts);
    }
    for (const k of Object.keys(d)) if (typeof d[k] !== 'number') throw new TypeError('setAutoExposure: ' + k + ' must be a number');
    addon.setAutoExposure(this._target, on === undefined ? true : !!on, d.key, d.low, d.high, d.adaptUp, d.adaptDown, d.minLog2, d.maxLog2);
  }
  /** Bloom (include/fspt.h, DESIGN.md 8.12): setBloom(true, {intensity, scatter, levels}) makes every drawQuad(), present(), drawDenoised() and
   *  temporalDraw() build an HDR pyramid of the buffer it draws on the GPU and mix its glow in before the exposure (omitted parameters = the
   *  library's defaults).  A call that changes only the parameters keeps the allocation.  bloom: the parameters in force, or null (off). */
  setBloom(on, opts) {
    const d = { intensity: 0.05, scatter: 0.7, levels: 6 };  // include/fspt_tuning.h FSPT_BLOOM_*
    if (opts != null) {
      for (const k of Object.keys(opts)) if (!(k in d)) throw new RangeError('setBloom: unknown parameter ' + k);
      Object.assign(d, opts);
    }
    for (const k of Object.keys(d)) if (typeof d[k] !== 'number') throw new TypeError('setBloom: ' + k + ' must be a number');
    if (!Number.isInteger(d.levels)) throw new RangeError('setBloom: levels must be a whole number');
    addon.setBloom(this._target, on === undefined ? true : !!on, d.intensity, d.scatter, d.levels);
  }
  get bloom() { return addon.bloom(this._target); }
  exposure() { return addon.exposure(this._target); }
  exposureReset() { addon.exposureReset(this._target); }
  temporalDraw(exposure, saturation, denoised, out) {
    out = out || new Uint8Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('temporalDraw: need W*H*4 bytes');
    return addon.temporalDraw(this._target, exposure === undefined ? 1 : exposure, saturation === undefined ? 1 : saturation, !!denoised, out);
  }
  motionBegin() { addon.sceneMotionBegin(this._scene); }
  motionEnd() { addon.sceneMotionEnd(this._scene); }
  /** gl.viewport(0, 0, w, h) of drawCamera / drawTracer (main.js:744,761); the reference: resolution * resScale. */
  setViewport(w, h) { addon.setViewport(this._target, w || 0, h || 0); }
  setShard(shard, nShards, tile) { addon.setShard(this._target, shard, nShards, tile || 32); }
  /** the paths' random numbers (include/fspt.h fspt_target_set_sampler): 'reference' (default, rnd() bit for bit) or
   *  'sobol' (Owen-scrambled Sobol seeded by `seed`, an integer in [0, 2^32)) */
  setSampler(kind, seed) {
    const code = { reference: 0, sobol: 1 }[kind];
    if (code === undefined) throw new RangeError("setSampler: kind must be 'reference' or 'sobol'");
    const s = seed === undefined ? 0 : seed;
    if (!Number.isInteger(s) || s < 0 || s > 0xFFFFFFFF) throw new RangeError('setSampler: seed must be an integer in [0, 2^32)');
    addon.setSampler(this._target, code, s);
  }
  /** next-event estimation of emissive triangles (include/fspt.h fspt_target_set_lights, DESIGN 8.3): 'emitters' or 'off'
   *  (default, the reference bit for bit); emitterFraction in (0, 1], default 0.5 */
  setLights(mode, emitterFraction) {
    const code = { off: 0, emitters: 1 }[mode === undefined ? 'emitters' : mode];
    if (code === undefined) throw new RangeError("setLights: mode must be 'off' or 'emitters'");
    const f = emitterFraction === undefined ? 0.5 : emitterFraction;
    if (typeof f !== 'number' || !(f > 0 && f <= 1)) throw new RangeError('setLights: emitterFraction must be a number in (0, 1]');
    addon.setLights(this._target, code, f);
  }
  /** who builds the scene's emitter light table (include/fspt.h fspt_scene_set_light_builder, DESIGN 8.23): 'host' (default)
   *  or 'gpu' (on the device: 8 bytes are read back per build).  Drops an existing table; it is rebuilt at once when the
   *  lights are on.  Throws Error('render in flight') during a renderAsync. */
  setLightBuilder(builder) {
    const code = { host: 0, gpu: 1 }[builder];
    if (code === undefined) throw new RangeError("setLightBuilder: builder must be 'host' or 'gpu'");
    addon.sceneSetLightBuilder(this._scene, code);
  }
  getLightBuilder() {
    return ['host', 'gpu'][addon.sceneGetLightBuilder(this._scene)];
  }
  /** the camera model (include/fspt.h fspt_target_set_camera_model, DESIGN 8.15): { model: 'pinhole' (default) | 'ortho' |
   *  'fisheye' | 'equirect' | 'stereo', angle (fisheye: field of view over the frame height in radians, in (0, 2 pi],
   *  default pi), ipd (stereo: scene units, >= 0, default 0.064; the height must be even) }.  Runs the recorded ticks
   *  first, does not clear.  Throws Error('render in flight') during a renderAsync. */
  setCameraModel(params) {
    addon.setCameraModel(this._target, ...cameraModelArgs(params));
  }
  get cameraModel() {
    const p = addon.cameraModel(this._target);
    return { model: CAMERA_MODELS[p.model], angle: p.angle, ipd: p.ipd };
  }
  /** new vertices (Float32Array, 9 per triangle) and optionally normTex records (27 per triangle) for the scene's triangles
   *  in leaf order: the BVH is refitted on the GPU, nothing else changes (include/fspt.h fspt_scene_update_geometry, DESIGN
   *  8.6).  The accumulator is not cleared: call clear().  Throws Error('render in flight') during a renderAsync. */
  updateGeometry(tri, norm) {
    if (!(tri instanceof Float32Array) || tri.length !== this._nTris * 9) throw new RangeError('updateGeometry: tri must be a Float32Array of ' + this._nTris + ' x 9 floats');
    if (norm != null && (!(norm instanceof Float32Array) || norm.length !== this._nTris * 27)) throw new RangeError('updateGeometry: norm must be a Float32Array of ' + this._nTris + ' x 27 floats');
    addon.sceneUpdateGeometry(this._scene, this._nTris, tri, norm == null ? null : norm);
  }
  /** Hand the scene a pose (fspt_scene_set_pose, DESIGN 8.14): part = Uint32Array, one part id per triangle in the current leaf
   *  order; tri / norm = the rest mesh in that order (norm null: updateTransforms leaves the normals alone); nParts defaults
   *  to max(part) + 1.  setPose(null) drops the pose.  Nothing renders differently until updateTransforms. */
  setPose(part, tri, norm, nParts) {
    if (part == null) { addon.sceneSetPose(this._scene, this._nTris, null, 0, null, null); return; }
    if (!(part instanceof Uint32Array) || part.length !== this._nTris) throw new RangeError('setPose: part must be a Uint32Array of ' + this._nTris + ' ids');
    if (!(tri instanceof Float32Array) || tri.length !== this._nTris * 9) throw new RangeError('setPose: tri must be a Float32Array of ' + this._nTris + ' x 9 floats');
    if (norm != null && (!(norm instanceof Float32Array) || norm.length !== this._nTris * 27)) throw new RangeError('setPose: norm must be a Float32Array of ' + this._nTris + ' x 27 floats');
    let n = 0;
    for (let i = 0; i < part.length; i++) if (part[i] >= n) n = part[i] + 1;
    if (nParts != null) {
      if (!Number.isInteger(nParts) || nParts < Math.max(n, 1)) throw new RangeError('setPose: nParts must be an integer >= max(part) + 1');
      n = nParts;
    }
    addon.sceneSetPose(this._scene, this._nTris, part, Math.max(n, 1), tri, norm == null ? null : norm);
  }
  /** One row-major 3 x 4 matrix per part (Float32Array, 12 floats each): a kernel poses the rest mesh and the tree is refitted
   *  exactly as updateGeometry on the posed arrays would (fspt_scene_update_transforms, DESIGN 8.14). */
  updateTransforms(xf) {
    if (!(xf instanceof Float32Array) || xf.length === 0 || xf.length % 12 !== 0) throw new RangeError('updateTransforms: xf must be a Float32Array of n_parts x 12 floats');
    addon.sceneUpdateTransforms(this._scene, xf);
  }
  /** Hand the scene a skin (fspt_scene_set_skin, DESIGN 8.16): { joints: Uint16Array, weights: Float32Array } hold 4 ids and
   *  4 weights per triangle corner (12 per triangle, current leaf order; weights are used as given), tri / norm the rest mesh
   *  in that order (norm null: updateSkin leaves the normals alone), morph / morphNorm the morph targets as deltas, target
   *  after target (9 / 27 floats per triangle each; morphNorm needs norm), nJoints the joint count (default max(joints) + 1).
   *  setSkin(null) drops the skin.  Nothing renders differently until updateSkin. */
  setSkin(skin) {
    if (skin == null) { addon.sceneSetSkin(this._scene, this._nTris, null, null, 0, null, null, null, null); return; }
    const { joints, weights, tri, norm, morph, morphNorm, nJoints } = skin;
    const n = this._nTris;
    if (!(joints instanceof Uint16Array) || joints.length !== n * 12) throw new RangeError('setSkin: joints must be a Uint16Array of ' + n + ' x 12 ids');
    if (!(weights instanceof Float32Array) || weights.length !== n * 12) throw new RangeError('setSkin: weights must be a Float32Array of ' + n + ' x 12 floats');
    if (!(tri instanceof Float32Array) || tri.length !== n * 9) throw new RangeError('setSkin: tri must be a Float32Array of ' + n + ' x 9 floats');
    if (norm != null && (!(norm instanceof Float32Array) || norm.length !== n * 27)) throw new RangeError('setSkin: norm must be a Float32Array of ' + n + ' x 27 floats');
    let nMorph = 0;
    if (morph != null) {
      if (!(morph instanceof Float32Array) || n === 0 || morph.length === 0 || morph.length % (n * 9) !== 0) throw new RangeError('setSkin: morph must be a Float32Array of nMorph x ' + n + ' x 9 floats');
      nMorph = morph.length / (n * 9);
      if (nMorph > 64) throw new RangeError('setSkin: at most 64 morph targets, got ' + nMorph);
    }
    if (morphNorm != null) {
      if (norm == null) throw new RangeError('setSkin: morphNorm needs norm');
      if (!(morphNorm instanceof Float32Array) || nMorph === 0 || morphNorm.length !== nMorph * n * 27) throw new RangeError('setSkin: morphNorm must be a Float32Array of ' + nMorph + ' x ' + n + ' x 27 floats');
    }
    let nj = 0;
    for (let i = 0; i < joints.length; i++) if (joints[i] >= nj) nj = joints[i] + 1;
    nj = Math.max(nj, 1);
    if (nJoints != null) {
      if (!Number.isInteger(nJoints) || nJoints < nj || nJoints > 65535) throw new RangeError('setSkin: nJoints must be an integer in [max(joints) + 1, 65535]');
      nj = nJoints;
    }
    if (nj > 65535) throw new RangeError('setSkin: joint ids must be < 65535');
    addon.sceneSetSkin(this._scene, n, joints, weights, nj, tri, norm == null ? null : norm, morph == null ? null : morph, morphNorm == null ? null : morphNorm);
  }
  /** One frame of the skin: xf = one row-major 3 x 4 matrix per joint (Float32Array, 12 floats each), morphWeights = one float
   *  per morph target (Float32Array; null when the skin has none).  A kernel morphs, blends and poses every corner and the
   *  tree is refitted exactly as updateGeometry on the result would (fspt_scene_update_skin, DESIGN 8.16). */
  updateSkin(xf, morphWeights) {
    if (!(xf instanceof Float32Array) || xf.length === 0 || xf.length % 12 !== 0) throw new RangeError('updateSkin: xf must be a Float32Array of n_joints x 12 floats');
    if (morphWeights != null && !(morphWeights instanceof Float32Array)) throw new RangeError('updateSkin: morphWeights must be a Float32Array of n_morph floats');
    addon.sceneUpdateSkin(this._scene, xf, morphWeights == null || morphWeights.length === 0 ? null : morphWeights);
  }
  /** Hand the scene an indexed mesh (fspt_scene_set_mesh, DESIGN 8.24): { vertex: Uint32Array, 3 indices per triangle in the
   *  current leaf order (0xFFFFFFFF three times: a static triangle), uv: Float64Array, the 6 raw vt values per triangle,
   *  nVertices (default max(vertex) + 1), smooth: Uint8Array | null, one flag per triangle (null: all flat), rank: Uint32Array |
   *  null, the order a face normal is summed in (null: the leaf position), tri / norm: the rest mesh the static triangles keep
   *  (null only when none is static) }.  setMesh(null) drops the mesh.  Nothing renders differently until updateVertices. */
  setMesh(mesh) {
    if (mesh == null) { addon.sceneSetMesh(this._scene, this._nTris, null, 0, null, null, null, null, null); return; }
    const { vertex, uv, nVertices, smooth, rank, tri, norm } = mesh;
    const n = this._nTris;
    if (!(vertex instanceof Uint32Array) || vertex.length !== n * 3) throw new RangeError('setMesh: vertex must be a Uint32Array of ' + n + ' x 3 indices');
    if (!(uv instanceof Float64Array) || uv.length !== n * 6) throw new RangeError('setMesh: uv must be a Float64Array of ' + n + ' x 6 values');
    if (smooth != null && (!(smooth instanceof Uint8Array) || smooth.length !== n)) throw new RangeError('setMesh: smooth must be a Uint8Array of ' + n + ' flags');
    if (rank != null && (!(rank instanceof Uint32Array) || rank.length !== n)) throw new RangeError('setMesh: rank must be a Uint32Array of ' + n + ' ranks');
    if (tri != null && (!(tri instanceof Float32Array) || tri.length !== n * 9)) throw new RangeError('setMesh: tri must be a Float32Array of ' + n + ' x 9 floats');
    if (norm != null && (!(norm instanceof Float32Array) || norm.length !== n * 27)) throw new RangeError('setMesh: norm must be a Float32Array of ' + n + ' x 27 floats');
    let nv = 0, anyStatic = false;
    for (let i = 0; i < vertex.length; i++) { if (vertex[i] === 0xFFFFFFFF) anyStatic = true; else if (vertex[i] >= nv) nv = vertex[i] + 1; }
    nv = Math.max(nv, 1);
    if (anyStatic && (tri == null || norm == null)) throw new RangeError('setMesh: static triangles need the rest tri and norm');
    if (nVertices != null) {
      if (!Number.isInteger(nVertices) || nVertices < nv || nVertices > 0xFFFFFFFE) throw new RangeError('setMesh: nVertices must be an integer in [max(vertex) + 1, 2^32 - 2]');
      nv = nVertices;
    }
    addon.sceneSetMesh(this._scene, n, vertex, nv, uv, smooth == null ? null : smooth, rank == null ? null : rank, tri == null ? null : tri, norm == null ? null : norm);
  }
  /** One frame of the mesh: pos = one position per vertex (Float32Array, 3 floats each).  Kernels derive the vertices and
   *  normal frames of every meshed triangle by the reference's rules in float64 and the tree is refitted exactly as
   *  updateGeometry on the result would (fspt_scene_update_vertices, DESIGN 8.24). */
  updateVertices(pos) {
    if (!(pos instanceof Float32Array) || pos.length === 0 || pos.length % 3 !== 0) throw new RangeError('updateVertices: pos must be a Float32Array of n_vertices x 3 floats');
    addon.sceneUpdateVertices(this._scene, pos);
  }
  /** { tri, norm }: the Float32Arrays (9 / 27 floats per triangle) the most recent updateVertices derived (fspt_scene_read_mesh). */
  readMesh() { return addon.sceneReadMesh(this._scene, this._nTris); }
  /** The arguments of updateGeometry, but the scene gets a NEW tree - the binned SAH of the GPU builder over `tri` in the
   *  order given - built on the GPU and installed in place (fspt_scene_rebuild_geometry, DESIGN 8.7).  Returns a Uint32Array:
   *  order[k] = index in `tri` of the triangle now at leaf position k; later updateGeometry / rebuildGeometry calls take
   *  their triangles in that order.  clear() restarts the mean. */
  rebuildGeometry(tri, norm) {
    if (!(tri instanceof Float32Array) || tri.length !== this._nTris * 9) throw new RangeError('rebuildGeometry: tri must be a Float32Array of ' + this._nTris + ' x 9 floats');
    if (norm != null && (!(norm instanceof Float32Array) || norm.length !== this._nTris * 27)) throw new RangeError('rebuildGeometry: norm must be a Float32Array of ' + this._nTris + ' x 27 floats');
    return addon.sceneRebuildGeometry(this._scene, this._nTris, tri, norm == null ? null : norm);
  }
  /** new materials for the scene's triangles in leaf order: {mat (Float32Array, 12 per triangle), uv (Float32Array, 6 per
   *  triangle; omitted: kept), atlas (Uint8Array, atlasRes^2 * atlasLayers RGBA8 texels; omitted: the atlas of the last call
   *  that carried one), atlasRes, atlasLayers}.  Laid out again on the GPU; the scene then renders like one created from the
   *  same arrays (include/fspt.h fspt_scene_update_materials, DESIGN 8.13).  Accumulator, history and exposure stay: call
   *  clear().  Throws Error('render in flight') during a renderAsync. */
  updateMaterials(o) {
    if (o == null || typeof o !== 'object') throw new TypeError('updateMaterials: expected {mat, uv, atlas, atlasRes, atlasLayers}');
    const { mat, uv, atlas, atlasRes, atlasLayers } = o;
    if (!(mat instanceof Float32Array) || mat.length !== this._nTris * 12) throw new RangeError('updateMaterials: mat must be a Float32Array of ' + this._nTris + ' x 12 floats');
    if (uv != null && (!(uv instanceof Float32Array) || uv.length !== this._nTris * 6)) throw new RangeError('updateMaterials: uv must be a Float32Array of ' + this._nTris + ' x 6 floats');
    if (atlas != null) {
      if (!Number.isInteger(atlasRes) || !Number.isInteger(atlasLayers) || atlasRes < 1 || atlasLayers < 1) throw new RangeError('updateMaterials: an atlas needs atlasRes >= 1 and atlasLayers >= 1');
      if (!(atlas instanceof Uint8Array) || atlas.length !== atlasRes * atlasRes * atlasLayers * 4) throw new RangeError('updateMaterials: atlas must be a Uint8Array of ' + atlasRes + ' x ' + atlasRes + ' x ' + atlasLayers + ' x 4 bytes');
    }
    addon.sceneUpdateMaterials(this._scene, this._nTris, mat, uv == null ? null : uv, atlas == null ? null : atlas, atlas == null ? 0 : atlasRes, atlas == null ? 0 : atlasLayers);
  }
  /** updateMaterials with the atlas made on the GPU: {mat, uv (omitted: kept), textures: a texture description or an
   *  AtlasLayers}.  Only the decoded images cross the bus; a kernel resamples them into a new raw atlas and the call goes on
   *  as updateMaterials carrying it (fspt_scene_update_textures, DESIGN 8.18).  Throws Error('render in flight') during a renderAsync. */
  updateTextures(o) {
    if (o == null || typeof o !== 'object') throw new TypeError('updateTextures: expected {mat, uv, textures}');
    const { mat, uv, textures } = o;
    if (!(mat instanceof Float32Array) || mat.length !== this._nTris * 12) throw new RangeError('updateTextures: mat must be a Float32Array of ' + this._nTris + ' x 12 floats');
    if (uv != null && (!(uv instanceof Float32Array) || uv.length !== this._nTris * 6)) throw new RangeError('updateTextures: uv must be a Float32Array of ' + this._nTris + ' x 6 floats');
    const k = texDescArgs('updateTextures', textures);
    addon.sceneUpdateTextures(this._scene, this._nTris, mat, uv == null ? null : uv, k.images, k.dims, k.layers, k.res);
  }
  /** replace layers of the atlas the scene retains: {layerIds, layers, images, res} - layers[k] (indexing `images`) becomes
   *  layer layerIds[k]; res is the retained atlas's.  The scene is laid out again with its current materials
   *  (fspt_scene_patch_textures, DESIGN 8.18).  Throws Error('render in flight') during a renderAsync. */
  patchTextures(o) {
    if (o == null || typeof o !== 'object') throw new TypeError('patchTextures: expected {layerIds, layers, images, res}');
    const ids = o.layerIds instanceof Uint32Array ? o.layerIds : Array.isArray(o.layerIds) && o.layerIds.every((x) => Number.isInteger(x) && x >= 0 && x <= 0xFFFFFFFF) ? Uint32Array.from(o.layerIds) : null;
    if (ids === null) throw new TypeError('patchTextures: layerIds must be a Uint32Array or an array of layer indices');
    const k = texDescArgs('patchTextures', { res: o.res, images: o.images || [], layers: o.layers });
    if (ids.length !== k.layers.length / 10) throw new RangeError('patchTextures: ' + ids.length + ' layer ids for ' + k.layers.length / 10 + ' layers');
    addon.scenePatchTextures(this._scene, ids, k.images, k.dims, k.layers, k.res);
  }
  /** a new environment: {env (Uint8Array RGBE, envW * envH texels; null: black), envW, envH, bins (Uint32Array, 4 per bin,
   *  required)} (fspt_scene_update_environment, DESIGN 8.13); state stays as for updateMaterials */
  updateEnvironment(o) {
    if (o == null || typeof o !== 'object') throw new TypeError('updateEnvironment: expected {env, envW, envH, bins}');
    const { env, envW, envH, bins } = o;
    if (!(bins instanceof Uint32Array) || bins.length < 4 || bins.length % 4 !== 0) throw new RangeError('updateEnvironment: bins must be a Uint32Array of 4 words per bin, at least one bin');
    if (env != null) {
      if (!Number.isInteger(envW) || !Number.isInteger(envH) || envW < 1 || envH < 1) throw new RangeError('updateEnvironment: an env needs envW >= 1 and envH >= 1');
      if (!(env instanceof Uint8Array) || env.length !== envW * envH * 4) throw new RangeError('updateEnvironment: env must be a Uint8Array of ' + envW + ' x ' + envH + ' x 4 bytes');
    }
    addon.sceneUpdateEnvironment(this._scene, env == null ? null : env, env == null ? 0 : envW, env == null ? 0 : envH, bins);
  }
  /** a new environment whose bins the GPU builds from the uploaded map: {env (Uint8Array RGBE, envW * envH texels), envW, envH}
   *  (fspt_scene_update_environment_auto, DESIGN 8.17); state stays as for updateMaterials.  (updateEnvironment keeps asking for
   *  bins: a host that forgot them is told so.) */
  updateEnvironmentAuto(o) {
    if (o == null || typeof o !== 'object') throw new TypeError('updateEnvironmentAuto: expected {env, envW, envH}');
    const { env, envW, envH } = o;
    if (!Number.isInteger(envW) || !Number.isInteger(envH) || envW < 1 || envH < 1) throw new RangeError('updateEnvironmentAuto: an env needs envW >= 1 and envH >= 1');
    if (!(env instanceof Uint8Array) || env.length !== envW * envH * 4) throw new RangeError('updateEnvironmentAuto: env must be a Uint8Array of ' + envW + ' x ' + envH + ' x 4 bytes');
    addon.sceneUpdateEnvironmentAuto(this._scene, env, envW, envH);
  }
  /** the environment replaced by a sky generated, binned and tiled on the GPU: {sunDir [x, y, z], width (1024), height (512),
   *  turbidity, sunIntensity, sunRadius, gain, groundAlbedo (a number or [r, g, b]), viewSamples, lightSamples} (skyArgs'
   *  defaults; fspt_scene_update_sky, DESIGN 8.17); state stays as for updateMaterials */
  updateSky(o) {
    const k = skyArgs('updateSky', o);
    addon.sceneUpdateSky(this._scene, k.params, k.viewSamples, k.lightSamples, k.width, k.height);
  }
  /** SAH cost of the tree with its current boxes relative to the root's area (fspt_scene_sah_cost) */
  sahCost() { return addon.sceneSahCost(this._scene); }
  /** 'wavefront' (batches of ticks), 'stream' (fixed pool of live paths), 'megakernel' (include/fspt_tuning.h) */
  setPipeline(name, batch) { addon.setPipeline(this._target, pipelineCode(name), batch || 0); }
  /** traversal steps a starved trace wave walks on before it suspends its rays (0 = never; include/fspt.h) */
  setTraceBudget(steps) { addon.setTraceBudget(this._target, steps); }
  /** stream scheduler: live paths per state set (0 = default), drain iterations (-1 = default), iteration cap (0 = none) */
  setPool(paths, drain, maxIterations, overlap) { addon.setPool(this._target, paths || 0, drain === undefined ? -1 : drain, maxIterations || 0, overlap === undefined ? -1 : overlap); }
  /** -1 adaptive (default), 0 never, r >= 1: the tail kernel takes the live paths over after wavefront round r */
  setTail(round) { addon.setTail(this._target, round === undefined ? -1 : round); }
  /** drawCamera + drawTracer ticks are recorded and run as batches at the next read-out (default, include/fspt.h);
   *  false: every drawTracer executes at once */
  setDeferred(on) { addon.setDeferred(this._target, on !== false); }
  /** HIP event pairs around every kernel launch (per-kernel timing for measurement hosts; ~1.3 % of a 20-tick batch): on by default */
  setStageTiming(on) { addon.setStageTiming(this._target, on !== false); }
  /** cap / query the wavefront path state (include/fspt.h: fspt_target_set_memory_limit) and pre-allocate it */
  setMemoryLimit(bytes) { addon.setMemoryLimit(this._target, bytes || 0); }
  pathStateBytes() { return addon.pathStateBytes(this._target); }
  prepare() { addon.prepare(this._target); }
  enableCounters(on) { addon.enableCounters(this._target, !!on); }
  counters() { return addon.counters(this._target); }
  /** Recorded (deferred) ticks are executed first: fspt_target_destroy itself drops them (it never writes to a
   *  caller-owned accumulator, include/fspt.h).  With a renderAsync in flight close() waits for it and returns a
   *  Promise; otherwise it is synchronous.  (A tracer that is simply dropped is cleaned up by the handles' finalizers.) */
  close() {
    if (this._inflight) return this._inflight.then(() => this.close());
    if (this._target) { try { addon.sync(this._target); } finally { addon.targetDestroy(this._target); addon.sceneDestroy(this._scene); this._target = null; this._scene = null; } }
    return undefined;
  }
}

/** The same frame driver over several GPUs of the node from this one JS thread (include/fspt.h: fspt_multi_*):
 *  every device traces every devices.length-th 32x32 tile, nothing moves between devices while rendering, and
 *  readRadiance() / drawQuad() gather the tiles onto devices[0] with peer-to-peer copies.  Bit-identical to one GPU. */
class MultiPathTracer {
  constructor(scene, width, height, devices) {
    this.resolution = [width, height];
    this.devices = devices && devices.length ? devices.slice() : [0];
    this._multi = addon.multiCreate(scene, this.devices, width, height);
    this.fovScale = 0.5; this.envTheta = 0; this.dir = [0, 0, -1]; this.eye = [0, 0, 2];
    this.lensFeatures = [1 - 1 / 2.0, 0.02];
    this.numBounces = 4;
    this.pingpong = 0;
    this._rng = new BigUint64Array([1n]);
  }
  seed(s) { this._rng[0] = BigInt(s); }
  _randBase() { return addon.randBaseNext(this._rng); }
  _params() { return { P: this.eye, I: this.dir, fovScale: this.fovScale, lens: this.lensFeatures, envTheta: this.envTheta, numBounces: this.numBounces }; }
  drawCamera(randBase) { addon.multiCamera(this._multi, this.eye, this.dir, this.fovScale, this.lensFeatures, randBase === undefined ? this._randBase() : randBase); }
  drawTracer(i, randBase) { addon.multiTrace(this._multi, i, randBase === undefined ? this._randBase() : randBase, this.envTheta, this.numBounces); }
  tick() { this.drawCamera(); this.drawTracer(this.pingpong); this.pingpong++; }
  _advance(nTicks) { for (let k = 0; k < 2 * nTicks; k++) this._randBase(); this.pingpong += nTicks; }
  render(nTicks) { addon.multiRender(this._multi, this._params(), this.pingpong, nTicks, this._rng[0]); this._advance(nTicks); }
  /** as PathTracer.renderAsync: other calls throw Error('render in flight') until it settles; close() waits */
  renderAsync(nTicks) {
    const p = addon.multiRenderAsync(this._multi, this._params(), this.pingpong, nTicks, this._rng[0]);
    this._advance(nTicks);
    const settled = p.then(() => {}, () => {});
    this._inflight = settled;
    settled.then(() => { if (this._inflight === settled) this._inflight = null; });
    return p;
  }
  /** per device [render, pack, transfer, scatter] ms of the most recent render + read-out (fspt_multi_last_stage_ms; -1 = did not run) */
  stageMs() {
    const flat = addon.multiLastStageMs(this._multi, this.devices.length), out = [];
    for (let i = 0; i < this.devices.length; i++) out.push(Array.from(flat.subarray(4 * i, 4 * i + 4)));
    return out;
  }
  clear() { addon.multiClear(this._multi); this.pingpong = 0; }
  sync() { addon.multiSync(this._multi); }
  /** the read-out exchange (include/fspt_multi.h): 'peer' (hipMemcpyPeerAsync of the packed tiles, default), 'rccl_gather'
   *  (ncclSend / ncclRecv of the same tiles), 'rccl_reduce' (ncclReduce(SUM) of own-tiles-only frames); RCCL needs distinct devices */
  setExchange(mode) {
    const codes = { peer: 0, rccl_gather: 1, rccl_reduce: 2 };
    if (codes[mode] === undefined) throw new Error("unknown exchange '" + mode + "' (want " + Object.keys(codes).join(', ') + ')');
    addon.multiSetExchange(this._multi, codes[mode]);
  }
  exchange() { return addon.multiGetExchange(this._multi); }
  readRadiance(out) {
    out = out || new Float32Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('readRadiance: need W*H*4 floats');
    return addon.multiReadRadiance(this._multi, out);
  }
  drawQuad(exposure, saturation, denoise, maxSigma, out) {
    out = out || new Uint8Array(this.resolution[0] * this.resolution[1] * 4);
    if (out.length !== this.resolution[0] * this.resolution[1] * 4) throw new RangeError('drawQuad: need W*H*4 bytes');
    return addon.multiDraw(this._multi, exposure === undefined ? 1 : exposure, saturation === undefined ? 1 : saturation,
      !!denoise, maxSigma === undefined ? 3 : maxSigma, out);
  }
  setPipeline(name, batch) {
    const code = pipelineCode(name);
    for (let i = 0; i < this.devices.length; i++) addon.setPipeline(addon.multiTarget(this._multi, i), code, batch || 0);
  }
  /** PathTracer.setCameraModel on every device's target (a ray depends on its pixel only) */
  setCameraModel(params) {
    const args = cameraModelArgs(params);
    for (let i = 0; i < this.devices.length; i++) addon.setCameraModel(addon.multiTarget(this._multi, i), ...args);
  }
  close() {
    if (this._inflight) return this._inflight.then(() => this.close());
    if (this._multi) { addon.multiDestroy(this._multi); this._multi = null; }
    return undefined;
  }
}

// memory later scenes may spend on interleaved material textures (fspt_set_texture_interleave_budget; results do not depend on it)
function setTextureInterleaveBudget(bytes) { addon.setTextureInterleaveBudget(bytes); }

module.exports = { addon, setTextureInterleaveBudget, jpegEncode, pngEncode, pngFilteredEval, exrEncode, matteHash, matteManifest, skyGenerate, envBinsGpu, atlasPackGpu, SKY_DEFAULTS, MultiPathTracer, AtlasLayers, resolveMaterial, readMtl, mergeSceneProps, resampleImage, packReferenceScene, buildScene,
  PathTracer, saveBlob, loadBlob };
