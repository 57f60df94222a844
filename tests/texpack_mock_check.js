'use strict';
// Driven by tests/test_texpack_cpu.py: node texpack_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's atlasPackGpu() / updateTextures() / patchTextures() / AtlasLayers.packDesc() on the mock library: argument
// checks in fspt.js and in the addon, every refusal of the library, the calls through the addon, the renderAsync guard on the
// scene handle, wrong and destroyed handles.  sahCost() reads the mock's count of what arrived.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const img = (w, h, src) => ({ width: w, height: h, data: new Uint8Array(w * h * 4), currentSrc: src });
const good = (res) => ({ res: res === undefined ? 4 : res, images: [img(3, 5, 'a'), img(res === undefined ? 4 : res, res === undefined ? 4 : res, 'b')],
  layers: [{ kind: 'color', color: [0.1, 0.2, 0.3] }, { kind: 'image', image: 0, corrected: true, swizzle: [0, 2, 1, 3] }, { kind: 'pixels', image: 1 }] });
const spoil = (f) => { const d = good(); f(d); return d; };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const mat = new Float32Array(24), uv = new Float32Array(12);
  // packDesc: the first layer twice (index 0 is never found again), flags as the images carry them at the end
  const pk = new F.AtlasLayers(2048), a = img(16, 8, 'a.png'), b = img(5, 12, 'b.png');
  out.ids = [pk.image(a, true), pk.colour([0.5, 0.25, 1.5]), pk.image(a, false), pk.image(b, false), pk.image(b, true)];
  a.swizzle = [0, 2, 1, 3];
  const pd = pk.packDesc();
  out.pack_desc = { res: pd.res, n_images: pd.images.length, same: pd.images[0] === a, layers: pd.layers };
  out.describe = pk.describe();
  const atlas = F.atlasPackGpu(good(), 1);
  out.atlas = [atlas.length, Array.from(atlas.slice(0, 4)), Array.from(atlas.slice(64, 68)), Array.from(atlas.slice(128, 132))];
  out.pixels_device = Array.from(pk.pixels({ device: 2 }).slice(0, 4));
  out.c0 = pt.sahCost();
  out.patch_no_atlas = thrown(() => pt.patchTextures({ layerIds: [0], layers: [good().layers[0]], res: 4 }));   // FSPT_E_STATE: nothing retained
  pt.updateTextures({ mat, uv, textures: good() });
  out.c1 = pt.sahCost();
  pt.updateTextures({ mat, textures: pk });
  out.c2 = pt.sahCost();
  out.patch_other_res = thrown(() => pt.patchTextures({ layerIds: [1], layers: [good().layers[0]], res: 4 }));
  pt.patchTextures({ layerIds: [3, 0], layers: [good().layers[0], { kind: 'image', image: 0 }], images: [img(2, 2, 'c')], res: 12 });
  out.c3 = pt.sahCost();
  // fspt.js
  out.no_object = [thrown(() => pt.updateTextures()), thrown(() => pt.patchTextures()), thrown(() => F.atlasPackGpu())];
  out.short_mat = thrown(() => pt.updateTextures({ mat: new Float32Array(12), textures: good() }));
  out.short_uv = thrown(() => pt.updateTextures({ mat, uv: new Float32Array(6), textures: good() }));
  out.no_textures = thrown(() => pt.updateTextures({ mat }));
  out.short_image = thrown(() => F.atlasPackGpu(spoil((d) => { d.images[0].data = new Uint8Array(8); })));
  out.u16_image = thrown(() => F.atlasPackGpu(spoil((d) => { d.images[0].data = new Uint16Array(60); })));
  out.clamped_image = thrown(() => F.atlasPackGpu(spoil((d) => { d.images[0].data = new Uint8ClampedArray(60); })));
  out.res_float = thrown(() => F.atlasPackGpu(spoil((d) => { d.res = 2.5; })));
  out.short_swizzle = thrown(() => F.atlasPackGpu(spoil((d) => { d.layers[1].swizzle = [0, 1, 2]; })));
  out.short_colour = thrown(() => F.atlasPackGpu(spoil((d) => { d.layers[0].color = [1, 2]; })));
  out.image_float = thrown(() => F.atlasPackGpu(spoil((d) => { d.layers[1].image = 0.5; })));
  out.ids_count = thrown(() => pt.patchTextures({ layerIds: [0, 1], layers: [good().layers[0]], res: 12 }));
  out.ids_type = thrown(() => pt.patchTextures({ layerIds: [0.5], layers: [good().layers[0]], res: 12 }));
  // the library's refusals, through fspt.js
  const lib = {
    res_0: (d) => { d.res = 0; }, res_16385: (d) => { d.res = 16385; }, no_layers: (d) => { d.layers = []; },
    w_0: (d) => { d.images[0] = img(0, 5, 'z'); }, h_16385: (d) => { d.images[0] = img(1, 16385, 'z'); },
    image_index: (d) => { d.layers[1].image = 2; }, swizzle_4: (d) => { d.layers[1].swizzle = [0, 1, 4, 3]; }, swizzle_nan: (d) => { d.layers[1].swizzle = [0, NaN, 1, 3]; },
    kind_3: (d) => { d.layers[1].kind = 3; }, kind_word: (d) => { d.layers[1].kind = 'cube'; }, colour_nan: (d) => { d.layers[0].color = [0, NaN, 0]; },
    colour_inf: (d) => { d.layers[0].color = [Infinity, 0, 0]; }, pixels_not_res: (d) => { d.layers[2].image = 0; } };
  out.refused_by_library = {};
  for (const k of Object.keys(lib)) out.refused_by_library[k] = [thrown(() => F.atlasPackGpu(spoil(lib[k]))), thrown(() => pt.updateTextures({ mat, textures: spoil(lib[k]) }))];
  out.patch_refused = [thrown(() => pt.patchTextures({ layerIds: [4], layers: [good().layers[0]], res: 12 })),        // the mock retains 4 layers
    thrown(() => pt.patchTextures({ layerIds: [1, 1], layers: [good().layers[0], good().layers[0]], res: 12 }))];
  out.cost_after_refused = pt.sahCost();
  // the addon on its own
  const scene = pt._scene, target = pt._target, k = { images: [new Uint8Array(60)], dims: Uint32Array.of(3, 5), layers: Float32Array.of(1, 0, 0, 0, 0, 0, 0, 1, 2, 3) };
  out.addon_dims = thrown(() => addon.atlasPackGpu(0, k.images, Uint32Array.of(3, 5, 1), k.layers, 4));
  out.addon_image_len = thrown(() => addon.atlasPackGpu(0, [new Uint8Array(56)], k.dims, k.layers, 4));
  out.addon_layers_len = thrown(() => addon.atlasPackGpu(0, k.images, k.dims, new Float32Array(9), 4));
  out.addon_images_type = thrown(() => addon.atlasPackGpu(0, new Uint8Array(60), k.dims, k.layers, 4));
  out.addon_image_type = thrown(() => addon.atlasPackGpu(0, [new Float32Array(15)], k.dims, k.layers, 4));
  out.addon_mat = thrown(() => addon.sceneUpdateTextures(scene, 2, new Float32Array(12), null, k.images, k.dims, k.layers, 4));
  out.addon_ids = thrown(() => addon.scenePatchTextures(scene, Uint32Array.of(0, 1), k.images, k.dims, k.layers, 12));
  out.target_as_scene = [thrown(() => addon.sceneUpdateTextures(target, 2, mat, null, k.images, k.dims, k.layers, 4)),
    thrown(() => addon.scenePatchTextures(target, Uint32Array.of(0), k.images, k.dims, k.layers, 12))];
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.updateTextures({ mat, textures: good() })), thrown(() => pt.patchTextures({ layerIds: [0], layers: [good().layers[0]], res: 12 }))];
  await job;
  out.after = [thrown(() => pt.updateTextures({ mat, textures: good(12) })), thrown(() => pt.patchTextures({ layerIds: [0], layers: [good().layers[0]], res: 12 }))];
  await pt.close();
  out.closed = [thrown(() => addon.sceneUpdateTextures(scene, 2, mat, null, k.images, k.dims, k.layers, 4)),
    thrown(() => addon.scenePatchTextures(scene, Uint32Array.of(0), k.images, k.dims, k.layers, 12))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
