'use strict';
// Driven by tests/test_texpack_gpu.py: node texpack_node_check.js <dir with fspt.js> <job dir>
// The JS host on the description and the scene arrays the test wrote: atlasPackGpu()'s bytes go to <job dir>/atlas.bin; then
// render(), updateTextures(), clear(), render() - the radiance goes to out.bin - and patchTextures(), whose radiance goes to
// out2.bin.
const fs = require('fs');
const path = require('path');
const F = require(path.join(process.argv[2], 'fspt.js'));
const dir = process.argv[3];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const rd = (name, T) => { const b = fs.readFileSync(path.join(dir, name + '.bin')); const c = new Uint8Array(b); return new T(c.buffer, 0, c.byteLength / T.BYTES_PER_ELEMENT); };
const desc = { bvh: rd('bvh', Float32Array), tri: rd('tri', Float32Array), mat: rd('mat', Float32Array), norm: rd('norm', Float32Array),
  uv: rd('uv', Float32Array), atlas: rd('atlas0', Uint8Array), atlasRes: job.atlasRes, atlasLayers: job.atlasLayers, env: rd('env', Uint8Array),
  envW: job.envW, envH: job.envH, bins: rd('bins', Uint32Array), leafSize: job.leafSize };
const images = (list) => list.map((im) => ({ width: im.w, height: im.h, data: rd(im.file, Uint8Array) }));
const textures = { res: job.textures.res, images: images(job.textures.images), layers: job.textures.layers };
const atlas = F.atlasPackGpu(textures, 0);
fs.writeFileSync(path.join(dir, 'atlas.bin'), Buffer.from(atlas.buffer, atlas.byteOffset, atlas.byteLength));
const pt = new F.PathTracer(desc, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.lens; pt.numBounces = 4;
const frame = (name) => {
  pt.clear();
  pt.seed(7);
  pt.render(job.n);
  const out = new Float32Array(job.W * job.H * 4);
  pt.readRadiance(out);
  fs.writeFileSync(path.join(dir, name), Buffer.from(out.buffer));
};
pt.seed(3);
pt.render(2);
pt.updateTextures({ mat: rd('mat1', Float32Array), uv: rd('uv1', Float32Array), textures });
frame('out.bin');
pt.patchTextures({ layerIds: job.patch.ids, layers: job.patch.layers, images: images(job.patch.images), res: job.textures.res });
frame('out2.bin');
Promise.resolve(pt.close()).then(() => {});
