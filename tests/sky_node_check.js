'use strict';
// Driven by tests/test_sky_gpu.py: node sky_node_check.js <dir with fspt.js> <job dir>
// The JS host's render(), updateSky(), clear(), render() on the scene arrays the test wrote: the radiance goes to
// <job dir>/out.bin; then updateEnvironmentAuto() of skyGenerate()'s bytes, whose radiance goes to out2.bin, the bytes to
// sky.bin and envBinsGpu() of them to bins.bin.
const fs = require('fs');
const path = require('path');
const F = require(path.join(process.argv[2], 'fspt.js'));
const dir = process.argv[3];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const rd = (name, T) => { const b = fs.readFileSync(path.join(dir, name + '.bin')); const c = new Uint8Array(b); return new T(c.buffer, 0, c.byteLength / T.BYTES_PER_ELEMENT); };
const desc = { bvh: rd('bvh', Float32Array), tri: rd('tri', Float32Array), mat: rd('mat', Float32Array), norm: rd('norm', Float32Array),
  uv: rd('uv', Float32Array), atlas: rd('atlas', Uint8Array), atlasRes: job.atlasRes, atlasLayers: job.atlasLayers, env: rd('env', Uint8Array),
  envW: job.envW, envH: job.envH, bins: rd('bins', Uint32Array), leafSize: job.leafSize };
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
pt.updateSky(job.sky);
frame('out.bin');
const sky = F.skyGenerate(job.sky2, 0);
fs.writeFileSync(path.join(dir, 'sky.bin'), Buffer.from(sky.rgbe.buffer, sky.rgbe.byteOffset, sky.rgbe.byteLength));
const bins = F.envBinsGpu(sky.rgbe, sky.width, sky.height, 0);
fs.writeFileSync(path.join(dir, 'bins.bin'), Buffer.from(bins.buffer, bins.byteOffset, bins.byteLength));
pt.updateEnvironmentAuto({ env: sky.rgbe, envW: sky.width, envH: sky.height });
frame('out2.bin');
Promise.resolve(pt.close()).then(() => {});
