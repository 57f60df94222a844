'use strict';
// Driven by tests/test_bloom_gpu.py: node bloom_node_check.js <dir with fspt.js> <job dir>
// The JS host's bloom on the scene arrays the test wrote: setBloom with the test's parameters, a render and a drawQuad; then
// other parameters (the allocation stays) and a second drawQuad; then off and a third.  The drawings go to d1.bin .. d3.bin,
// the three `bloom` records to state.json.
const fs = require('fs');
const path = require('path');
const F = require(path.join(process.argv[2], 'fspt.js'));
const dir = process.argv[3];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const rd = (name, T) => { const b = fs.readFileSync(path.join(dir, name + '.bin')); return new T(b.buffer, b.byteOffset, b.byteLength / T.BYTES_PER_ELEMENT); };
const wr = (name, a) => fs.writeFileSync(path.join(dir, name + '.bin'), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const desc = { bvh: rd('bvh', Float32Array), tri: rd('tri', Float32Array), mat: rd('mat', Float32Array), norm: rd('norm', Float32Array),
  uv: rd('uv', Float32Array), atlas: rd('atlas', Uint8Array), atlasRes: job.atlasRes, atlasLayers: job.atlasLayers,
  env: job.envW ? rd('env', Uint8Array) : null, envW: job.envW, envH: job.envH, bins: rd('bins', Uint32Array), leafSize: job.leafSize };
const pt = new F.PathTracer(desc, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.lens; pt.numBounces = 4;
pt.setBloom(true, job.params);
pt.seed(3);
pt.render(job.n);
wr('d1', pt.drawQuad(1.2, 0.9, false, 3.0));
const s1 = pt.bloom;
pt.setBloom(true, job.params2);
wr('d2', pt.drawQuad(1.2, 0.9, true, 2.0));
const s2 = pt.bloom;
pt.setBloom(false);
wr('d3', pt.drawQuad(1.2, 0.9, false, 3.0));
fs.writeFileSync(path.join(dir, 'state.json'), JSON.stringify([s1, s2, pt.bloom]));
Promise.resolve(pt.close()).then(() => {});
