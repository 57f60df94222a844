'use strict';
// Driven by tests/test_clamp_gpu.py: node clamp_node_check.js <dir with fspt.js> <job dir>
// The JS host's history clamp on the scene arrays the test wrote: temporalSetClamp with the test's parameters, then three
// frames (render, temporalAccumulate) with a camera move before the second and a turned environment before the third.
// The histories go to h1.bin / h2.bin / h3.bin, the drawing of the last to draw.bin.
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
pt.temporalSetClamp(true, { fastHistory: job.fastHistory, sigmaScale: job.sigmaScale });
pt.seed(3);
pt.render(job.n);
wr('h1', pt.temporalAccumulate());
pt.eye = job.cam2.P;
pt.clear();
pt.seed(7);
pt.render(job.n);
wr('h2', pt.temporalAccumulate());
pt.envTheta = job.cam.env_theta + 1.5;
pt.clear();
pt.seed(9);
pt.render(job.n);
wr('h3', pt.temporalAccumulate());
wr('draw', pt.temporalDraw(1.2, 0.9, false));
Promise.resolve(pt.close()).then(() => {});
