'use strict';
// Driven by tests/test_svgf_gpu.py: node svgf_node_check.js <dir with fspt.js> <job dir>
// The JS host's variance-guided frame protocol on the scene arrays the test wrote: temporalSetMoments, then per frame
// render, features, temporalAccumulate; after the second frame (a moved camera) temporalDenoiseVariance and temporalDraw.
// The histories go to h1.bin / h2.bin, the filtered frame to den.bin, its drawing to draw_den.bin.
const fs = require('fs');
const path = require('path');
const F = require(path.join(process.argv[2], 'fspt.js'));
const dir = process.argv[3];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const rd = (name, T) => { const b = fs.readFileSync(path.join(dir, name + '.bin')); return new T(b.buffer, b.byteOffset, b.byteLength / T.BYTES_PER_ELEMENT); };
const wr = (name, a) => fs.writeFileSync(path.join(dir, name + '.bin'), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
const desc = { bvh: rd('bvh', Float32Array), tri: rd('tri', Float32Array), mat: rd('mat', Float32Array), norm: rd('norm', Float32Array),
  uv: rd('uv', Float32Array), atlas: rd('atlas', Uint8Array), atlasRes: job.atlasRes, atlasLayers: job.atlasLayers, env: null, envW: 0,
  envH: 0, bins: rd('bins', Uint32Array), leafSize: job.leafSize };
const pt = new F.PathTracer(desc, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.lens; pt.numBounces = 4;
pt.temporalSetMoments(true);
pt.seed(3);
pt.render(job.n);
pt.features(4, 3);
wr('h1', pt.temporalAccumulate());
pt.eye = job.cam2.P;
pt.clear();
pt.seed(7);
pt.render(job.n);
pt.features(4, 3);
wr('h2', pt.temporalAccumulate());
wr('den', pt.temporalDenoiseVariance({ iterations: 2, sigmaColor: 3 }));
wr('draw_den', pt.temporalDraw(1.2, 0.9, true));
Promise.resolve(pt.close()).then(() => {});
