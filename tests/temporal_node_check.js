'use strict';
// Driven by tests/test_temporal_gpu.py: node temporal_node_check.js <dir with fspt.js> <job dir>
// The JS host's frame protocol on the scene arrays the test wrote: render, temporalAccumulate; then motionBegin,
// updateGeometry, clear, render, temporalAccumulate from a moved camera; features, temporalDenoise, temporalDraw.  The
// two histories go to h1.bin / h2.bin, the denoised frame to den.bin, the drawn frames to draw.bin / draw_den.bin.
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
pt.seed(3);
pt.render(job.n);
wr('h1', pt.temporalAccumulate());
pt.motionBegin();
pt.updateGeometry(rd('tri2', Float32Array), rd('norm2', Float32Array));
pt.eye = job.cam2.P;
pt.clear();
pt.seed(7);
pt.render(job.n);
wr('h2', pt.temporalAccumulate({ maxHistory: 5, depthTol: 0.1 }));
pt.features(4, 3);
wr('den', pt.temporalDenoise({ iterations: 2 }));
wr('draw_den', pt.temporalDraw(1.2, 0.9, true));
wr('draw', pt.temporalDraw(1.2, 0.9, false));
Promise.resolve(pt.close()).then(() => {});
