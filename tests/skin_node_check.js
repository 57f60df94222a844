'use strict';
// Driven by tests/test_skin_node.py: node skin_node_check.js <dir with fspt.js> <job dir>
// The JS host's render(), setSkin(), updateSkin(), clear(), render() on the scene arrays the test wrote; the radiance after
// the frame goes to <job dir>/out.bin.
const fs = require('fs');
const path = require('path');
const F = require(path.join(process.argv[2], 'fspt.js'));
const dir = process.argv[3];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'meta.json'), 'utf8'));
const rd = (name, T) => { const b = fs.readFileSync(path.join(dir, name + '.bin')); const c = new Uint8Array(b); return new T(c.buffer, 0, c.byteLength / T.BYTES_PER_ELEMENT); };
const desc = { bvh: rd('bvh', Float32Array), tri: rd('tri', Float32Array), mat: rd('mat', Float32Array), norm: rd('norm', Float32Array),
  uv: rd('uv', Float32Array), atlas: rd('atlas', Uint8Array), atlasRes: job.atlasRes, atlasLayers: job.atlasLayers, env: null, envW: 0, envH: 0,
  bins: rd('bins', Uint32Array), leafSize: job.leafSize };
const pt = new F.PathTracer(desc, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.lens; pt.numBounces = 4;
pt.seed(3);
pt.render(2);
pt.setSkin({ joints: rd('joints', Uint16Array), weights: rd('weights', Float32Array), tri: desc.tri, norm: desc.norm,
  morph: rd('morph', Float32Array), morphNorm: rd('morph_norm', Float32Array), nJoints: job.nJoints });
pt.updateSkin(rd('xf', Float32Array), rd('mw', Float32Array));
pt.clear();
pt.seed(7);
pt.render(job.n);
const out = new Float32Array(job.W * job.H * 4);
pt.readRadiance(out);
fs.writeFileSync(path.join(dir, 'out.bin'), Buffer.from(out.buffer));
Promise.resolve(pt.close()).then(() => {});
