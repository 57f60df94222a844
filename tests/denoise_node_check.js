'use strict';
// Driven by tests/test_denoise_gpu.py: node denoise_node_check.js <job.json> <out.json>
// The JS host's features / denoise / drawDenoised on a rendered frame, and the renderAsync guard on the three calls.
const fs = require('fs');
const path = require('path');
const F = require(path.join(__dirname, '..', 'fspt_amd', 'js', 'fspt.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const b64 = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength).toString('base64');
const env = { rgbe: Uint8Array.from(Buffer.from(job.env.rgbe_b64, 'base64')), width: job.env.width, height: job.env.height };
const s = F.buildScene(job.props, job.objs, env, 4);
const pt = new F.PathTracer(s, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.cam.lens; pt.numBounces = job.bounces;
pt.seed(job.seed);
pt.render(job.ticks);
pt.features(job.samples, job.feature_seed);
out.denoised = b64(pt.denoise());
out.denoised_k2 = b64(pt.denoise({ iterations: 2, sigmaColor: 2.0 }));
out.drawn = b64(pt.drawDenoised(1.5, 0.8));
const thrown = (f) => { try { f(); return null; } catch (e) { return String(e.message); } };
const p = pt.renderAsync(2);
out.during = { features: thrown(() => pt.features(1, 1)), denoise: thrown(() => pt.denoise()),
  drawDenoised: thrown(() => pt.drawDenoised()) };
p.then(() => {
  out.after = thrown(() => pt.denoise());
  const c = pt.close();
  return Promise.resolve(c).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)));
}).catch((e) => { console.error(e); process.exit(1); });
