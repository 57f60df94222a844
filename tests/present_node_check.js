'use strict';
// Driven by tests/test_present_gpu.py: node present_node_check.js <job.json> <out.json>
// The JS host's tick() + present() loop on the fixture scene, and the renderAsync guard on present.
const fs = require('fs');
const path = require('path');
const F = require(path.join(__dirname, '..', 'fspt_amd', 'js', 'fspt.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { frames: [] };
const b64 = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength).toString('base64');
const env = { rgbe: Uint8Array.from(Buffer.from(job.env.rgbe_b64, 'base64')), width: job.env.width, height: job.env.height };
const s = F.buildScene(job.props, job.objs, env, 4);
const pt = new F.PathTracer(s, job.W, job.H, 0);
pt.eye = job.cam.P; pt.dir = job.cam.I; pt.fovScale = job.cam.fov_scale; pt.envTheta = job.cam.env_theta;
pt.lensFeatures = job.cam.lens; pt.numBounces = job.bounces;
pt.seed(job.seed);
const frame = new Uint8Array(job.W * job.H * 4);
for (let k = 0; k < job.ticks; k++) {
  pt.tick();
  const n = pt.present(1.3, 0.9, false, 3, frame);
  out.frames.push([n, n ? b64(frame) : null]);
}
const thrown = (f) => { try { f(); return null; } catch (e) { return String(e.message); } };
const p = pt.renderAsync(2);
out.during = thrown(() => pt.present(1, 1, false, 3, frame));
p.then(() => {
  out.after = thrown(() => pt.present(1, 1, false, 3, frame));
  const c = pt.close();
  return Promise.resolve(c).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)));
}).catch((e) => { console.error(e); process.exit(1); });
