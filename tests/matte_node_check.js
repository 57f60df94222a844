'use strict';
// Driven by tests/test_matte_gpu.py: node matte_node_check.js <job.json> <out.json>
// The JS host's setMatte / mattes / readMattes / mattesLost / drawExr with the matte layers / exrEncode({mattes}) on a rendered
// frame, and the renderAsync guard.
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
const n = s.tri.length / 9;
out.n_tris = n;
const labels = (m) => Int32Array.from({ length: n }, (_, k) => k % m);
pt.setMatte('object', labels(job.object_names.length), job.object_names);
pt.setMatte('material', labels(job.material_names.length), job.material_names);
pt.seed(job.seed);
pt.render(job.ticks);
pt.mattes(job.samples, job.matte_seed);
out.object = b64(pt.readMattes('object', true));
out.material = b64(pt.readMattes('material', true));
const o = pt.readMattes('object');
out.object_ids = b64(o.ids); out.object_cov = b64(o.coverage);
out.lost = [pt.mattesLost('object'), pt.mattesLost('material')];
const file = pt.drawExr({ layers: ['alpha', 'crypto_object', 'crypto_material'], compression: 'zips' });
out.file = file.toString('base64');
const rgba = pt.readRadiance();
out.encoded = F.exrEncode(rgba, null, job.W, job.H, { bottomUp: true, layers: 'alpha,crypto_object,crypto_material', compression: 'zips',
  mattes: { object: { ranks: pt.readMattes('object', true), manifest: F.matteManifest(job.object_names) },
    material: { ranks: pt.readMattes('material', true), manifest: F.matteManifest(job.material_names) } } }).toString('base64');
const thrown = (f) => { try { f(); return null; } catch (e) { return String(e.message); } };
const p = pt.renderAsync(2);
out.during = { mattes: thrown(() => pt.mattes(1, 1)), readMattes: thrown(() => pt.readMattes('object')), drawExr: thrown(() => pt.drawExr({ layers: 'crypto_object' })) };
p.then(() => {
  out.after = thrown(() => pt.mattes(1, 1));
  const c = pt.close();
  return Promise.resolve(c).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)));
}).catch((e) => { console.error(e); process.exit(1); });
