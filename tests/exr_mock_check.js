'use strict';
// Driven by tests/test_exr_cpu.py: node exr_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's drawExr / exrEncode on the mock library: the argument checks, the calls through the addon, the reusable
// buffer sized by the bound, and the renderAsync guard.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
const d = pt.drawExr({ source: 'temporalDenoised', compression: 'zips', float32: true, layers: ['alpha', 'depth'], chunkBytes: 512 });
out.draw = Array.from(d); out.drawIsBuffer = Buffer.isBuffer(d);
out.drawDefault = Array.from(pt.drawExr());
out.badSource = thrown(() => pt.drawExr({ source: 'radiance' }));
out.badCompression = thrown(() => pt.drawExr({ compression: 'piz' }));
out.badLayer = thrown(() => pt.drawExr({ layers: 'alpha,uv' }));
out.badChunk = thrown(() => pt.drawExr({ chunkBytes: 255 }));
pt._exrBuf = new Uint8Array(4);             // too small: replaced by one of the bound
out.grownDraw = Array.from(pt.drawExr({ source: 'denoised', layers: 'alpha,albedo,normal,depth' })); out.grownBytes = pt._exrBuf.length;
const rgba = new Float32Array(5 * 2 * 4), feat = new Float32Array(5 * 2 * 8);
const e = F.exrEncode(rgba, feat, 5, 2, { bottomUp: true, compression: 'none', layers: ['albedo'], chunkBytes: 1024 });
out.encode = Array.from(e); out.encodeIsBuffer = Buffer.isBuffer(e);
out.encodePlain = Array.from(F.exrEncode(rgba, null, 5, 2));
out.encodeShort = thrown(() => F.exrEncode(new Float32Array(5 * 2 * 4 - 1), null, 5, 2));
out.encodeNoFeatures = thrown(() => F.exrEncode(rgba, null, 5, 2, { layers: 'depth' }));
const p = pt.renderAsync(1);
out.duringDraw = thrown(() => pt.drawExr());
p.then(() => {
  out.after = thrown(() => pt.drawExr());
  return Promise.resolve(pt.close());
}).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)))
  .catch((err) => { console.error(err); process.exit(1); });
