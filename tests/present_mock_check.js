'use strict';
// Driven by tests/test_present_cpu.py: node present_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's present() on the mock library: the buffer-length RangeError, the call through the addon, and the
// renderAsync guard.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
out.short = thrown(() => pt.present(1, 1, false, 3, new Uint8Array(3 * 2 * 4 - 1)));
out.missing = thrown(() => pt.present(1, 1, false, 3));
const frame = new Uint8Array(3 * 2 * 4);
out.ticks = pt.present(1, 1, false, 3, frame, 1);
out.frame = Array.from(frame);
const p = pt.renderAsync(1);
out.during = thrown(() => pt.present(1, 1, false, 3, frame));
p.then(() => {
  out.after = thrown(() => pt.present(1, 1, false, 3, frame));
  return Promise.resolve(pt.close());
}).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)))
  .catch((e) => { console.error(e); process.exit(1); });
