'use strict';
// Driven by tests/test_bloom_cpu.py: node bloom_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's bloom calls on the mock library: the mode and the three parameters reach the library (omitted ones as the
// defaults), bad parameters are refused (unknown names, non-numbers and fractional levels before the library, ranges by it),
// the target handle is guarded while a renderAsync runs, wrong and destroyed handles are refused.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  out.off = pt.bloom;
  pt.setBloom();
  out.defaults = pt.bloom;
  pt.setBloom(true, { intensity: 0.5, levels: 3 });
  out.some = pt.bloom;
  out.unknown = thrown(() => pt.setBloom(true, { intensify: 0.5 }));
  out.not_a_number = thrown(() => pt.setBloom(true, { intensity: '0.5' }));
  out.fraction = thrown(() => pt.setBloom(true, { levels: 2.5 }));
  out.bad = [thrown(() => pt.setBloom(true, { intensity: -0.1 })), thrown(() => pt.setBloom(true, { intensity: 1.5 })), thrown(() => pt.setBloom(true, { intensity: NaN })),
    thrown(() => pt.setBloom(true, { scatter: -1 })), thrown(() => pt.setBloom(true, { scatter: Infinity })), thrown(() => pt.setBloom(true, { levels: 0 })),
    thrown(() => pt.setBloom(true, { levels: 9 })), thrown(() => pt.setBloom(true, { levels: -1 }))];
  out.kept = pt.bloom;
  const scene = pt._scene, target = pt._target;
  out.scene_as_target = thrown(() => addon.bloom(scene));
  out.too_few = thrown(() => addon.setBloom(target, true, 0.05));
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.setBloom(true)), thrown(() => pt.bloom)];
  await job;
  out.after = thrown(() => pt.setBloom(true));
  pt.setBloom(false);
  out.off_again = pt.bloom;
  await pt.close();
  out.closed = thrown(() => addon.setBloom(target, true, 0.05, 0.7, 6));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
