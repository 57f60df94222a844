'use strict';
// Driven by tests/test_clamp_cpu.py: node clamp_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's history-clamp call on the mock library: the mode and the two parameters reach the library (omitted ones as
// the defaults), bad parameters are refused (unknown names and non-numbers before the library, ranges by it), the target
// handle is guarded while a renderAsync runs, wrong and destroyed handles are refused.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const state = () => Array.from(pt.temporalAccumulate().slice(0, 4));
  out.initial = state();
  pt.temporalSetClamp();
  out.defaults = state();
  pt.temporalSetClamp(true, { fastHistory: 8, sigmaScale: 1.5 });
  out.both = state();
  pt.temporalSetClamp(true, { sigmaScale: Infinity });
  out.inf = state();
  pt.temporalSetClamp(false);
  out.off = state();
  out.unknown = thrown(() => pt.temporalSetClamp(true, { fast: 8 }));
  out.not_a_number = thrown(() => pt.temporalSetClamp(true, { sigmaScale: '2' }));
  out.bad = [thrown(() => pt.temporalSetClamp(true, { fastHistory: 0.5 })), thrown(() => pt.temporalSetClamp(true, { fastHistory: Infinity })),
    thrown(() => pt.temporalSetClamp(true, { fastHistory: NaN })), thrown(() => pt.temporalSetClamp(true, { sigmaScale: -1 })),
    thrown(() => pt.temporalSetClamp(true, { sigmaScale: NaN }))];
  out.off_ignores_numbers = thrown(() => pt.temporalSetClamp(false, { sigmaScale: -1 }));
  const scene = pt._scene, target = pt._target;
  out.scene_as_target = thrown(() => addon.temporalSetClamp(scene, true, 16, 2));
  out.too_few = thrown(() => addon.temporalSetClamp(target, true));
  const job = pt.renderAsync(1);
  out.during = thrown(() => pt.temporalSetClamp(true));
  await job;
  out.after = thrown(() => pt.temporalSetClamp(true));
  out.last = state();
  await pt.close();
  out.closed = thrown(() => addon.temporalSetClamp(target, true, 16, 2));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
