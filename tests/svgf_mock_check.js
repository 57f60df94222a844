'use strict';
// Driven by tests/test_svgf_cpu.py: node svgf_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's variance-guidance calls on the mock library: the mode and the parameters reach the library (defaults as
// NULL), a call with the mode off is the library's FSPT_E_STATE, bad arrays are refused before it, the target handle is
// guarded while a renderAsync runs, wrong and destroyed handles are refused.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  out.off = thrown(() => pt.temporalDenoiseVariance());
  pt.temporalSetMoments();
  const d1 = pt.temporalDenoiseVariance();
  out.d1 = Array.from(d1.slice(0, 6)); out.d1_type = d1.constructor.name; out.d1_len = d1.length;
  out.d2 = Array.from(pt.temporalDenoiseVariance({ iterations: 3, sigmaColor: 2.5 }).slice(0, 6));
  const own = new Float32Array(24);
  out.same_buffer = pt.temporalDenoiseVariance(null, own) === own;
  out.short_out = thrown(() => pt.temporalDenoiseVariance(null, new Float32Array(8)));
  out.bad_iterations = thrown(() => pt.temporalDenoiseVariance({ iterations: 2.5 }));
  out.bad_sigma = thrown(() => pt.temporalDenoiseVariance({ sigmaDepth: 0 }));
  pt.temporalSetMoments(false);
  out.off_again = thrown(() => pt.temporalDenoiseVariance());
  pt.temporalSetMoments(true);
  const scene = pt._scene, target = pt._target;
  out.addon_len = thrown(() => addon.temporalDenoiseVariance(target, null, new Float32Array(8)));
  out.no_readback = addon.temporalDenoiseVariance(target, null, null) === undefined;
  out.scene_as_target = [thrown(() => addon.temporalSetMoments(scene, true)), thrown(() => addon.temporalDenoiseVariance(scene, null, null))];
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.temporalSetMoments(true)), thrown(() => pt.temporalDenoiseVariance())];
  await job;
  out.after = thrown(() => pt.temporalDenoiseVariance());
  out.sets = pt.temporalDenoiseVariance()[5];
  await pt.close();
  out.closed = [thrown(() => addon.temporalSetMoments(target, true)), thrown(() => addon.temporalDenoiseVariance(target, null, null))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
