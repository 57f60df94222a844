'use strict';
// Driven by tests/test_temporal_cpu.py: node temporal_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's temporal calls on the mock library: parameters reach the library (defaults as NULL), bad ones are refused
// before it, the scene and target handles are guarded while a renderAsync runs, wrong and destroyed handles are refused.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  pt.fovScale = 0.75;
  out.draw_before = thrown(() => pt.temporalDraw());
  const h1 = pt.temporalAccumulate();
  out.h1 = Array.from(h1.slice(0, 7)); out.h1_type = h1.constructor.name; out.h1_len = h1.length;
  pt.motionBegin(); pt.motionBegin();
  const h2 = pt.temporalAccumulate({ alpha: 0.25, maxHistory: 8 });
  out.h2 = Array.from(h2.slice(0, 7));
  pt.motionEnd();
  const own = new Float32Array(24);
  out.same_buffer = pt.temporalAccumulate(null, own) === own;
  out.h3 = Array.from(own.slice(4, 6));
  for (const [k, o] of Object.entries({ alpha: { alpha: 1.5 }, history: { maxHistory: 0 }, depth: { depthTol: -1 }, normal: { normalCos: 2 }, nan: { alpha: NaN }, unknown: { sigma: 1 } }))
    out['bad_' + k] = thrown(() => pt.temporalAccumulate(o));
  out.short_out = thrown(() => pt.temporalAccumulate(null, new Float32Array(8)));
  out.no_readback = pt.temporalAccumulate(null, null) === undefined;
  out.calls_after_refused = pt.temporalAccumulate()[4];
  out.denoise = Array.from(pt.temporalDenoise({ iterations: 3 }).slice(0, 1));
  out.denoise_default = Array.from(pt.temporalDenoise().slice(0, 1));
  out.draw = Array.from(pt.temporalDraw(1.2, 0.9, true).slice(0, 3));
  out.draw_short = thrown(() => pt.temporalDraw(1, 1, false, new Uint8Array(5)));
  const scene = pt._scene, target = pt._target, cam = { P: pt.eye, I: pt.dir, fovScale: 0.5, lens: pt.lensFeatures, envTheta: 0, numBounces: 4 };
  out.addon_range = thrown(() => addon.temporalAccumulate(target, cam, { alpha: 2 }, null));
  out.addon_len = thrown(() => addon.temporalAccumulate(target, cam, null, new Float32Array(8)));
  out.scene_as_target = thrown(() => addon.temporalAccumulate(scene, cam, null, null));
  out.target_as_scene = thrown(() => addon.sceneMotionBegin(target));
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.temporalAccumulate()), thrown(() => pt.temporalReset()), thrown(() => pt.temporalDenoise()),
    thrown(() => pt.temporalDraw()), thrown(() => pt.motionBegin()), thrown(() => pt.motionEnd())];
  await job;
  out.after = thrown(() => pt.temporalAccumulate());
  pt.temporalReset();
  out.calls_after_reset = pt.temporalAccumulate()[4];
  await pt.close();
  out.closed = [thrown(() => addon.temporalAccumulate(target, cam, null, null)), thrown(() => addon.sceneMotionBegin(scene))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
