'use strict';
// Driven by tests/test_lights_cpu.py: node lights_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's setLights() on the mock library: argument checks, the call through the addon, the renderAsync guard and
// a closed handle.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
out.mode = thrown(() => pt.setLights('area', 0.5));
out.fraction = thrown(() => pt.setLights('emitters', 0));
out.nan = thrown(() => pt.setLights('emitters', NaN));
out.ok = thrown(() => { pt.setLights('emitters', 0.25); pt.setLights(); pt.setLights('off', 1); });
const target = pt._target, scene = pt._scene;
out.wrong_kind = thrown(() => addon.setLights(scene, 1, 0.5));
const p = pt.renderAsync(1);
out.during = thrown(() => pt.setLights('emitters', 0.5));
p.then(() => {
  out.after = thrown(() => pt.setLights('emitters', 0.75));
  return Promise.resolve(pt.close());
}).then(() => {
  out.destroyed = thrown(() => addon.setLights(target, 1, 0.5));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}).catch((e) => { console.error(e); process.exit(1); });
