'use strict';
// Driven by tests/test_lighttable_node.py: node lightbuilder_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's setLightBuilder() / getLightBuilder() on the mock library: argument checks, the calls through the addon,
// the renderAsync guard and a closed handle.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
out.first = pt.getLightBuilder();
out.bad = thrown(() => pt.setLightBuilder('device'));
out.none = thrown(() => pt.setLightBuilder());
out.ok = thrown(() => { pt.setLightBuilder('gpu'); });
out.gpu = pt.getLightBuilder();
out.back = thrown(() => { pt.setLightBuilder('host'); });
out.host = pt.getLightBuilder();
out.addon_bad = thrown(() => addon.sceneSetLightBuilder(pt._scene, 5));
const target = pt._target, scene = pt._scene;
out.wrong_kind = [thrown(() => addon.sceneSetLightBuilder(target, 1)), thrown(() => addon.sceneGetLightBuilder(target))];
const p = pt.renderAsync(1);
out.during = [thrown(() => pt.setLightBuilder('gpu')), thrown(() => pt.getLightBuilder())];
p.then(() => {
  out.after = thrown(() => pt.setLightBuilder('gpu'));
  return Promise.resolve(pt.close());
}).then(() => {
  out.destroyed = [thrown(() => addon.sceneSetLightBuilder(scene, 1)), thrown(() => addon.sceneGetLightBuilder(scene))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}).catch((e) => { console.error(e); process.exit(1); });
