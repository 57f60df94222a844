'use strict';
// Driven by tests/test_rebuild_cpu.py: node rebuild_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's rebuildGeometry() on the mock library: argument checks, the call through the addon and the order it
// returns, the renderAsync guard on the scene handle, wrong and destroyed handles.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const tri = new Float32Array(18), norm = new Float32Array(54);
  out.cost0 = pt.sahCost();
  const o1 = pt.rebuildGeometry(tri);
  out.order = Array.from(o1);
  out.order_type = o1.constructor.name;
  out.cost1 = pt.sahCost();
  pt.rebuildGeometry(tri, norm);
  pt.rebuildGeometry(tri, null);
  out.cost2 = pt.sahCost();
  out.short_tri = thrown(() => pt.rebuildGeometry(new Float32Array(9)));
  out.f64_tri = thrown(() => pt.rebuildGeometry(new Float64Array(18)));
  out.short_norm = thrown(() => pt.rebuildGeometry(tri, new Float32Array(27)));
  out.cost_after_refused = pt.sahCost();
  const scene = pt._scene, target = pt._target;
  out.addon_len = thrown(() => addon.sceneRebuildGeometry(scene, 3, tri, null));
  out.addon_type = thrown(() => addon.sceneRebuildGeometry(scene, 2, [0, 1], null));
  out.target_as_scene = thrown(() => addon.sceneRebuildGeometry(target, 2, tri, null));
  const job = pt.renderAsync(1);
  out.during = thrown(() => pt.rebuildGeometry(tri));
  await job;
  out.after = thrown(() => pt.rebuildGeometry(tri));
  await pt.close();
  out.closed = thrown(() => addon.sceneRebuildGeometry(scene, 2, tri, null));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
