'use strict';
// Driven by tests/test_appearance_cpu.py: node appearance_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's updateMaterials() / updateEnvironment() on the mock library: argument checks, the calls through the addon,
// the renderAsync guard on the scene handle, wrong and destroyed handles.  sahCost() reads the mock's count of what arrived.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const mat = new Float32Array(24), uv = new Float32Array(12), atlas = new Uint8Array(2 * 2 * 3 * 4), env = new Uint8Array(3 * 2 * 4), bins = new Uint32Array(8);
  out.c0 = pt.sahCost();
  pt.updateMaterials({ mat, uv, atlas, atlasRes: 2, atlasLayers: 3 });
  out.c1 = pt.sahCost();
  pt.updateMaterials({ mat });
  pt.updateMaterials({ mat, uv: null, atlas: null });
  out.c2 = pt.sahCost();
  pt.updateEnvironment({ env, envW: 3, envH: 2, bins });
  out.c3 = pt.sahCost();
  pt.updateEnvironment({ env: null, bins: new Uint32Array(4) });
  out.c4 = pt.sahCost();
  out.short_mat = thrown(() => pt.updateMaterials({ mat: new Float32Array(12) }));
  out.f64_mat = thrown(() => pt.updateMaterials({ mat: new Float64Array(24) }));
  out.short_uv = thrown(() => pt.updateMaterials({ mat, uv: new Float32Array(6) }));
  out.short_atlas = thrown(() => pt.updateMaterials({ mat, atlas: new Uint8Array(8), atlasRes: 2, atlasLayers: 3 }));
  out.atlas_no_shape = thrown(() => pt.updateMaterials({ mat, atlas }));
  out.no_object = thrown(() => pt.updateMaterials());
  out.no_bins = thrown(() => pt.updateEnvironment({ env, envW: 3, envH: 2 }));
  out.odd_bins = thrown(() => pt.updateEnvironment({ env: null, bins: new Uint32Array(6) }));
  out.short_env = thrown(() => pt.updateEnvironment({ env: new Uint8Array(8), envW: 3, envH: 2, bins }));
  out.env_zero = thrown(() => pt.updateEnvironment({ env, envW: 0, envH: 2, bins }));
  out.cost_after_refused = pt.sahCost();
  const scene = pt._scene, target = pt._target;
  out.addon_len = thrown(() => addon.sceneUpdateMaterials(scene, 3, mat, null, null, 0, 0));
  out.addon_atlas = thrown(() => addon.sceneUpdateMaterials(scene, 2, mat, null, atlas, 2, 2));
  out.addon_type = thrown(() => addon.sceneUpdateMaterials(scene, 2, [0, 1], null, null, 0, 0));
  out.addon_no_bins = thrown(() => addon.sceneUpdateEnvironment(scene, null, 0, 0, null));
  out.addon_env_len = thrown(() => addon.sceneUpdateEnvironment(scene, env, 4, 2, bins));
  out.target_as_scene = [thrown(() => addon.sceneUpdateMaterials(target, 2, mat, null, null, 0, 0)), thrown(() => addon.sceneUpdateEnvironment(target, null, 0, 0, bins))];
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.updateMaterials({ mat })), thrown(() => pt.updateEnvironment({ env: null, bins }))];
  await job;
  out.after = [thrown(() => pt.updateMaterials({ mat })), thrown(() => pt.updateEnvironment({ env: null, bins }))];
  await pt.close();
  out.closed = [thrown(() => addon.sceneUpdateMaterials(scene, 2, mat, null, null, 0, 0)), thrown(() => addon.sceneUpdateEnvironment(scene, null, 0, 0, bins))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
