'use strict';
// Driven by tests/test_pose_node.py: node pose_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's setPose() / updateTransforms() on the mock library: argument checks, the calls through the addon, the
// renderAsync guard on the scene handle, wrong and destroyed handles.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const tri = new Float32Array(18), norm = new Float32Array(54), part = new Uint32Array([0, 2]);
  const xf = new Float32Array(36);
  out.no_pose = thrown(() => pt.updateTransforms(xf));
  pt.setPose(part, tri, norm);
  out.cost_pose = pt.sahCost();
  pt.updateTransforms(xf);
  pt.updateTransforms(xf);
  out.cost_updates = pt.sahCost();
  out.wrong_parts = thrown(() => pt.updateTransforms(new Float32Array(24)));
  pt.setPose(part, tri, null, 5);
  out.cost_five = pt.sahCost();
  pt.setPose(null);
  out.cost_dropped = pt.sahCost();
  out.short_part = thrown(() => pt.setPose(new Uint32Array(1), tri, norm));
  out.i32_part = thrown(() => pt.setPose(new Int32Array(2), tri, norm));
  out.short_tri = thrown(() => pt.setPose(part, new Float32Array(9), norm));
  out.no_tri = thrown(() => pt.setPose(part));
  out.short_norm = thrown(() => pt.setPose(part, tri, new Float32Array(27)));
  out.few_parts = thrown(() => pt.setPose(part, tri, norm, 2));
  out.xf_len = thrown(() => pt.updateTransforms(new Float32Array(13)));
  out.xf_type = thrown(() => pt.updateTransforms(new Float64Array(12)));
  out.cost_after_refused = pt.sahCost();
  const scene = pt._scene, target = pt._target;
  out.addon_len = thrown(() => addon.sceneSetPose(scene, 3, part, 3, tri, null));
  out.addon_xf = thrown(() => addon.sceneUpdateTransforms(scene, new Float32Array(7)));
  out.target_as_scene = [thrown(() => addon.sceneSetPose(target, 2, part, 3, tri, null)), thrown(() => addon.sceneUpdateTransforms(target, xf))];
  pt.setPose(part, tri, norm);
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.setPose(part, tri, norm)), thrown(() => pt.updateTransforms(xf))];
  await job;
  out.after = [thrown(() => pt.setPose(part, tri, norm)), thrown(() => pt.updateTransforms(xf))];
  await pt.close();
  out.closed = [thrown(() => addon.sceneSetPose(scene, 2, part, 3, tri, null)), thrown(() => addon.sceneUpdateTransforms(scene, xf))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
