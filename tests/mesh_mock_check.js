'use strict';
// Driven by tests/test_mesh_node.py: node mesh_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's setMesh() / updateVertices() / readMesh() on the mock library: argument checks in fspt.js and in the addon, the
// calls through the addon, the renderAsync guard on the scene handle, wrong and destroyed handles.
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
  const vertex = new Uint32Array([0, 1, 2, 2, 1, 3]), uv = new Float64Array(12);
  const smooth = new Uint8Array(2), rank = new Uint32Array([1, 0]);
  const pos = new Float32Array(12);
  out.no_mesh = thrown(() => pt.updateVertices(pos));
  out.no_read = thrown(() => pt.readMesh());
  pt.setMesh({ vertex, uv });
  out.cost_mesh = pt.sahCost();
  out.read_before_update = thrown(() => pt.readMesh());
  pt.updateVertices(pos);
  pt.updateVertices(pos);
  out.cost_updates = pt.sahCost();
  const r = pt.readMesh();
  out.read = [r.tri instanceof Float32Array, r.tri.length, r.tri[0], r.norm instanceof Float32Array, r.norm.length, r.norm[0]];
  out.wrong_count = thrown(() => pt.updateVertices(new Float32Array(9)));
  pt.setMesh({ vertex, uv, smooth, rank, tri, norm, nVertices: 300 });
  out.cost_full = pt.sahCost();
  pt.updateVertices(new Float32Array(900));
  out.cost_full_update = pt.sahCost();
  const stat = new Uint32Array([0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]);
  pt.setMesh({ vertex: stat, uv, tri, norm });
  out.cost_static = pt.sahCost();
  pt.setMesh(null);
  out.cost_dropped = pt.sahCost();
  out.short_vertex = thrown(() => pt.setMesh({ vertex: new Uint32Array(3), uv }));
  out.u16_vertex = thrown(() => pt.setMesh({ vertex: new Uint16Array(6), uv }));
  out.f32_uv = thrown(() => pt.setMesh({ vertex, uv: new Float32Array(12) }));
  out.no_uv = thrown(() => pt.setMesh({ vertex }));
  out.short_smooth = thrown(() => pt.setMesh({ vertex, uv, smooth: new Uint8Array(1) }));
  out.short_rank = thrown(() => pt.setMesh({ vertex, uv, rank: new Uint32Array(3) }));
  out.short_tri = thrown(() => pt.setMesh({ vertex, uv, tri: new Float32Array(9), norm }));
  out.short_norm = thrown(() => pt.setMesh({ vertex, uv, tri, norm: new Float32Array(27) }));
  out.static_no_rest = thrown(() => pt.setMesh({ vertex: stat, uv }));
  out.static_no_norm = thrown(() => pt.setMesh({ vertex: stat, uv, tri }));
  out.few_vertices = thrown(() => pt.setMesh({ vertex, uv, nVertices: 3 }));
  out.many_vertices = thrown(() => pt.setMesh({ vertex, uv, nVertices: 0xFFFFFFFF }));
  out.pos_len = thrown(() => pt.updateVertices(new Float32Array(10)));
  out.pos_type = thrown(() => pt.updateVertices(new Float64Array(12)));
  out.cost_after_refused = pt.sahCost();
  const scene = pt._scene, target = pt._target;
  out.addon_len = thrown(() => addon.sceneSetMesh(scene, 3, vertex, 4, uv, null, null, null, null));
  out.addon_uv = thrown(() => addon.sceneSetMesh(scene, 2, vertex, 4, new Float64Array(6), null, null, null, null));
  out.addon_pos = thrown(() => addon.sceneUpdateVertices(scene, new Float32Array(7)));
  out.target_as_scene = [thrown(() => addon.sceneSetMesh(target, 2, vertex, 4, uv, null, null, null, null)), thrown(() => addon.sceneUpdateVertices(target, pos)),
    thrown(() => addon.sceneReadMesh(target, 2))];
  pt.setMesh({ vertex, uv });
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.setMesh({ vertex, uv })), thrown(() => pt.updateVertices(pos)), thrown(() => pt.readMesh())];
  await job;
  out.after = [thrown(() => pt.setMesh({ vertex, uv })), thrown(() => pt.updateVertices(pos)), thrown(() => pt.readMesh())];
  await pt.close();
  out.closed = [thrown(() => addon.sceneSetMesh(scene, 2, vertex, 4, uv, null, null, null, null)), thrown(() => addon.sceneUpdateVertices(scene, pos)),
    thrown(() => addon.sceneReadMesh(scene, 2))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
