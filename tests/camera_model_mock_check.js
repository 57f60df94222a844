'use strict';
// Driven by tests/test_camera_model_cpu.py: node camera_model_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's setCameraModel() / cameraModel on the mock library: argument checks in fspt.js and again in the addon, the
// calls through the addon, the renderAsync guard, a destroyed handle.  The mock's getter reports ipd + 1000 x the calls
// that reached the library.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0), odd = new F.PathTracer(desc, 3, 3, 0);
  const calls = () => Math.round(pt.cameraModel.ipd / 1000);
  out.initial = pt.cameraModel.model;
  pt.setCameraModel({ model: 'fisheye', angle: 2.5 });
  out.fisheye = [pt.cameraModel.model, pt.cameraModel.angle, calls()];
  pt.setCameraModel({ model: 'stereo', ipd: 0.25 });
  out.stereo = [pt.cameraModel.model, Math.round((pt.cameraModel.ipd % 1000) * 1000) / 1000, calls()];
  pt.setCameraModel({ model: 'equirect' });
  pt.setCameraModel();
  out.back = [pt.cameraModel.model, calls()];
  out.unknown = thrown(() => pt.setCameraModel({ model: 'cube' }));
  out.not_object = thrown(() => pt.setCameraModel('equirect'));
  out.angle_zero = thrown(() => pt.setCameraModel({ model: 'fisheye', angle: 0 }));
  out.angle_big = thrown(() => pt.setCameraModel({ model: 'fisheye', angle: 6.3 }));
  out.angle_nan = thrown(() => pt.setCameraModel({ model: 'fisheye', angle: NaN }));
  out.angle_string = thrown(() => pt.setCameraModel({ model: 'fisheye', angle: '2' }));
  out.angle_stray = thrown(() => pt.setCameraModel({ model: 'ortho', angle: 1 }));
  out.ipd_neg = thrown(() => pt.setCameraModel({ model: 'stereo', ipd: -0.1 }));
  out.ipd_inf = thrown(() => pt.setCameraModel({ model: 'stereo', ipd: Infinity }));
  out.ipd_stray = thrown(() => pt.setCameraModel({ model: 'equirect', ipd: 0.1 }));
  out.calls_after_refused = calls();
  const target = pt._target;
  out.addon_model = thrown(() => addon.setCameraModel(target, 7, 1, 0.064));
  out.addon_angle = thrown(() => addon.setCameraModel(target, 2, 0, 0.064));
  out.addon_ipd = thrown(() => addon.setCameraModel(target, 4, 1, -1));
  out.scene_as_target = thrown(() => addon.setCameraModel(pt._scene, 3, 1, 0.064));
  out.calls_after_addon = calls();
  out.odd_height = thrown(() => odd.setCameraModel({ model: 'stereo' }));
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.setCameraModel({ model: 'ortho' })), thrown(() => pt.cameraModel)];
  await job;
  out.after = thrown(() => pt.setCameraModel({ model: 'ortho' }));
  await pt.close(); await odd.close();
  out.closed = thrown(() => addon.setCameraModel(target, 3, 1, 0.064));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
