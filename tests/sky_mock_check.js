'use strict';
// Driven by tests/test_sky_cpu.py: node sky_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's updateSky() / updateEnvironmentAuto() / skyGenerate() / envBinsGpu() on the mock library: argument checks, the
// calls through the addon, the renderAsync guard on the scene handle, wrong and destroyed handles.  sahCost() reads the mock's
// count of what arrived.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  const env = new Uint8Array(3 * 2 * 4), sun = [0.5, 0.6, 0.4];
  out.c0 = pt.sahCost();
  pt.updateSky({ sunDir: sun, width: 8, height: 4, turbidity: 3 });
  out.c1 = pt.sahCost();
  pt.updateSky({ sunDir: new Float32Array(sun) });
  out.c2 = pt.sahCost();
  pt.updateEnvironmentAuto({ env, envW: 3, envH: 2 });
  out.c3 = pt.sahCost();
  const sky = F.skyGenerate({ sunDir: sun, width: 5, height: 2, viewSamples: 4, lightSamples: 2 }, 1);
  out.sky = [sky.width, sky.height, sky.rgbe.length, Array.from(sky.rgbe.slice(0, 4)), Array.from(sky.rgbe.slice(36, 40))];
  out.bins = Array.from(F.envBinsGpu(sky.rgbe, 5, 2, 3));
  out.no_object = thrown(() => pt.updateSky());
  out.no_sun = thrown(() => pt.updateSky({ width: 8, height: 4 }));
  out.short_sun = thrown(() => pt.updateSky({ sunDir: [1, 0] }));
  out.unknown = thrown(() => pt.updateSky({ sunDir: sun, turbidty: 2 }));
  out.albedo = thrown(() => pt.updateSky({ sunDir: sun, groundAlbedo: [1, 2] }));
  out.samples = thrown(() => pt.updateSky({ sunDir: sun, viewSamples: 2.5 }));
  out.refused_by_library = [thrown(() => pt.updateSky({ sunDir: sun, turbidity: 65 })), thrown(() => pt.updateSky({ sunDir: [0, 0, 0] })),
    thrown(() => pt.updateSky({ sunDir: sun, width: 0 })), thrown(() => F.skyGenerate({ sunDir: sun, lightSamples: 33 }))];
  out.auto_short = thrown(() => pt.updateEnvironmentAuto({ env: new Uint8Array(8), envW: 3, envH: 2 }));
  out.auto_zero = thrown(() => pt.updateEnvironmentAuto({ env, envW: 0, envH: 2 }));
  out.auto_null = thrown(() => pt.updateEnvironmentAuto({ env: null, envW: 3, envH: 2 }));
  out.still_needs_bins = thrown(() => pt.updateEnvironment({ env, envW: 3, envH: 2 }));
  out.cost_after_refused = pt.sahCost();
  const scene = pt._scene, target = pt._target, k = Float32Array.of(0.5, 0.6, 0.4, 1, 20, 0.02, 1, 0.3, 0.3, 0.3);
  out.addon_len = thrown(() => addon.sceneUpdateSky(scene, new Float32Array(9), 16, 8, 8, 4));
  out.addon_type = thrown(() => addon.sceneUpdateSky(scene, [1, 2], 16, 8, 8, 4));
  out.addon_env_len = thrown(() => addon.sceneUpdateEnvironmentAuto(scene, env, 4, 2));
  out.addon_bins_len = thrown(() => addon.envBinsGpu(env, 4, 2, 0));
  out.target_as_scene = [thrown(() => addon.sceneUpdateSky(target, k, 16, 8, 8, 4)), thrown(() => addon.sceneUpdateEnvironmentAuto(target, env, 3, 2))];
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.updateSky({ sunDir: sun, width: 8, height: 4 })), thrown(() => pt.updateEnvironmentAuto({ env, envW: 3, envH: 2 }))];
  await job;
  out.after = [thrown(() => pt.updateSky({ sunDir: sun, width: 8, height: 4 })), thrown(() => pt.updateEnvironmentAuto({ env, envW: 3, envH: 2 }))];
  await pt.close();
  out.closed = [thrown(() => addon.sceneUpdateSky(scene, k, 16, 8, 8, 4)), thrown(() => addon.sceneUpdateEnvironmentAuto(scene, env, 3, 2))];
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
