'use strict';
// Driven by tests/test_exposure_cpu.py: node exposure_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's auto-exposure calls on the mock library: the mode and the seven parameters reach the library (omitted ones
// as the defaults), bad parameters are refused (unknown names and non-numbers before the library, ranges by it), exposure()
// and exposureReset() need the mode, the target handle is guarded while a renderAsync runs, wrong and destroyed handles are
// refused.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(18), mat: new Float32Array(24), norm: new Float32Array(54), uv: new Float32Array(12),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
(async () => {
  const out = {};
  const pt = new F.PathTracer(desc, 3, 2, 0);
  out.off_get = thrown(() => pt.exposure());
  out.off_reset = thrown(() => pt.exposureReset());
  pt.setAutoExposure();
  out.defaults = pt.exposure();
  pt.setAutoExposure(true, { key: 0.5, adaptDown: 0.25 });
  out.some = pt.exposure();
  pt.exposureReset();
  out.reset = pt.exposure();
  out.unknown = thrown(() => pt.setAutoExposure(true, { keyValue: 0.5 }));
  out.not_a_number = thrown(() => pt.setAutoExposure(true, { key: '0.5' }));
  out.bad = [thrown(() => pt.setAutoExposure(true, { key: 0 })), thrown(() => pt.setAutoExposure(true, { key: NaN })),
    thrown(() => pt.setAutoExposure(true, { low: 0.9, high: 0.1 })), thrown(() => pt.setAutoExposure(true, { high: 1.5 })),
    thrown(() => pt.setAutoExposure(true, { adaptUp: 0 })), thrown(() => pt.setAutoExposure(true, { adaptDown: 1.5 })),
    thrown(() => pt.setAutoExposure(true, { minLog2: 2, maxLog2: 1 })), thrown(() => pt.setAutoExposure(true, { maxLog2: Infinity }))];
  const scene = pt._scene, target = pt._target;
  out.scene_as_target = thrown(() => addon.exposure(scene));
  out.too_few = thrown(() => addon.setAutoExposure(target, true, 0.18));
  const job = pt.renderAsync(1);
  out.during = [thrown(() => pt.setAutoExposure(true)), thrown(() => pt.exposure()), thrown(() => pt.exposureReset())];
  await job;
  out.after = thrown(() => pt.setAutoExposure(true));
  pt.setAutoExposure(false);
  out.off_again = thrown(() => pt.exposure());
  await pt.close();
  out.closed = thrown(() => addon.exposureReset(target));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
