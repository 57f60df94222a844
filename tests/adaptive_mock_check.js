'use strict';
// Driven by tests/test_adaptive_cpu.py: node adaptive_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's renderAdaptive() / readSampleCounts() on the mock library: argument checks, the calls through the addon,
// the host state afterwards, the renderAsync guard and a closed handle.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
out.target = thrown(() => pt.renderAdaptive({ targetRelMse: -1 }));
out.nan = thrown(() => pt.renderAdaptive({ targetRelMse: NaN }));
out.missing = thrown(() => pt.renderAdaptive({}));
out.ticks = thrown(() => pt.renderAdaptive({ targetRelMse: 0.01, maxTicks: 1.5 }));
out.invalid = thrown(() => pt.renderAdaptive({ targetRelMse: 0.01, roundTicks: 1 }));
pt.renderAdaptive({ targetRelMse: 0.0025 });
const ref = new F.PathTracer(desc, 3, 2, 0);
ref.seed(7); pt.seed(7);
out.n = pt.renderAdaptive({ targetRelMse: 0, maxTicks: 256 });
ref.render(256);
out.pingpong = pt.pingpong;
out.advanced = pt._rng[0] === ref._rng[0];
out.counts = Array.from(pt.readSampleCounts());
out.counts_len = thrown(() => pt.readSampleCounts(new Uint32Array(5)));
const target = pt._target, scene = pt._scene;
out.wrong_kind = thrown(() => addon.renderAdaptive(scene, {}, 0, 64, 64, 32, 1n));
const p = pt.renderAsync(1);
out.during = thrown(() => pt.renderAdaptive({ targetRelMse: 0.01 }));
p.then(() => Promise.resolve(ref.close())).then(() => Promise.resolve(pt.close())).then(() => {
  out.destroyed = thrown(() => addon.readSampleCounts(target, new Uint32Array(6)));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}).catch((e) => { console.error(e); process.exit(1); });
