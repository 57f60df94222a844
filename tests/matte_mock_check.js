'use strict';
// Driven by tests/test_matte_cpu.py: node matte_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's ID-matte entries on the mock library (tests/matte_mock_stub.c): hashes and manifests, the argument checks,
// the calls through the addon, drawExr's and exrEncode's matte forms, and the renderAsync guard.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const names = ['', 'hello', 'CryptoObject', 'CryptoMaterial', '0:a.obj', '1:b "q".obj', 'été'];
out.hashes = names.map((n) => F.matteHash(n));
out.manifest = F.matteManifest(names.slice(4));
const pt = new F.PathTracer(desc, 3, 2, 0);
out.noIds = thrown(() => pt.mattes(2, 5));
out.badKind = thrown(() => pt.setMatte('asset', [0], ['a']));
out.badCount = thrown(() => pt.setMatte('object', [0, 0], ['a']));
out.badLabel = thrown(() => pt.setMatte('object', [1], ['a']));
pt.setMatte('object', [1], ['a', 'b']);
pt.setMatte('material', new Int32Array([-1]), ['m0000']);
pt.mattes(4, 9);
const o = pt.readMattes('object'), m = pt.readMattes('material');
out.object = { id: o.ids[0], cov: o.coverage[0], samples: o.coverage[1] * 0 + pt.readMattes('object', true)[2], seed: pt.readMattes('object', true)[3],
  manifestLen: pt.readMattes('object', true)[4], lengths: [o.ids.length, o.coverage.length] };
out.material = { id: m.ids[0], manifestLen: pt.readMattes('material', true)[4] };
out.lost = [pt.mattesLost('object'), pt.mattesLost('material')];
out.badReadKind = thrown(() => pt.readMattes('uv'));
out.wrongHandle = [thrown(() => F.addon.readMattes(pt._scene, 0, new Float32Array(72))), thrown(() => F.addon.sceneSetMatte(pt._target, 1, 0, null, null))];
out.draw = Array.from(pt.drawExr({ layers: 'alpha,crypto_object,crypto_material', compression: 'zips' }));
out.drawBufferBytes = pt._exrBuf.length;
out.badLayer = thrown(() => pt.drawExr({ layers: 'crypto_asset' }));
const rgba = new Float32Array(5 * 2 * 4), ranks = new Float32Array(5 * 2 * 12);
out.encode = Array.from(F.exrEncode(rgba, null, 5, 2, { bottomUp: true, layers: ['crypto_object', 'crypto_material'],
  mattes: { object: { ranks, manifest: '{"a":"1"}' }, material: ranks } }));
out.encodeShortRanks = thrown(() => F.exrEncode(rgba, null, 5, 2, { layers: ['crypto_object'], mattes: { object: new Float32Array(7) } }));
pt.setMatte('material', null);
out.droppedManifest = pt._manifests[1];
const p = pt.renderAsync(1);
out.during = [thrown(() => pt.mattes(1, 1)), thrown(() => pt.readMattes('object')), thrown(() => pt.mattesLost('object')), thrown(() => pt.setMatte('object', [0], ['a']))];
p.then(() => {
  out.after = thrown(() => pt.mattes(1, 1));
  return Promise.resolve(pt.close());
}).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)))
  .catch((err) => { console.error(err); process.exit(1); });
