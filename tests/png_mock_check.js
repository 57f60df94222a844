'use strict';
// Driven by tests/test_png_cpu.py: node png_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's drawPng / pngEncode / pngFilteredEval on the mock library: the argument checks, the calls through the addon,
// the growth of the reusable buffer, and the renderAsync guard.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
const d = pt.drawPng({ source: 'temporalDenoised', channels: 4, filter: 'paeth', chunkBytes: 512 });
out.draw = Array.from(d); out.drawIsBuffer = Buffer.isBuffer(d);
out.drawDefault = Array.from(pt.drawPng());
out.bufferBytes = pt._pngBuf.length;
out.badSource = thrown(() => pt.drawPng({ source: 'radiance' }));
out.badChannels = thrown(() => pt.drawPng({ channels: 1 }));
out.badFilter = thrown(() => pt.drawPng({ filter: 'best' }));
out.badChunk = thrown(() => pt.drawPng({ chunkBytes: 255 }));
pt._pngBuf = new Uint8Array(4);             // too small for the mock's 8 bytes: grown to the bound, the draw repeated
out.grownDraw = Array.from(pt.drawPng({ source: 'denoised' })); out.grownBytes = pt._pngBuf.length;
const e = F.pngEncode(new Uint8Array(5 * 2 * 4), 5, 2, { bottomUp: true, filter: 'up', chunkBytes: 1024 });
out.encode = Array.from(e); out.encodeIsBuffer = Buffer.isBuffer(e);
out.encodeShort = thrown(() => F.pngEncode(new Uint8Array(5 * 2 * 4 - 1), 5, 2));
out.encodeBadFilter = thrown(() => F.pngEncode(new Uint8Array(8), 1, 2, { filter: 'x' }));
out.filtered = Array.from(F.pngFilteredEval(new Uint8Array(2 * 3 * 4), 2, 3, { channels: 4, filter: 'sub' }));
const p = pt.renderAsync(1);
out.duringDraw = thrown(() => pt.drawPng());
p.then(() => {
  out.after = thrown(() => pt.drawPng());
  return Promise.resolve(pt.close());
}).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)))
  .catch((err) => { console.error(err); process.exit(1); });
