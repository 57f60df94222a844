'use strict';
// Driven by tests/test_jpeg_cpu.py: node jpeg_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// The JS host's drawJpeg / presentJpeg / jpegEncode on the mock library: the argument checks, the calls through the addon,
// the growth of the reusable buffer, and the renderAsync guard.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const desc = { bvh: new Float32Array(9), tri: new Float32Array(9), mat: new Float32Array(12), norm: new Float32Array(27), uv: new Float32Array(6),
  atlas: new Uint8Array(4), atlasRes: 1, atlasLayers: 1, env: null, envW: 0, envH: 0, bins: new Uint32Array(4), leafSize: 4 };
const out = {};
const pt = new F.PathTracer(desc, 3, 2, 0);
const d = pt.drawJpeg({ source: 'temporalDenoised', quality: 60, subsampling: '444', restartMcus: 3 });
out.draw = Array.from(d); out.drawIsBuffer = Buffer.isBuffer(d);
out.drawDefault = Array.from(pt.drawJpeg());
out.bufferBytes = pt._jpegBuf.length;
const p1 = pt.presentJpeg({ denoise: true, quality: 50 });
out.present = { jpeg: Array.from(p1.jpeg), ticks: p1.ticks, isBuffer: Buffer.isBuffer(p1.jpeg) };
const p0 = pt.presentJpeg({ scale: 0.25 });
out.presentNothing = { jpeg: p0.jpeg, ticks: p0.ticks };
out.badSource = thrown(() => pt.drawJpeg({ source: 'radiance' }));
out.badSub = thrown(() => pt.presentJpeg({ subsampling: '422' }));
out.badQuality = thrown(() => pt.drawJpeg({ quality: 0 }));
out.badRestart = thrown(() => pt.presentJpeg({ restartMcus: 65536 }));
pt._jpegBuf = new Uint8Array(4);            // too small for the mock's 8 bytes: grown to the bound, the draw repeated
out.grownDraw = Array.from(pt.drawJpeg({ source: 'denoised' })); out.grownBytes = pt._jpegBuf.length;
pt._jpegBuf = new Uint8Array(4);            // a present frame that does not fit is dropped, the buffer grown for the next
const pd = pt.presentJpeg();
out.droppedPresent = { jpeg: pd.jpeg, ticks: pd.ticks, bytes: pt._jpegBuf.length };
out.afterDrop = pt.presentJpeg().ticks;
const e = F.jpegEncode(new Uint8Array(5 * 2 * 4), 5, 2, { bottomUp: true, quality: 90 });
out.encode = Array.from(e); out.encodeIsBuffer = Buffer.isBuffer(e);
out.encodeShort = thrown(() => F.jpegEncode(new Uint8Array(5 * 2 * 4 - 1), 5, 2));
out.encodeBadSub = thrown(() => F.jpegEncode(new Uint8Array(8), 1, 2, { subsampling: 'x' }));
const p = pt.renderAsync(1);
out.duringDraw = thrown(() => pt.drawJpeg());
out.duringPresent = thrown(() => pt.presentJpeg());
p.then(() => {
  out.after = thrown(() => pt.presentJpeg());
  return Promise.resolve(pt.close());
}).then(() => fs.writeFileSync(process.argv[3], JSON.stringify(out)))
  .catch((err) => { console.error(err); process.exit(1); });
