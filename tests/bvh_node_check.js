'use strict';
// Driven by tests/test_bvh_build_gpu.py: node bvh_node_check.js <job.json> <out.json>
// job = {props, objs, device}: buildScene(props, objs, null, 4, {bvh: 'gpu', device}) on the real addon; the arrays go
// back base64-encoded with the depth and the builder's name.
const path = require('path'), fs = require('fs');
const F = require(path.join(__dirname, '..', 'fspt_amd', 'js', 'fspt.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const s = F.buildScene(job.props, job.objs, null, 4, { bvh: 'gpu', device: job.device });
const b64 = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64');
fs.writeFileSync(process.argv[3], JSON.stringify({ bvh: b64(s.bvh), tri: b64(s.tri), mat: b64(s.mat), norm: b64(s.norm), uv: b64(s.uv),
  depth: s.depth, builder: s.bvhBuilder }));
