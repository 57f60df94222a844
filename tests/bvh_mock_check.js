'use strict';
// Driven by tests/test_bvh_build_cpu.py: node bvh_mock_check.js <dir with fspt.js + fspt_napi.node (mock)> <out.json>
// buildScene's builder choice on the mock library: the option is checked, {bvh: 'gpu'} reaches fspt_builder_build_gpu with
// the leaf size and the device, the library's refusal surfaces as an exception, and the addon checks its handle.
const path = require('path'), fs = require('fs');
const F = require(path.join(process.argv[2], 'fspt.js'));
const addon = require(path.join(process.argv[2], 'fspt_napi.node'));
const thrown = (f) => { try { f(); return null; } catch (e) { return e.constructor.name + ': ' + e.message; } };
const out = {};
out.bad_option = thrown(() => F.buildScene([], {}, null, 4, { bvh: 'cpu' }));
// the mock builds nothing: the call reaches the library, then reading the arrays fails (the stubbed counts)
out.gpu = thrown(() => F.buildScene([], {}, null, 8, { bvh: 'gpu', device: 1 }));
out.gpu_default_device = thrown(() => F.buildScene([], {}, null, 2, { bvh: 'gpu' }));
out.refused = thrown(() => F.buildScene([], {}, null, 65, { bvh: 'gpu' }));
out.not_a_builder = thrown(() => addon.builderBuildGpu({}, 4, 0));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
