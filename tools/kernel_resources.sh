#!/bin/bash
# Per-kernel register / scratch / occupancy table of the three kernel files - fspt_kernels.hip (the renderers), fspt_passes.hip
# (the stand-alone passes: k_camera, k_intersect, k_features, k_temporal_gbuffer, k_adaptive_*, the test hooks) and
# fspt_post.hip (the image chain) - and of fspt_pose.hip (k_pose_transform; k_skin_transform),
# fspt_appearance.hip (the k_ap_* layouts), fspt_texpack.hip (k_tex_resample) and the encoders: fspt_jpeg.hip
# (DESIGN 8.19), fspt_png.hip, fspt_exr.hip and fspt_deflate.hip (k_deflate, the last two's)
# and fspt_lights_build.hip (the k_lt_* kernels of the GPU light-table builder)
# (hipcc -Rpass-analysis=kernel-resource-usage), demangled, in one table.
# usage: tools/kernel_resources.sh [extra -D flags]
cd "$(dirname "$0")/.." || exit 1
for f in fspt_kernels fspt_passes fspt_post fspt_pose fspt_appearance fspt_texpack fspt_jpeg fspt_png fspt_exr fspt_deflate fspt_lights_build; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -ffp-contract=off ${AB_SLP:--fno-slp-vectorize} -std=c++17 -Wno-unused-value -c --cuda-device-only \
    -Rpass-analysis=kernel-resource-usage "$@" fspt_amd/csrc/$f.hip -o /tmp/${f}_res.o 2>&1
done |
python3 -c '
import re, sys, subprocess
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m: cur = {"name": m.group(1)}; rows.append(cur); continue
    for key, pat in (("sgpr", r"SGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        m = re.search(pat, line)
        if m and cur is not None: cur[key] = int(m.group(1))
names = subprocess.run(["c++filt"] + [r["name"] for r in rows], capture_output=True, text=True).stdout.split("\n")
print("%-62s %5s %5s %7s %6s %4s %6s" % ("kernel", "VGPR", "SGPR", "scratch", "vspill", "occ", "LDS"))
for r, n in zip(rows, names):
    n = re.sub(r"^void fspt::", "", n.replace("(anonymous namespace)::", "")); n = re.sub(r"\(.*$", "", n)
    print("%-62s %5d %5d %7d %6d %4d %6d" % (n, r.get("vgpr", -1), r.get("sgpr", -1), r.get("scratch", -1), r.get("vspill", -1), r.get("occ", -1), r.get("lds", -1)))
'
