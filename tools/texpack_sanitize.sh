#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host side of the GPU texture packer: the argument checks
# and the per-layer records of fspt_amd/csrc/fspt_texpack_check.hpp, compiled into a stand-alone program (tools/texpack_sanitize.cpp)
# and run on the CPU.  The kernel and the entries around it need a GPU, which offers no sanitizer.
#   usage: bash tools/texpack_sanitize.sh        (from anywhere; builds into /tmp/fspt_san)
set -e
cd "$(dirname "$0")/.."
D=/tmp/fspt_san; mkdir -p $D
g++ -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $D/texpack_sanitize tools/texpack_sanitize.cpp
$D/texpack_sanitize
