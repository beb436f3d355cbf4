#!/bin/bash
# ASan + UBSan over the host-only sources of libtracs_hip.so (CPU build).  usage: bash scripts/sanitize_host.sh
set -e
cd "$(dirname "$0")/.."
OUT=${TMPDIR:-/tmp}/tracs_san
mkdir -p $OUT
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
    scripts/san_driver.cpp tracs_amd/csrc/fasta.cpp tracs_amd/csrc/alignio.cpp -lz -lpthread -o $OUT/san_driver
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $OUT/san_driver $OUT
# second pass: ThreadSanitizer over the same driver (parallel readers, writers)
g++ -std=c++17 -O1 -g -fsanitize=thread -Iinclude \
    scripts/san_driver.cpp tracs_amd/csrc/fasta.cpp tracs_amd/csrc/alignio.cpp -lz -lpthread -o $OUT/tsan_driver
TSAN_OPTIONS=halt_on_error=1 $OUT/tsan_driver $OUT
# third pass: the owners and the allocation path (csrc/common.h, csrc/alloc_path.h) against stub HIP calls
${HIPCC:-/opt/rocm/bin/hipcc} -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
    scripts/san_alloc.cpp -o $OUT/san_alloc
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $OUT/san_alloc
# fourth pass: the run-time switches' accessors (csrc/switches.h): host only, nothing from HIP
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer scripts/san_switches.cpp -lpthread -o $OUT/san_switches
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $OUT/san_switches
