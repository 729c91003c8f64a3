#!/usr/bin/env bash
# Sanitizer run of the host-submit code (HOST code only, CPU only): host_submit_check.cpp, the product sources and the
# emulator in one program built with AddressSanitizer and UndefinedBehaviorSanitizer, then run.  Not part of the pytest
# suite (the build takes minutes); run it by hand after a change to the submits of fastp_amd/csrc/fastp_gpu.hip.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
SRC=$HERE/../../fastp_amd/csrc
OUT=${1:-$HERE/host_submit_check}
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas \
    -Wno-unused-variable -I"$HERE" -I"$SRC" -I"$HERE/../../include" "$HERE/host_submit_check.cpp" \
    -x c++ "$SRC/fastp_gpu.hip" "$SRC/fq_host.cpp" "$SRC/fq_glue.cpp" "$SRC/fq_comm.cpp" "$SRC/fq_stream.cpp" "$HERE/sim.cpp" \
    -ldl -lpthread -lz -o "$OUT"
"$OUT"
