# build + run tools/convbench (isolated 64->64 conv kernels with phase counters)
set -e
cd /root/repo/tools
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -DDEX_TIMING -I../include -I../dex_tts_amd/csrc -o convbench convbench.hip ../dex_tts_amd/csrc/conv3x3_stream.hip ../dex_tts_amd/csrc/conv3x3_regw.hip 2>/dev/null
# `convbench b1` timing without the phase counters (they add instructions to every workgroup)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../include -I../dex_tts_amd/csrc -o convbench_nt convbench.hip ../dex_tts_amd/csrc/conv3x3_stream.hip ../dex_tts_amd/csrc/conv3x3_regw.hip 2>/dev/null
