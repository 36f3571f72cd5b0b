#!/bin/bash
# Host code of the replays under AddressSanitizer + UBSan, as stand-alone programs on the CPU (no GPU is opened, nothing is
# loaded into python): replay_plan, the route gates, the batch's route plan, the site windows and the resident planes' lists of ramx_device.hip, pad_to_tiles, the sinks' one-family view and the subfamily sink's host steps of ramx_extend.c, all static, so each program includes
# its source file and takes the rest of the library from the built libramx.so; and ramx_linkage.c, which stands alone.
# usage: tools/host_asan/run.sh        (after the library has been built)
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
rocm=${ROCM:-/opt/rocm}
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
inc="-I$root/include -I$root/repeatafterme_amd/csrc"
lib="-L$root/repeatafterme_amd -lramx -Wl,-rpath,$root/repeatafterme_amd -Wl,-rpath,$rocm/lib"
san="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g"
gcc -std=gnu11 -O1 -Wno-alloc-size-larger-than $san $inc -o "$out/pad_to_tiles" "$here/pad_to_tiles_main.c" $lib -lm -lpthread
"$out/pad_to_tiles"
# the pure host steps of the subfamily sink of ramx_extend.c on hand-made tables: gather and scatter of a per-K call, the distances, the kept groups
gcc -std=gnu11 -O1 -Wno-alloc-size-larger-than $san $inc -o "$out/subfam_sink" "$here/subfam_sink_main.c" $lib -lm -lpthread
"$out/subfam_sink"
# the selection, the pair statistic and the components of the linkage (ramx_linkage.c is compiled into the program, under the sanitizers too)
gcc -std=gnu11 -O1 $san $inc -o "$out/linkage" "$here/linkage_main.c" -lm
"$out/linkage"
# the selection of copies, the Kimura distance of a pair and the summary of a pair matrix (ramx_dist.c is compiled into the program, under the sanitizers too)
gcc -std=gnu11 -O1 $san $inc -o "$out/dist" "$here/dist_main.c" -lm
"$out/dist"
# the pair record, the candidates and the groups of the cross-family overlap against a brute force (ramx_xfam.c and ramx_term.c are compiled into the program, under the sanitizers too)
gcc -std=gnu11 -O1 $san $inc -o "$out/xfam" "$here/xfam_main.c"
"$out/xfam"
# the CpG-aware re-call on random records (ramx_recall.c is compiled into the program, under the sanitizers too)
gcc -std=gnu11 -O1 $san $inc -o "$out/recall_cpg" "$here/recall_cpg_main.c" "$root/repeatafterme_amd/csrc/ramx_recall.c"
"$out/recall_cpg"
# the command line's analysis outputs: hand-made records through the sinks, the writers and the post-passes of two families
# (ramx_cli_outputs.c is compiled into the program, under the sanitizers too)
gcc -std=gnu11 -O1 $san $inc -o "$out/cli_outputs" "$here/cli_outputs_main.c" $lib -lm
"$out/cli_outputs"
# (the device side of ramx_device.hip is compiled too, which takes a minute or two: the host object refers to its code object)
"$rocm/bin/hipcc" --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -fno-omit-frame-pointer $inc -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=undefined -o "$out/replay_plan" "$here/replay_plan_main.cpp" $lib -L"$rocm/lib" -lrccl -lpthread
"$out/replay_plan"
# the route of a direction at the edges of its gates (route_gates / route_settle of ramx_device.hip)
"$rocm/bin/hipcc" --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -fno-omit-frame-pointer $inc -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=undefined -o "$out/route" "$here/route_main.cpp" $lib -L"$rocm/lib" -lrccl -lpthread
"$out/route"
# the route plan of a batch at the edges of its classes, shapes and rounds (family_plan of ramx_device.hip)
"$rocm/bin/hipcc" --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -fno-omit-frame-pointer $inc -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=undefined -o "$out/family_plan" "$here/family_plan_main.cpp" $lib -L"$rocm/lib" -lrccl -lpthread
"$out/family_plan"
# the windows of the site-window analyses against their definition by enumeration, the sites' checks and the tile budget at their
# edges (window_flank / check_sites / tile_group of ramx_device.hip)
"$rocm/bin/hipcc" --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -fno-omit-frame-pointer $inc -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=undefined -o "$out/site_windows" "$here/site_windows_main.cpp" $lib -L"$rocm/lib" -lrccl -lpthread
"$out/site_windows"
# a family's plane list at the edges of its contract and the block lists of the calls that answer from the resident planes
# (plane_list / upper_blocks of ramx_device.hip)
"$rocm/bin/hipcc" --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -fno-omit-frame-pointer $inc -Xarch_host -fsanitize=address,undefined \
  -Xarch_host -fno-sanitize-recover=undefined -o "$out/resident" "$here/resident_main.cpp" $lib -L"$rocm/lib" -lrccl -lpthread
"$out/resident"
