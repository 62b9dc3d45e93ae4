#!/bin/bash
# Build libseeme_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="${SEEME_BUILD_OUT:-$here/../libseeme_hip.so}"
srcs=("$here"/api.hip "$here"/vae_kernels.hip "$here"/den_kernels.hip "$here"/misc_kernels.hip "$here"/pointnet_bf16.hip "$here"/vae_h16.hip "$here"/glue_kernels.hip "$here"/vae_train.hip "$here"/hyp_metrics.hip "$here"/social_metrics.hip "$here"/resnet.hip "$here"/mesh_metrics.hip "$here"/collision.hip "$here"/smpl_kernels.hip "$here"/recording.hip "$here"/scene_views.hip "$here"/crop_patches.hip "$here"/render.hip "$here"/flow_head.hip "$here"/track.hip "$here"/headset.hip "$here"/scene_depth.hip)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
    -Wall -Wno-unused-function -o "$out" "${srcs[@]}" "$@"
echo "built $out"
