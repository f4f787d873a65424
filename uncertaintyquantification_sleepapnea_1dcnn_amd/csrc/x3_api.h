// Host interface of the fp32-faithful layer-wise inference kernels (x3_layers.hip), included by that file and
// by x3_bindings.cpp.  The argument structs are in x3_args.h, the layer kernel's geometry in x3_geo.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "x3_args.h"
#include "x3_geo.h"

namespace apneauq {
// the row of the layer table this library was built with (x3_geo.h; S == 0: no such layer)
x3::LayerInfo x3_layer_info(int layer);
hipError_t x3_launch_layer(int layer, const x3::LayerArgs& A, int grid, bool dense_rows, hipStream_t stream);
hipError_t x3_launch_l1(const x3::L1Args& A, hipStream_t stream);
hipError_t x3_launch_aff(const x3::AffArgs& A, hipStream_t stream);
hipError_t x3_launch_head(const x3::HeadArgs& A, hipStream_t stream);
}  // namespace apneauq
