// XCD-aware workgroup order, shared by every kernel that uses it (included by common.h) and by a host
// test (tests/tiled_geo_check.cpp): a plain constexpr integer function, no HIP types.
#pragma once

#ifndef __host__
#define APNEAUQ_XCD_ORDER_PLAIN 1
#define __host__
#define __device__
#define __forceinline__ inline
#endif

namespace apneauq {

// Hardware dispatch round-robins the workgroup ids of a grid over the XCDs (id % nx picks the XCD), so
// workgroups with neighbouring ids, which usually share weights or input rows, would land on nx
// different L2s.  xcd_order maps hardware id `bid` of a grid of `nwg` workgroups to a logical id such
// that the workgroups of one XCD take one contiguous range of logical ids: XCD x owns q + 1 ids if
// x < rem and q otherwise (q = nwg / nx, rem = nwg % nx), and bid is the (bid / nx)-th workgroup of
// XCD bid % nx.  A bijection of [0, nwg) for any grid size (checked for nwg <= 300 and nx = 1, 2, 4, 8
// by tests/test_tiled_geo_cpu.py).  nx: the XCDs the grid spans (8 on MI355X; a member-batched training
// grid spans the XCDs of one member: train_wgrad.hip, which keeps this expression written out).
__host__ __device__ __forceinline__ constexpr int xcd_order(int bid, int nwg, int nx = 8) {
  const int q = nwg / nx, rem = nwg % nx, xcd = bid % nx;
  return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + bid / nx;
}

}  // namespace apneauq

#ifdef APNEAUQ_XCD_ORDER_PLAIN
#undef __host__
#undef __device__
#undef __forceinline__
#undef APNEAUQ_XCD_ORDER_PLAIN
#endif
