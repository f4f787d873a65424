// Index map of the dense-row tiles of the x3 layer kernels (x3_layers.hip, DENSE = true), shared by
// the kernel, the host bindings and a host test (plain constexpr integer functions, no HIP types).
//
// A group's windows form one dense row space: dense row d is window d / 60, time step d % 60.  A tile
// is `rows` (128 or 256) consecutive dense rows, so it starts anywhere inside a window and its GEMM rows
// carry no halo rows.  In LDS every window the tile touches keeps a fixed 64-row slot relative to the
// first one (60 time steps + 4 rows that stay zero: the 'same' padding of the conv), so with
// dl = d - 60 w_first the LDS row is kHalo + 64 (dl / 60) + dl % 60 = kHalo + dl + 4 (dl / 60).
#pragma once

#ifndef __host__
#define APNEAUQ_X3_DENSE_MAP_PLAIN 1
#define __host__
#define __device__
#endif

namespace apneauq {
namespace x3 {
namespace dense {

constexpr int kLen = 60, kSlot = 64, kHaloRows = 4;

// tiles of one group of n_win windows
__host__ __device__ constexpr long long tiles(long long n_win, int rows) { return (kLen * n_win + rows - 1) / rows; }
// tile starts are multiples of `rows` (a multiple of 4), so a tile starts at most at step 56 of a window
__host__ __device__ constexpr int max_windows(int rows) { return (kLen - 4 + rows - 1) / kLen + 1; }
__host__ __device__ constexpr int lds_rows(int rows) { return kHaloRows + kSlot * max_windows(rows) + kHaloRows; }

// first dense row, first window and start offset inside it of tile tl of a group
__host__ __device__ constexpr long long first_row(long long tl, int rows) { return tl * rows; }
__host__ __device__ constexpr int first_window(long long tl, int rows) { return (int)(first_row(tl, rows) / kLen); }
__host__ __device__ constexpr int offset(long long tl, int rows) { return (int)(first_row(tl, rows) % kLen); }
// windows the tile touches (the rows past the group's end included)
__host__ __device__ constexpr int windows(int off, int rows) { return (off + rows - 1) / kLen + 1; }

// local dense index dl = d - 60 w_first (tile rows: off .. off + rows - 1) -> window slot and LDS row
// (dl < 60 max_windows <= 360: dl / 60 as a 24-bit multiply and a shift, exact for 0 <= dl < 1024, instead of
// the quarter-rate 32-bit multiply-high of a general division)
__host__ __device__ constexpr int slot_of(int dl) { return (int)(((unsigned)dl & 1023u) * 1093u >> 16); }
__host__ __device__ constexpr int step_of(int dl) { return dl - kLen * slot_of(dl); }
__host__ __device__ constexpr int lds_row(int dl) { return kHaloRows + dl + (kSlot - kLen) * slot_of(dl); }

// Staged per chunk: dl = off - pad .. off + rows + pad - 1, the tile's rows and up to `pad` rows past
// either edge, the latter only where their window also owns a row of the tile (otherwise the halo is
// the slot's zero rows).
__host__ __device__ constexpr int staged_units(int rows, int pad) { return rows + 2 * pad; }
__host__ __device__ constexpr bool staged(int dl, int off, int rows, int pad) {
  return dl >= 0 && dl >= off - pad && dl < off + rows + pad && dl < kLen * windows(off, rows);
}

}  // namespace dense
}  // namespace x3
}  // namespace apneauq

#ifdef APNEAUQ_X3_DENSE_MAP_PLAIN
#undef __host__
#undef __device__
#undef APNEAUQ_X3_DENSE_MAP_PLAIN
#endif
