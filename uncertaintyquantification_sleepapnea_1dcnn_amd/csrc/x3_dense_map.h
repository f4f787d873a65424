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

// ---- per-tile row descriptors.  Everything the staging and the epilogue need to know about a row
// depends on (tile, row) only, not on the chunk or the channel tile, so it is computed once per tile.
// A row is named by rel = its dense row minus the tile's first (-pad .. rows + pad - 1; dl = off + rel).
// Its global row is the tile's first global row + rel (linear: no descriptor needed), and it lies inside
// the group iff rel < rows_left = 60 n_win - first_row(tile) (callers may clamp it to any value above
// rows + pad), which is the same as window < n_win.
// Packed word: LDS row (9 bits: lds_rows(256) = 392), time step (6 bits), window slot (3 bits), valid.
constexpr int kDescStepShift = 9, kDescSlotShift = 15, kDescValidShift = 18;
__host__ __device__ constexpr unsigned desc_pack(int lrow, int step, int slot, bool valid) {
  return (unsigned)lrow | (unsigned)step << kDescStepShift | (unsigned)slot << kDescSlotShift |
         (valid ? 1u : 0u) << kDescValidShift;
}
__host__ __device__ constexpr int desc_lds_row(unsigned d) { return (int)(d & 511u); }
__host__ __device__ constexpr int desc_step(unsigned d) { return (int)(d >> kDescStepShift & 63u); }
__host__ __device__ constexpr int desc_slot(unsigned d) { return (int)(d >> kDescSlotShift & 7u); }
__host__ __device__ constexpr bool desc_valid(unsigned d) { return (d >> kDescValidShift & 1u) != 0u; }
// descriptor of row rel of a tile that starts `off` steps into its first window; valid: the row is staged
// (staged(), edge rows) and inside the group.  A row that is not staged has descriptor 0.
__host__ __device__ constexpr unsigned row_desc(int rel, int off, int rows, int pad, int rows_left) {
  const int dl = off + rel;
  if (!staged(dl, off, rows, pad)) return 0u;
  return desc_pack(lds_row(dl), step_of(dl), slot_of(dl), rel < rows_left);
}
// whole-window slot tiles (row ri = 60 s + t of the tile's S windows): LDS row kHalo + 64 s + t
__host__ __device__ constexpr unsigned slot_row_desc(int ri, int rows_left) {
  return desc_pack(lds_row(ri), step_of(ri), slot_of(ri), ri < rows_left);
}
// The mask word of a row: dropout_bits2(key, t, c) = mix32(key ^ (t << 9 | c >> 1)) = mix32(mask_word ^ (c >> 1))
// for c < 1024, so a row keeps key ^ (t << 9) and a channel pair costs one xor and one mix32.
__host__ __device__ constexpr unsigned mask_word(unsigned sample_key, int step) { return sample_key ^ ((unsigned)step << 9); }

}  // namespace dense
}  // namespace x3
}  // namespace apneauq

#ifdef APNEAUQ_X3_DENSE_MAP_PLAIN
#undef __host__
#undef __device__
#undef APNEAUQ_X3_DENSE_MAP_PLAIN
#endif
