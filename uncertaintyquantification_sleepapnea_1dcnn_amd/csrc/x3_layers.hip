// fp32-faithful layer-wise inference of the Alarcón 1D-CNN on gfx950 (MI355X): "fp16x3" MFMA.
//
// Replaces the reference's inference hot loops at fp32 precision (Keras runs fp32, no mixed-precision
// policy anywhere in the reference):
//   * MC Dropout  np.stack([model(x, training=True) for _ in range(T)])   (uq_techniques.py:22): BN on
//     per-pass batch statistics of the WHOLE window set, dropout on, moving averages updated;
//   * Deep Ensemble  np.stack([m.predict(x) for m in models])           (uq_techniques.py:29): BN on
//     moving statistics, no dropout;
//   * standard MC Dropout (BN on moving statistics, dropout on).
//
// Precision.  Every conv operand is split into two fp16 halves, v = hi + lo with hi = fp16(v) and
// lo = fp16(v - hi) (22 significant bits), and each product is formed by three v_mfma_f32_16x16x32_f16
// (hi*hi + hi*lo + lo*hi, fp32 accumulate): the dropped lo*lo term and the split residuals are ~2^-22
// relative, below fp32 GEMM rounding over K = 28..2304.  Weights are pre-scaled by an exact power of
// two per layer (host) so that both halves stay in the fp16 normal range; the epilogue undoes it.
// Block 1 (Cin = 4, 0.4 % of the FLOPs) runs in plain fp32 FMAs.  BN moments are fp32 per tile, fp64
// across tiles; the BN affine, dropout, GAP, Dense and sigmoid are fp32.
//
// Data flow (one launch per layer; the window set stays resident in HBM):
//   l1_kernel      R_1 = relu(conv(x) + b) fp32 (+ batch moments)           [G1][N][60][128]
//   aff_kernel     per-group BN affine of block l (batch moments or moving stats), pre-scaled by 1/(1-p)
//   layer_kernel   stage A_{l-1} = dropout(BN(R_{l-1})) as fp16 hi/lo into LDS (the mask of block l-1
//                  drawn from the counter hash here, by the loader waves), conv on MFMA,
//                  epilogue: bias + ReLU + moments, R_l stored fp32
//                  block 6: per-sample masked channel sums  S1 = sum_t keep*R,  S0 = sum_t keep
//   head_kernel    logit = b + (1/60) sum_c w_c (s_c S1_c + t_c S0_c)  (BN 6 + dropout 6 + GAP + Dense
//                  are linear per channel), p = sigmoid(logit)
//
// Layer kernel (CDNA4-first).  Its geometry (tiles, waves, staging units, the LDS carve, the layer table) is
// stated once in x3_geo.h and checked on the host (tests/x3_geo_check.cpp); what that header does not say:
//   * one persistent workgroup per CU (7-8 MFMA waves + 4 loader waves) walks a contiguous range of tiles;
//   * dense rows (DENSE, the batch-moment kernels of blocks 2..5, picked per call): 6.25 % fewer tiles at the
//     same wave tiling, accumulators and tile size.  A tile starts anywhere inside a window; the staging
//     writes the tile's rows plus up to PAD rows past either edge where their window also owns a row of
//     the tile, and the B-fragment address of a lane's row tile is 4 rows further down per window
//     boundary crossed (one register per row tile, recomputed per chunk).  What staging and epilogue need
//     per row is looked up in two small LDS tables the staging waves write once per tile, and global rows are
//     addressed linearly from the tile's first row (profiles/x3_row_descriptors.md).  Stored outputs are bitwise
//     those of the slot mapping (the k-order of an output element does not depend on the row tile that
//     holds it); only the grouping of the fp32 per-tile moment partials differs.  Index map:
//     x3_dense_map.h; measurements: profiles/x3_dense_rows.md;
//   * the epilogue runs on every MFMA wave of the workgroup at once (the matrix pipe idles meanwhile), so the
//     dense-row kernels keep it short: every channel tile's bias is loaded and waited for ahead of the first
//     store, so that no memory wait stands between the stores of a tile, and where a layer's loader waves have
//     the slack (block 5, mask_tab_layer) they draw the output mask during the main loop into an LDS bit table
//     that the epilogue only applies to the sign bit (profiles/x3_epilogue_offload.md);
//   * the input channels stream through LDS in chunks, double-buffered: while the MFMA waves
//     consume chunk c, the loader waves write chunk c+1 (BN affine + dropout + fp16 split of registers
//     loaded one chunk earlier) and issue the HBM loads of chunk c+2; one LDS-only barrier per chunk,
//     no vmcnt drain, and no HBM load ever queued in front of an MFMA wave's weight loads;
//   * conv = implicit GEMM  D[co][row] = sum_{tap, ci} W[tap][ci][co] A[row + tap - pad][ci]: weights are
//     the A operand (host-packed fragments, one 1-KiB coalesced load per fragment, prefetched one k-step
//     ahead), activations the B operand (LDS).  Waves tile rows x output channels (WM x WN) per layer so
//     that each weight fragment is re-read by at most WM waves of the 256-row tile.
#include "common.h"
#include "f16x3.h"
#include "x3_api.h"
#include "x3_dense_map.h"
#include "x3_geo.h"

namespace apneauq {
namespace x3 {

// Range-safe fp16 split.  The staging splits a = s_c R + t_c (BN affine x dropout rescale, R >= 0) into
// fp16 hi + lo, which needs |a| < 65504 (hi finite) and |a| well above 2^-14 (lo normal).  Per SAMPLE
// (the rows of one window in one pass / member), |a| <= max_c |s_c| * max R + max_c |t_c| =: b, so the
// sample's activations are multiplied by the exact power of two 2^sa that puts b in [2^13, 2^14), and
// the accumulator rows of that sample by 2^-sa (a conv row sums over its own sample's rows only).  The
// prescale depends on the sample's own data and the (global) affine only: results are independent of
// sharding, chunking and grouping.  Under batch moments the bound comes free with the moments instead
// (max R_c <= sqrt(sum R_c^2), aff_kernel): one power of two per group, folded into the affine, and no
// per-sample tracking in the producer's epilogue (the moments are global, so this is invariant too).
__device__ __forceinline__ int sample_prescale(unsigned rmax_bits, const float* amax) {
  return prescale_exp(__builtin_fmaf(amax[0], __uint_as_float(rmax_bits), amax[1]));
}

// global-address-space load (keeps global_load_*, never flat_*)
template <typename T>
__device__ __forceinline__ T gld(const void* p) {
  return *(const __attribute__((address_space(1))) T*)(p);
}

// Thread index the optimiser cannot see through: per-iteration address math of the persistent tile
// loop is recomputed instead of being hoisted into ~100 loop-invariant VGPRs.
__device__ __forceinline__ int opaque_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// LDS hazard barrier: orders LDS traffic only (global loads in flight stay in flight)
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// One layer of blocks 2..6 on a persistent workgroup; the template parameters are a row of the layer table and
// every constant derived from them is Cfg's (x3_geo.h).
template <int CIN, int COUT, int KS, int S, int WM, int WN, bool LAST, int LW, int CK, int WPC, bool PS, bool DENSE = false>
__global__ __launch_bounds__((WM * WN + loaders(LW)) * 64, (waves_per_eu<WM * WN + loaders(LW), WPC>())) void layer_kernel(
    const LayerArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = Cfg<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, PS, DENSE>;
  constexpr int NWM = C::NWM, kThreads = C::kThreads, kCK = CK, kRowB = C::kRowB, NQ = C::NQ, kQ = C::kQ;
  constexpr int PAD = C::PAD, kRows = C::kRows, kS = S, kBufB = C::kBufB, kValidRows = C::kValidRows;
  constexpr int SW = C::SW, kSBase = C::kSBase, kST = C::kST, kMainU = C::kMainU, kNU = C::kNU;
  constexpr int NCH = C::NCH, NCT = C::NCT, NRT = C::NRT, NSTEP = C::NSTEP, RG = C::RG, kSP = C::kSP;
  constexpr bool BDB = C::BDB;
  constexpr long long FRAG_STEP = C::FRAG_STEP;
  constexpr int kTabRows = C::kTabRows;
  constexpr bool kMaskTab = C::kMaskTab;
  constexpr bool kBiasHoist = DENSE;  // the epilogue loads every channel tile's bias ahead of its first store
  constexpr int kMtRowW = C::kMtRowW, kMtT = C::kMtT, kMtW = C::kMtW, kMtPhase = C::kMtPhase;
  // the LDS carve (x3_geo.h): moment sums, epilogue factors, and the dense-row kernels' row and mask tables
  double* st = reinterpret_cast<double*>(smem + C::st);
  float* wsc = reinterpret_cast<float*>(smem + C::wsc);
  unsigned* ektab = reinterpret_cast<unsigned*>(smem + C::ektab);
  uint2* stab = reinterpret_cast<uint2*>(smem + C::stab);
  unsigned short* mtab = reinterpret_cast<unsigned short*>(smem + C::mtab);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = (wave / WN) % WM;  // (loader waves: unused)
  const int ct0 = wn * NCT, rt0 = wm * NRT;
  const int m = lane & 15, h = lane >> 4;
  APNEAUQ_DASSERT(blockDim.x == kThreads);

  const int wg = xcd_order(blockIdx.x, gridDim.x);
  // the tile walk (x3_geo.h): tiles per group at this kernel's tile size, this workgroup's tiles
  const int tpg = tiles_per_group(DENSE, A.n_win, S);
  const int total_tiles = tpg * A.groups;
  const int t_begin = tile_begin(wg, total_tiles, gridDim.x), t_end = tile_begin(wg + 1, total_tiles, gridDim.x);
  if (t_begin >= t_end) return;  // workgroup-uniform
  const int slot = wg % kStatSlots;

  // ---- staging: staging thread i = tid - kSBase keeps the same 16-B units (C::slot_unit_row / C::unit_row,
  // channel quad q = i % kQ) of every chunk
  const bool loader = LW > 0 && wave >= NWM;
  const bool stager = LW > 0 ? loader : wave < SW;
  // C::edge_wave(wave), written out: the call in its place changes the schedule of the three dense-row kernels
  // with loader waves (profiles/x3_geo_refactor.md); the host check holds the two against each other
  const bool edge_wave = DENSE && wave >= kSBase / 64 && wave - kSBase / 64 < C::kEdgeWaves;  // wave-uniform
  // staging register set: the chunk's 16-B units + the BN affine (scale, shift) x 1/(1-p) of the
  // thread's 4 channels
  struct Stage {
    f32x4 v[kNU];
    f32x4 a, b;
  };
  Stage s0;
  // dropout keys of the current staging tile's S samples (the input's mask is drawn from the counter
  // hash of block l-1 here, at the consumer: the producer's epilogue then runs no hash at all, and the
  // loader waves' hashing overlaps the MFMA waves); recomputed when the staged tile changes
  // or the producer drew it and the input carries it in the sign bit (A.sign_in: per layer, whichever
  // side has the slack, profiles/x3_mask_side_r4.md)
  const bool hash_in = A.thr_in != 0u && !A.sign_in;
  const bool sign_in = A.thr_in != 0u && A.sign_in;
  const bool prescale = PS && A.smax_in != nullptr;
  int key_tile = -1;
  unsigned skeys[kS];
  unsigned skey_tile = 0u;  // the tile's stream key
  // prescale exponents sa of the staging tile's samples, one signed byte each (4 per register)
  unsigned sa_pack[kSP];
  auto tile_geo = [&](int tile) { return x3::tile_geo<DENSE, S>(tile, tpg, A.n_win); };
  const bool mask_out = DENSE && A.sign_out && A.thr_out != 0u;  // the epilogue draws block l's mask
  // The row tables of tile `tile` (x3_geo.h stab, ektab), one staging thread per row.  A tile's tables are
  // written with the last chunk of the tile before it (the first tile's before the first barrier): one chunk
  // barrier ahead of their first reader, the staging of the tile's chunk 0, and a whole tile after the last
  // reader of the tables they replace (tile - 2, the parity).  The slot kernels (block 6, per-sample
  // prescale) keep their per-chunk index math: block 6 measured 0.8 % slower with the tables
  // (profiles/x3_row_descriptors.md).
  auto write_tables = [&](int tile) {
    if constexpr (DENSE) {
      const int tid = opaque_tid() - kSBase;
      const Geo G = tile_geo(tile);
      const unsigned ikey = stream_key(A.seed, A.layer - 1, A.pass_base + G.g);
      const unsigned okey = stream_key(A.seed, A.layer, A.pass_base + G.g);
#pragma unroll
      for (int i0 = 0; i0 < kTabRows; i0 += kST) {
        const int i = i0 + tid, rel = i - PAD;
        if (i < kTabRows) {
          const unsigned d = dense::row_desc(rel, G.off, kRows, PAD, G.rows_left);
          const unsigned win = A.window_offset + G.wf + dense::desc_slot(d);
          const int t = dense::desc_step(d);
          stab[(tile & 1) * kTabRows + i] = uint2{d, hash_in ? dense::mask_word(sample_key(ikey, win), t) : 0u};
          if (mask_out && rel >= 0 && rel < kRows) ektab[(tile & 1) * kRows + rel] = dense::mask_word(sample_key(okey, win), t);
        }
      }
    }
  };
  // Output keep-bits of the current tile (kMaskTab, x3_geo.h mtab).  Where the epilogue stores the block's mask
  // in the sign bit (A.sign_out), the loader waves draw it during the tile's main loop, from the same ektab mask
  // words and the same hash, and the epilogue only inserts the bits: no hash and no threshold compare on an
  // MFMA wave.  One table, no parity, no barrier of its own.  Tile T's epilogue runs in the MFMA waves'
  // iteration of its chunk NCH - 1, between the chunk barriers of iterations NCH - 2 and NCH - 1; the loaders
  // write T's bits in their iterations of chunks 0 .. NCH - 2, so the last write is before the barrier ahead of
  // the epilogue and the first one after the barrier behind the epilogue of tile T - 1 (a group change only adds
  // barriers, on both sides alike).  The ektab row read here was written one barrier or more earlier, and its
  // parity is rewritten (tile T + 2) in iteration NCH - 2 of tile T + 1.
  // Iteration of chunk c < NCH - 1 of the tile: words c kMtPhase .. of the thread's kMtW words; bits 2 p,
  // 2 p + 1 of a word are the two halves of mix32(kt ^ (8 word + p)), the epilogue's
  // dropout_bits2(key, t, 16 word + 2 p)
  auto draw_mask = [&](int tile, int c) {
    if constexpr (kMaskTab) {
      const int tid = opaque_tid() - kSBase, row = tid / kMtT, w0 = (tid % kMtT) * kMtW;
      const unsigned kt = ektab[(tile & 1) * kRows + row];
      unsigned short* dst = mtab + row * kMtRowW + w0;
#pragma unroll
      for (int j = 0; j < kMtPhase; ++j) {
        const int i = c * kMtPhase + j;
        if (i < kMtW) {
          const unsigned cp = (unsigned)(w0 + i) * 8u;
          unsigned bits = 0u;
#pragma unroll
          for (int p = 0; p < 8; ++p) {
            const unsigned b = mix32(kt ^ (cp + p));
            bits |= ((b & 0xFFFFu) >= A.thr_out ? 1u : 0u) << (2 * p) | ((b >> 16) >= A.thr_out ? 1u : 0u) << (2 * p + 1);
          }
          dst[i] = (unsigned short)bits;
        }
      }
    }
  };
  auto load_chunk = [&](int tile, int c, Stage& R) {
    const int tid = opaque_tid() - kSBase, q = tid % kQ;
    const Geo G = tile_geo(tile);
    const float* af = A.aff_in + (long long)G.g * A.aff_gstride + c * kCK + 4 * q;
    R.a = gld<f32x4>(af);
    R.b = gld<f32x4>(af + CIN);
    if constexpr (DENSE) {
      // the rows of a tile are consecutive rows of the input: row rel of the tile is row row0 + rel
      const long long row0 = (A.in_shared ? 0ll : (long long)G.g * A.n_win * kL) + G.w0;
      const float* in = A.in + row0 * CIN + c * kCK + 4 * q;
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        int rel;
        bool have = C::unit_row(u, tid, edge_wave, rel);
        if (u >= kMainU) have = have && dense::staged(G.off + rel, G.off, kRows, PAD);
        R.v[u] = f32x4{-0.f, -0.f, -0.f, -0.f};
        if (have && rel < G.rows_left) R.v[u] = gld<f32x4>(in + rel * CIN);
      }
    } else {
#pragma unroll
      for (int u = 0; u < kNU; ++u) {
        const int ri = C::slot_unit_row(u, tid);
        R.v[u] = f32x4{-0.f, -0.f, -0.f, -0.f};
        if (ri < kValidRows) {
          const int s = ri / kL, t = ri - s * kL, w = G.w0 + s;
          if (w < A.n_win) {
            const long long si = A.in_shared ? w : (long long)G.g * A.n_win + w;
            R.v[u] = gld<f32x4>(A.in + (si * kL + t) * CIN + c * kCK + 4 * q);
          }
        }
      }
    }
  };
  auto store_chunk = [&](int tile, int c, char* buf, const Stage& R) {
    const int tid = opaque_tid() - kSBase, q = tid % kQ;
    const Geo G = tile_geo(tile);
    const int g = G.g, w0 = G.w0;
    // the next tile's tables, one chunk barrier before the staging of its first chunk reads them
    if (DENSE && c == NCH - 1 && tile + 1 < t_end) write_tables(tile + 1);
    if (tile != key_tile) {  // workgroup-uniform
      const unsigned skey = stream_key(A.seed, A.layer - 1, A.pass_base + g);
      skey_tile = skey;
      const float* am = A.amax_in + (A.aff_gstride ? 2 * g : 0);
      float ws0 = A.wscale[A.p_gstride ? g : 0];
      if (A.gscale_in != nullptr) ws0 *= A.gscale_in[A.aff_gstride ? g : 0];
#pragma unroll
      for (int i = 0; i < kSP; ++i) sa_pack[i] = 0u;
      // dense rows: one epilogue factor per tile (the prescale is per group)
      if (DENSE && tid == 0) wsc[(tile & 1) * kS] = ws0;
#pragma unroll
      for (int s = 0; s < (DENSE ? 0 : kS); ++s) {
        skeys[s] = sample_key(skey, A.window_offset + w0 + s);
        int sa = 0;
        if (prescale && w0 + s < A.n_win) {
          const long long si = A.in_shared ? w0 + s : (long long)g * A.n_win + w0 + s;
          sa = sample_prescale(A.smax_in[si], am);
          sa_pack[s >> 2] |= ((unsigned)sa & 0xFFu) << (8 * (s & 3));
        }
        // read by this tile's epilogue (after >= 1 barrier); the slot's previous tile (tile - 2) had its
        // epilogue before the barrier that precedes this store
        if (tid == s) wsc[(tile & 1) * kS + s] = ldexpf(ws0, -sa);
      }
      key_tile = tile;
    }
    const uint2* tab = stab + (tile & 1) * kTabRows + PAD;
#pragma unroll
    for (int u = 0; u < kNU; ++u) {
      int s, lrow;      // window slot of the tile, LDS row
      bool valid;
      unsigned kt = 0u;  // the row's input-mask word key ^ (t << 9)
      if constexpr (DENSE) {
        int rel;
        if (!C::unit_row(u, tid, edge_wave, rel)) continue;
        const uint2 e = tab[rel];  // the row's descriptor and mask word
        if (e.x == 0u) continue;   // a row that is not staged (an LDS row is >= kHalo)
        s = dense::desc_slot(e.x), lrow = dense::desc_lds_row(e.x), valid = dense::desc_valid(e.x), kt = e.y;
      } else {
        const int ri = C::slot_unit_row(u, tid);
        if (ri >= kValidRows) continue;
        s = ri / kL;
        const int t = ri - s * kL;
        lrow = kHalo + s * kSR + t, valid = w0 + s < A.n_win;
        if (hash_in) {
          // the sample's key: recomputed per staged unit (batch moments: block 2 -4 % over a select from
          // the tile's cached keys), or selected from the cache where the prescale needs its registers
          unsigned k;
          if constexpr (!PS) {
            k = sample_key(skey_tile, A.window_offset + w0 + s);
          } else {
            k = skeys[0];
#pragma unroll
            for (int j = 1; j < kS; ++j) k = s == j ? skeys[j] : k;
          }
          kt = dense::mask_word(k, t);
        }
      }
      const f32x4 v = R.v[u];
      bool keep[4];
      if (hash_in) {
        // dropout_bits2(key, t, ch) and (key, t, ch + 2) of the unit's channels ch = c kCK + 4 q
        const unsigned cp = (unsigned)(c * kCK + 4 * q) >> 1;
        const unsigned b01 = mix32(kt ^ cp), b23 = mix32(kt ^ (cp + 1u));
        keep[0] = (b01 & 0xFFFFu) >= A.thr_in;
        keep[1] = (b01 >> 16) >= A.thr_in;
        keep[2] = (b23 & 0xFFFFu) >= A.thr_in;
        keep[3] = (b23 >> 16) >= A.thr_in;
      } else if (sign_in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = !__builtin_signbit(v[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = true;
      }
      // the sample's exponent: a signed byte of sa_pack (v_bfe_i32), applied exactly by v_ldexp_f32
      int sa = 0;
      if (prescale) {
        unsigned sp = sa_pack[0];
#pragma unroll
        for (int i = 1; i < kSP; ++i) sp = (s >> 2) == i ? sa_pack[i] : sp;
        sa = __builtin_amdgcn_sbfe((int)sp, 8 * (s & 3), 8);
      }
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = (valid && keep[i]) ? ldexpf(__builtin_fmaf(v[i], R.a[i], R.b[i]), sa) : 0.f;
      uint2 hi, lo;  // 6 VALU per 4 elements (f16x3.h:split2)
      split2(a[0], a[1], hi.x, lo.x);
      split2(a[2], a[3], hi.y, lo.y);
      char* row = buf + lrow * kRowB + 8 * q;
      *reinterpret_cast<uint2*>(row) = hi;
      *reinterpret_cast<uint2*>(row + 2 * kCK) = lo;
    }
  };

  // ---- accumulators and weight fragments
  f32x4 acc[NCT][NRT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto wbase = [&](int tile) -> const gf16x8* {
    const int g = tile / tpg;
    return (const gf16x8*)(A.wfrag) + (long long)g * A.w_gstride + ct0 * 128 + lane;
  };
  f16x8 ah[NCT], al[NCT];
  auto load_a = [&](const gf16x8* p, f16x8 (&xh)[NCT], f16x8 (&xl)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      xh[ct] = p[ct * 128];
      xl[ct] = p[ct * 128 + 64];
    }
  };

  // per-lane B-fragment base: row m of the wave's first row tile, 16-B slot h, tap offset -PAD
  const int bofs = ((rt0 * 16 + m + kHalo - PAD) * kRowB) + 16 * h;

  // conv over chunk c (k-steps c*KS .. c*KS+KS-1) from LDS buffer buf; wcur: this tile's fragments,
  // wnxt: the next tile's (prefetch across the tile boundary).  hook() runs after tap KS/2: the staging
  // waves write the NEXT chunk into the other LDS buffer there, so that VALU / LDS-write work overlaps
  // the partner wave's MFMAs instead of sitting between two barriers.
  // dense rows: row tile rt of the lane lies 4 (dl / 60) LDS rows further down, dl = off + its tile row
  // (off: the tile's start inside its first window); changes per tile only
  auto compute_chunk = [&](int c, int off, const char* buf, const gf16x8* wcur, const gf16x8* wnxt, auto&& hook) {
    const char* bp[DENSE ? NRT : 1];  // the lane's base address per row tile
    if constexpr (DENSE) {
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt)
        bp[rt] = buf + bofs + (off + (dense::kSlot - kL) * ((off + (rt0 + rt) * 16 + m) / kL)) * kRowB;
    }
#pragma unroll
    for (int kk = 0; kk < NQ * KS; ++kk) {
      const int q2 = kk / KS, j = kk - q2 * KS;  // 32-channel sub-chunk, tap
      const char* bb = buf + bofs + q2 * 64;
      const int s = c * NQ * KS + kk;
      const gf16x8* np = (s + 1 < NSTEP) ? wcur + (long long)(s + 1) * FRAG_STEP : wnxt;
      // all NCT weight fragments resident, the next k-step's issued first (a full tap of MFMAs hides its
      // L2 latency); B fragments double-buffered one row tile ahead when registers allow.  The
      // sched_barriers pin that issue order (left alone, the scheduler sinks each load to its use).
      f16x8 nh[NCT], nl[NCT];
      load_a(np, nh, nl);
      __builtin_amdgcn_sched_barrier(0);
      // row tiles in groups of RG: the 3 x NCT x RG MFMAs of a group cycle through NCT x RG
      // accumulators, so a dependent MFMA follows its predecessor >= 4 issues later
      auto ldb = [&](int rt, f16x8& h_, f16x8& l_) {
        const char* br = DENSE ? bp[rt] + q2 * 64 : bb;
        h_ = *reinterpret_cast<const f16x8*>(br + (rt * 16 + j) * kRowB);
        l_ = *reinterpret_cast<const f16x8*>(br + (rt * 16 + j) * kRowB + 2 * kCK);
      };
      f16x8 bh[RG], bl[RG];
#pragma unroll
      for (int r = 0; r < RG; ++r) ldb(r, bh[r], bl[r]);
#pragma unroll
      for (int rg = 0; rg < NRT; rg += RG) {
        f16x8 bh2[RG], bl2[RG];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          bh2[r] = bh[r];
          bl2[r] = bl[r];
          if (BDB && rg + RG < NRT) ldb(rg + RG + r, bh2[r], bl2[r]);
          if (!BDB) ldb(rg + r, bh[r], bl[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < RG; ++r)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[ct][rg + r] = mfma(ah[ct], bh[r], acc[ct][rg + r]);
#pragma unroll
        for (int r = 0; r < RG; ++r)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[ct][rg + r] = mfma(al[ct], bh[r], acc[ct][rg + r]);
#pragma unroll
        for (int r = 0; r < RG; ++r)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[ct][rg + r] = mfma(ah[ct], bl[r], acc[ct][rg + r]);
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          bh[r] = bh2[r];
          bl[r] = bl2[r];
        }
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        ah[ct] = nh[ct];
        al[ct] = nl[ct];
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kk == (NQ * KS) / 2) hook();
    }
  };

  // ---- epilogue of one tile: bias + ReLU, moments, block-l dropout, store / per-sample sums
  auto epilogue = [&](int tile) {
    const int lane = opaque_tid() & 63, m = lane & 15, h = lane >> 4;
    const Geo G = tile_geo(tile);
    const int g = G.g, w0 = G.w0;  // the tile's group, its first window / first dense row
    // undo the weight prescale 2^sw and each sample's activation prescale 2^sa (exact powers of two;
    // the factors were put in LDS by the staging waves)
    float wsq[NRT / 4];
#pragma unroll
    for (int q = 0; q < NRT / 4; ++q) wsq[q] = wsc[(tile & 1) * kS + (DENSE ? 0 : (rt0 >> 2) + q)];
    const bool track = PS && !LAST && A.smax_out != nullptr;
    float mxs[NRT / 4];  // max of R_l per sample slot of the wave (range-safe split of the next block)
#pragma unroll
    for (int q = 0; q < NRT / 4; ++q) mxs[q] = 0.f;
    const float* bias = A.bias + (long long)g * A.p_gstride;
    // block 6 draws its output mask here (the masked per-sample sums); blocks 2..5 either store the plain
    // ReLU output (their consumer draws the mask while staging it) or, with A.sign_out, draw it here too
    const bool drop = (LAST || A.sign_out) && A.thr_out != 0u;
    // a wave's row tiles cover whole 64-row sample slots (NRT % 4 == 0): the sample of row tile rt is
    // wave-uniform, so its dropout key is computed once per sample (scalar ALU), not per (ct, rt, lane)
    // dense rows: the window and step of a row are per lane and row tile; the staging waves put the row's
    // mask word key ^ (t << 9) into the tile's table (ektab), one LDS read per accumulator tile.  The
    // tile's rows are consecutive rows of the output, and a row is inside the group iff it is one of the
    // first rows_left of the tile
    constexpr int NKEY = DENSE ? 1 : NRT / 4;
    unsigned skeys[NKEY];
    if (!DENSE && drop) {
      const unsigned skey = stream_key(A.seed, A.layer, A.pass_base + g);
#pragma unroll
      for (int q = 0; q < NKEY; ++q) skeys[q] = sample_key(skey, A.window_offset + w0 + (rt0 >> 2) + q);
    }
    const long long left = (long long)A.n_win * kL - w0;
    const int rows_left = DENSE ? (int)(left < kRows ? left : kRows) : 0;
    // dense rows: the bias of every channel tile is loaded, and waited for, ahead of the first store.  The
    // stores of a row tile sit behind the lanes' `valid` branch, and the memory counter is one in-order count
    // of loads and stores: with the bias load still pending on the path that skips a branch, every later row
    // tile waited for the whole counter, that is for the previous row tile's store to be acknowledged, 16
    // write round trips in a row per tile and wave while the matrix pipe stood idle
    // (profiles/x3_epilogue_offload.md).  Once nothing loaded is pending, the stores drain behind the
    // epilogue's arithmetic and the next tile's first k-step.
    f32x4 bq[kBiasHoist ? NCT : 1];
    if constexpr (kBiasHoist) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) bq[ct] = gld<f32x4>(bias + (ct0 + ct) * 16 + 4 * h);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) asm volatile("" : "+v"(bq[ct]));  // the wait lands here, once
    }
    // channel-tile outer: only one tile's 4 channels of sums are live at a time
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int co0 = (ct0 + ct) * 16 + 4 * h;
      f32x4 b4;
      if constexpr (kBiasHoist)
        b4 = bq[ct];
      else
        b4 = gld<f32x4>(bias + co0);
      f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1, k1 = s1, k0 = s1;
      // dense rows: row, address and mask word of the lane's row tiles are re-derived per channel tile (an
      // add or an LDS read each) instead of being kept in NRT registers beside the accumulators
      int mo = m;
      if constexpr (DENSE) asm volatile("" : "+v"(mo));
      const int rel0 = rt0 * 16 + mo;  // the lane's row of the wave's first row tile
      const unsigned* ek = ektab + (tile & 1) * kRows + rel0;
      const unsigned short* mt = mtab + rel0 * kMtRowW + (ct0 + ct);  // kMaskTab: the keep bits of the lane's rows
      float* orow = DENSE ? A.out + (((long long)g * A.n_win * kL + w0 + rel0) * COUT + co0) : nullptr;
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) {
        int t = 0, w = 0;
        bool valid;
        if constexpr (DENSE) {
          valid = rel0 + rt * 16 < rows_left;
        } else {
          const int s = (rt0 + rt) >> 2;
          t = (((rt0 + rt) & 3) << 4) + m, w = w0 + s, valid = t < kL && w < A.n_win;
        }
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(__builtin_fmaf(acc[ct][rt][e], wsq[rt >> 2], b4[e]), 0.f);
        acc[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        bool keep[4] = {true, true, true, true};
        unsigned sgn = 0u;  // kMaskTab: the complement of the lane's four keep bits (bits 0..3)
        if constexpr (kMaskTab) {
          if (drop) sgn = ~((unsigned)mt[rt * 16 * kMtRowW] >> (4 * h));
        } else if (drop) {
          // the row's mask word: dropout_bits2(key, t, co0) and (key, t, co0 + 2) are one xor and mix32 each
          unsigned b01, b23;
          if constexpr (DENSE) {
            const unsigned kt = ek[rt * 16];
            b01 = mix32(kt ^ ((unsigned)co0 >> 1)), b23 = mix32(kt ^ (((unsigned)co0 >> 1) + 1u));
          } else {
            b01 = dropout_bits2(skeys[rt >> 2], t, co0), b23 = dropout_bits2(skeys[rt >> 2], t, co0 + 2);
          }
          keep[0] = (b01 & 0xFFFFu) >= A.thr_out;
          keep[1] = (b01 >> 16) >= A.thr_out;
          keep[2] = (b23 & 0xFFFFu) >= A.thr_out;
          keep[3] = (b23 >> 16) >= A.thr_out;
        }
        if (valid) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s1[e] += r[e];
            s2[e] = __builtin_fmaf(r[e], r[e], s2[e]);
            if (!LAST) mxs[rt >> 2] = fmaxf(mxs[rt >> 2], r[e]);
            if constexpr (LAST) {
              k1[e] += keep[e] ? r[e] : 0.f;
              k0[e] += keep[e] ? 1.f : 0.f;
            }
          }
          if constexpr (!LAST) {
            const long long sample = (long long)g * A.n_win + w;
            f32x4 o = r;
            if constexpr (kMaskTab) {  // a dropped element takes the sign bit, a kept one stays as it is
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = __uint_as_float(__float_as_uint(r[e]) | ((sgn << (31 - e)) & 0x80000000u));
            } else if (drop) {  // the mask travels in the sign bit (-0 for a dropped zero)
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = keep[e] ? r[e] : __builtin_copysignf(r[e], -1.f);
            }
            if constexpr (DENSE)
              *reinterpret_cast<f32x4*>(orow + rt * 16 * COUT) = o;
            else
              *reinterpret_cast<f32x4*>(A.out + (sample * kL + t) * COUT + co0) = o;
          }
        }
        if constexpr (LAST) {
          if ((rt & 3) == 3) {  // the 4 row tiles of sample slot (rt0 + rt) / 4 are complete
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              k1[e] = group16_sum(k1[e]);
              k0[e] = group16_sum(k0[e]);
            }
            const int wl = w0 + (rt0 + rt) / 4;
            if (m == 0 && wl < A.n_win) {
              float* o = A.out + ((long long)g * A.n_win + wl) * (2 * COUT);
              *reinterpret_cast<f32x4*>(o + co0) = k1;
              *reinterpret_cast<f32x4*>(o + COUT + co0) = k0;
            }
            k1 = f32x4{0.f, 0.f, 0.f, 0.f};
            k0 = k1;
          }
        }
      }
      // reduce over the 16 rows of each lane group (lanes sharing h hold the same 4 channels)
      if (A.stats != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = group16_sum(s1[e]), b = group16_sum(s2[e]);
          if (m == 0) {
            atomicAdd(&st[co0 + e], (double)a);
            atomicAdd(&st[COUT + co0 + e], (double)b);
          }
        }
      }
    }
    if (track) {  // per-sample maxima of R_l (R_l >= 0: fp32 bit order = value order; max is order-free)
#pragma unroll
      for (int q = 0; q < NRT / 4; ++q) {
        const float mq = wave_max(mxs[q]);
        const int w = w0 + (rt0 >> 2) + q;
        if (lane == 0 && w < A.n_win) atomicMax(A.smax_out + (long long)g * A.n_win + w, __float_as_uint(mq));
      }
    }
  };

  auto flush_stats = [&](int g) {
    __syncthreads();
    if (A.stats != nullptr) {
      double* dst = A.stats + ((long long)g * kStatSlots + slot) * 2 * COUT;
      // (dense rows: rare, so nothing of it is kept in registers across the tile loop)
      for (int i = DENSE ? opaque_tid() : tid; i < 2 * COUT; i += kThreads) {
        atomicAdd(dst + i, st[i]);
        st[i] = 0.0;
      }
    }
    __syncthreads();
  };

  // ---- persistent loop over the flattened (tile, chunk) sequence, software-pipelined:
  //   iteration it: compute chunk it from buf[it & 1]; staging waves write chunk it+1 (loaded into
  //   registers one iteration earlier) into buf[(it+1) & 1] mid-way; barrier; issue the loads of it+2.
  // buf[(it+1) & 1] was last read by compute(it-1), which every wave finished before barrier(it-1).
  for (int i = tid; i < C::st / 16; i += kThreads) reinterpret_cast<f32x4*>(smem)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < 2 * COUT; i += kThreads) st[i] = 0.0;
  if (DENSE && stager) write_tables(t_begin);
  __syncthreads();
  const int total = (t_end - t_begin) * NCH;
  auto chunk_tile = [&](int it) { return t_begin + it / NCH; };
  // dense rows: the tile's start inside its first window
  auto tile_off = [&](int tile) { return DENSE ? (int)((long long)(tile % tpg) * kRows % kL) : 0; };
  int g_cur = t_begin / tpg;
  // a tile's first chunk: the moment sums go out when the tile starts another group (workgroup-uniform)
  auto group_change = [&](int tile, int c) {
    if (c == 0) {
      const int g = tile / tpg;
      if (g != g_cur) {
        flush_stats(g_cur);
        g_cur = g;
      }
    }
  };
  if constexpr (LW > 0) {
    // Loader and MFMA waves run the same barrier sequence: one LDS barrier before the first chunk and
    // after every chunk, and the two of flush_stats at every group change and at the end.
    if (loader) {
      // chunk it+2's HBM loads are issued right after barrier(it) and land in registers during
      // compute(it+1) (two chunks of loads in flight measured no faster: profiles/x3_epilogue_ab_r3.md)
      if (stager) {
        load_chunk(t_begin, 0, s0);
        store_chunk(t_begin, 0, smem, s0);
      }
      lds_barrier();
      if (stager && total > 1) load_chunk(chunk_tile(1), 1 % NCH, s0);
#pragma unroll 1
      for (int it = 0; it < total; ++it) {
        const int tile = chunk_tile(it), c = it - (tile - t_begin) * NCH;
        group_change(tile, c);
        // chunk it+1 into the buffer compute(it-1) read (every wave passed the barrier after it)
        if (stager && it + 1 < total) store_chunk(chunk_tile(it + 1), (it + 1) % NCH, smem + ((it + 1) & 1) * kBufB, s0);
        // this tile's output keep-bits, a share per iteration ahead of its last (kMaskTab)
        if (kMaskTab && stager && mask_out && c < NCH - 1) draw_mask(tile, c);
        lds_barrier();
        if (stager && it + 2 < total) load_chunk(chunk_tile(it + 2), (it + 2) % NCH, s0);
      }
      flush_stats(g_cur);
      return;
    }
    lds_barrier();
    load_a(wbase(t_begin), ah, al);
#pragma unroll 1
    for (int it = 0; it < total; ++it) {
      const int tile = chunk_tile(it), c = it - (tile - t_begin) * NCH;
      group_change(tile, c);
      const gf16x8* wcur = wbase(tile);
      const gf16x8* wnxt = wbase(tile + 1 < t_end ? tile + 1 : tile);
      compute_chunk(c, tile_off(tile), smem + (it & 1) * kBufB, wcur, wnxt, []() {});
      if (c == NCH - 1) epilogue(tile);
      lds_barrier();
    }
    flush_stats(g_cur);
    return;
  }
  if (stager) {
    load_chunk(t_begin, 0, s0);
    store_chunk(t_begin, 0, smem, s0);
  }
  lds_barrier();
  if (stager && total > 1) load_chunk(chunk_tile(1), 1 % NCH, s0);
  load_a(wbase(t_begin), ah, al);
#pragma unroll 1
  for (int it = 0; it < total; ++it) {
    const int tile = chunk_tile(it), c = it - (tile - t_begin) * NCH;
    group_change(tile, c);
    const gf16x8* wcur = wbase(tile);
    const gf16x8* wnxt = wbase(tile + 1 < t_end ? tile + 1 : tile);
    char* buf = smem + (it & 1) * kBufB;
    char* nbuf = smem + ((it + 1) & 1) * kBufB;
    compute_chunk(c, tile_off(tile), buf, wcur, wnxt, [&]() {
      if (stager && it + 1 < total) store_chunk(chunk_tile(it + 1), (it + 1) % NCH, nbuf, s0);
    });
    if (c == NCH - 1) epilogue(tile);
    lds_barrier();
    if (stager && it + 2 < total) load_chunk(chunk_tile(it + 2), (it + 2) % NCH, s0);
  }
  flush_stats(g_cur);
}

// ------------------------------------------------------------------------------- block 1 (fp32)
// R_1[g][w][t][c] = relu(b[c] + sum_{j, ci} x[w][t + j - 3][ci] W[j][ci][c]) in fp32 FMAs, 8 windows
// per 256-thread block (thread = one output channel x one half of the time steps), + batch moments.
__global__ __launch_bounds__(256) void l1_kernel(const L1Args A) {
  __shared__ float xs[kL1Win][kL + 6][4];
  __shared__ float red[2][2][128];
  __shared__ unsigned wmax[kL1Win];  // per-window max of R_1 (fp32 bits)
  const int g = blockIdx.x / A.blocks_per_group;
  const int w0 = (blockIdx.x - g * A.blocks_per_group) * kL1Win;
  const int tid = threadIdx.x, c = tid & 127, half = tid >> 7;
  for (int i = tid; i < kL1Win * (kL + 6) * 4; i += 256) {
    const int s = i / ((kL + 6) * 4), r = (i / 4) % (kL + 6), ci = i & 3;
    const int t = r - 3, w = w0 + s;
    xs[s][r][ci] = (t >= 0 && t < kL && w < A.n_win) ? A.x[((long long)w * kL + t) * 4 + ci] : 0.f;
  }
  float wr[7][4];
#pragma unroll
  for (int j = 0; j < 7; ++j)
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) wr[j][ci] = A.w[(((long long)g * 7 + j) * 4 + ci) * 128 + c];
  const float bc = A.b[g * 128 + c];
  if (tid < kL1Win) wmax[tid] = 0u;
  __syncthreads();
  float s1 = 0.f, s2 = 0.f;
  for (int s = 0; s < kL1Win; ++s) {
    const int w = w0 + s;
    if (w >= A.n_win) break;
    float* o = A.out + (((long long)g * A.n_win + w) * kL) * 128 + c;
    float mx = 0.f;
    for (int t = half * 30; t < half * 30 + 30; ++t) {
      float v = bc;
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) v = __builtin_fmaf(xs[s][t + j][ci], wr[j][ci], v);
      v = fmaxf(v, 0.f);
      o[t * 128] = v;
      s1 += v;
      s2 = __builtin_fmaf(v, v, s2);
      mx = fmaxf(mx, v);
    }
    if (A.smax != nullptr) {
      mx = wave_max(mx);
      if ((tid & 63) == 0) atomicMax(&wmax[s], __float_as_uint(mx));
    }
  }
  if (A.stats != nullptr || A.smax != nullptr) {  // block-uniform
    red[half][0][c] = s1;
    red[half][1][c] = s2;
    __syncthreads();
    if (A.stats != nullptr && tid < 128) {
      double* dst = A.stats + ((long long)g * kStatSlots + (blockIdx.x % kStatSlots)) * 2 * 128;
      atomicAdd(dst + c, (double)red[0][0][c] + (double)red[1][0][c]);
      atomicAdd(dst + 128 + c, (double)red[0][1][c] + (double)red[1][1][c]);
    }
    // every window belongs to this block alone: a plain store of its max
    if (A.smax != nullptr && tid < kL1Win && w0 + tid < A.n_win) A.smax[(long long)g * A.n_win + w0 + tid] = wmax[tid];
  }
}

// ---------------------------------------------------------------------- BN affine (+ moving update)
// aff[g][0][c] = gamma * rstd * dsc, aff[g][1][c] = (beta - mean * gamma * rstd) * dsc, where (mean, var)
// are the biased batch moments of group g (stats != nullptr) or the moving statistics.  With
// update != 0 the Keras moving averages are updated once per group in group order (one MC-Dropout
// pass after the other, the side effect of model(x, training=True)).  amax[g] = (max_c |aff scale|,
// max_c |aff shift|): the consumer's range-safe split (sample_prescale).
// Blocks 0..groups-1: group g's affine (independent); block `groups` (batch moments with the moving
// update only): the moving averages, groups in order (the recurrence is sequential; the affines use
// the batch moments, so the two never touch the same data).  One block looping over every group's
// affine and its two block reductions took ~25 us per call.
__device__ __forceinline__ void aff_moments(const AffArgs& A, int g, int c, float& mean, float& var) {
  const double* p = A.stats + (long long)g * kStatSlots * 2 * A.C + c;
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int s = 0; s < kStatSlots; ++s) {
    a += p[s * 2 * A.C];
    b += p[s * 2 * A.C + A.C];
  }
  const double mu = a * A.inv_count;
  mean = (float)mu;
  var = (float)fmax(b * A.inv_count - mu * mu, 0.0);
}

__global__ __launch_bounds__(256) void aff_kernel(const AffArgs A) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x == A.groups) {  // the moving-average side effect (launched with stats + update)
    for (int c = tid; c < A.C; c += 256)
      for (int g = 0; g < A.groups; ++g) {
        const long long po = (long long)g * A.p_gstride + c;
        float mean, var;
        aff_moments(A, g, c, mean, var);
        for (int r = 0; r < A.repeat; ++r) {
          A.mmean[po] = A.mmean[po] * A.momentum + mean * (1.f - A.momentum);
          A.mvar[po] = A.mvar[po] * A.momentum + var * (1.f - A.momentum);
        }
      }
    return;
  }
  {
    const int g = blockIdx.x;
    float ms = 0.f, mt = 0.f;
    for (int c = tid; c < A.C; c += 256) {
      const long long po = (long long)g * A.p_gstride + c;
      float mean, var;
      if (A.stats != nullptr && !A.running) {
        aff_moments(A, g, c, mean, var);
      } else {
        mean = A.mmean[po];
        var = A.mvar[po];
      }
      const float sc = A.gamma[po] / sqrtf(var + A.eps);
      const float s_ = sc * A.dsc, t_ = (A.beta[po] - mean * sc) * A.dsc;
      A.aff[((long long)g * 2) * A.C + c] = s_;
      A.aff[((long long)g * 2 + 1) * A.C + c] = t_;
      if (A.gscale != nullptr) {
        // batch moments: R >= 0 gives max R_c <= sqrt(sum R_c^2) over the group's rows (of all ranks), so
        // b = max_c |s_c| sqrt(sum R_c^2) + |t_c| bounds every staged |a| of the group (with A.running the
        // affine is the moving statistics' and the sums of squares serve only this bound)
        const double* p = A.stats + (long long)g * kStatSlots * 2 * A.C + A.C + c;
        double q = 0.0;
        for (int s = 0; s < kStatSlots; ++s) q += p[s * 2 * A.C];
        ms = fmaxf(ms, __builtin_fmaf(fabsf(s_), (float)sqrt(fmax(q, 0.0)) * 1.0001f, fabsf(t_)));
      } else {
        ms = fmaxf(ms, fabsf(s_));
        mt = fmaxf(mt, fabsf(t_));
      }
    }
    if (A.gscale != nullptr) {
      // per-group power of two 2^sa putting the bound in [2^13, 2^14), folded into the affine; the layer
      // kernel multiplies its accumulators by gscale = 2^-sa
      ms = wave_max(ms);
      if ((tid & 63) == 0) red[0][tid >> 6] = ms;
      __syncthreads();
      const float bnd = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
      int e = 0;
      if (bnd > 0.f && bnd < INFINITY) frexpf(bnd, &e);
      const int sa = min(100, max(-100, 14 - e));
      for (int c = tid; c < A.C; c += 256) {
        float* af = A.aff + (long long)g * 2 * A.C + c;
        af[0] = ldexpf(af[0], sa);
        af[A.C] = ldexpf(af[A.C], sa);
      }
      if (tid == 0) A.gscale[g] = ldexpf(1.f, -sa);
      return;
    }
    if (A.amax == nullptr) return;  // kernel-uniform
    ms = wave_max(ms);
    mt = wave_max(mt);
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = ms;
      red[1][tid >> 6] = mt;
    }
    __syncthreads();
    if (tid == 0) {
      A.amax[2 * g] = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
      A.amax[2 * g + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
  }
}

// --------------------------------------------------------------------------------------- head
// p[g][w] = sigmoid(b + (1/60) sum_c w_c (aff_s[c] S1[c] + aff_t[c] S0[c])): one wave per sample.
__global__ __launch_bounds__(256) void head_kernel(const HeadArgs A) {
  const int lane = threadIdx.x & 63;
  const long long sidx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sidx >= A.samples) return;
  const int g = (int)(sidx / A.n_win);
  const float* s = A.sums + sidx * 2 * A.C;
  const float* af = A.aff + (long long)g * A.aff_gstride;
  const float* dw = A.dw + (long long)g * A.p_gstride;
  float v = 0.f;
  for (int c = lane; c < A.C; c += 64) v += dw[c] * __builtin_fmaf(af[c], s[c], af[A.C + c] * s[A.C + c]);
  v = wave_sum(v);
  if (lane == 0) {
    const float logit = v * (1.0f / kL) + A.db[A.p_gstride ? g : 0];
    A.out[sidx] = A.out_logits ? logit : 1.0f / (1.0f + expf(-logit));
  }
}

// ------------------------------------------------------------------------------- launch helpers
template <int CIN, int COUT, int KS, int S, int WM, int WN, bool LAST, int LW, int CK, int WPC, bool PS, bool DENSE = false>
hipError_t launch_layer(const LayerArgs& A, int grid, hipStream_t stream) {
  using C = Cfg<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, PS, DENSE>;
  auto k = layer_kernel<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, PS, DENSE>;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, C::bytes);
    if (e != hipSuccess) return e;
    attr = true;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(C::kThreads), C::bytes, stream, A);
  return hipGetLastError();
}

// the dense-row instantiation of a layer, compiled only where the layer table asks for it
template <bool HAVE, int CIN, int COUT, int KS, int S, int WM, int WN, int LW, int CK, int WPC>
hipError_t launch_dense(const LayerArgs& A, int grid, hipStream_t stream) {
  if constexpr (HAVE) {
    return launch_layer<CIN, COUT, KS, S, WM, WN, false, dense_lw(LW, WM, WN), CK, WPC, false, true>(A, grid, stream);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace x3

x3::LayerInfo x3_layer_info(int layer) { return x3::layer_info(layer); }

// the kernels of the layer table (x3_geo.h)
hipError_t x3_launch_layer(int layer, const x3::LayerArgs& A, int grid, bool dense_rows, hipStream_t stream) {
  using namespace x3;
  // the per-sample prescale variant only where it is used (moving statistics)
  const bool ps = A.smax_in != nullptr || A.smax_out != nullptr;
#define APNEAUQ_X3_LAUNCH(L, CI, CO, K, S, WM, WN, LAST, LW, LWB, CK, WPC, DENSE)                                  \
  if (layer == L) {                                                                                       \
    if (dense_rows)                                                                                       \
      return ps ? hipErrorInvalidValue                                                                    \
                : launch_dense<DENSE && !LAST, CI, CO, K, S, WM, WN, LWB, CK, WPC>(A, grid, stream);       \
    return ps ? launch_layer<CI, CO, K, S, WM, WN, LAST, LW, CK, WPC, true>(A, grid, stream)               \
              : launch_layer<CI, CO, K, S, WM, WN, LAST, LWB, CK, WPC, false>(A, grid, stream);            \
  }
  APNEAUQ_X3_LAYERS(APNEAUQ_X3_LAUNCH)
#undef APNEAUQ_X3_LAUNCH
  return hipErrorInvalidValue;
}

hipError_t x3_launch_l1(const x3::L1Args& A, hipStream_t stream) {
  const int grid = A.groups * A.blocks_per_group;
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(x3::l1_kernel, dim3(grid), dim3(256), 0, stream, A);
  return hipGetLastError();
}

hipError_t x3_launch_aff(const x3::AffArgs& A, hipStream_t stream) {
  const int blocks = A.groups + (A.stats != nullptr && A.update ? 1 : 0);
  hipLaunchKernelGGL(x3::aff_kernel, dim3(blocks), dim3(256), 0, stream, A);
  return hipGetLastError();
}

hipError_t x3_launch_head(const x3::HeadArgs& A, hipStream_t stream) {
  if (A.samples <= 0) return hipSuccess;
  hipLaunchKernelGGL(x3::head_kernel, dim3((A.samples + 3) / 4), dim3(256), 0, stream, A);
  return hipGetLastError();
}

}  // namespace apneauq
