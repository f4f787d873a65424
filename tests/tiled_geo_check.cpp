// Host check of the XCD-aware workgroup order (csrc/xcd_order.h) and of the slot geometry of the fused
// tiled kernels (csrc/fused_tiled_geo.h) against brute force.  Stand-alone: built and run by
// tests/test_tiled_geo_cpu.py with the host compiler.
//   * xcd_order(., nwg, nx) is a bijection of [0, nwg), and the workgroups with equal bid % nx (one XCD)
//     get one contiguous range, in order;
//   * for each of the four (net, precision) types and each block: the GEMM-row -> slot-row map is the
//     one a walk over samples and rows gives; every computed row that is stored lands inside its own
//     sample's slot (input and output side); every tap T0..T1-1 of every computed row reads a row inside
//     [-lead, max_act + trail); a tap of a stored row reads the sample's own valid row or a zero row; and
//     no skipped tap could have reached a valid row.
#include <cstdio>
#include <vector>

#include "fused_tiled_geo.h"
#include "xcd_order.h"

using namespace apneauq;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (failures++ < 20) {                     \
        std::printf("FAIL %s: ", #cond);         \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
    }                                            \
  } while (0)

static void check_order(int nwg, int nx) {
  std::vector<int> seen(nwg, 0), last(nx, -1);
  for (int bid = 0; bid < nwg; ++bid) {
    const int id = xcd_order(bid, nwg, nx);
    CHECK(id >= 0 && id < nwg, "nwg %d nx %d bid %d -> %d", nwg, nx, bid, id);
    if (id < 0 || id >= nwg) continue;
    ++seen[id];
    // the XCD's ids are consecutive in dispatch order
    const int x = bid % nx;
    CHECK(last[x] < 0 || id == last[x] + 1, "nwg %d nx %d bid %d: %d follows %d", nwg, nx, bid, id, last[x]);
    last[x] = id;
  }
  for (int id = 0; id < nwg; ++id) CHECK(seen[id] == 1, "nwg %d nx %d: id %d taken %d times", nwg, nx, id, seen[id]);
  // the ranges of the XCDs follow each other: XCD x + 1 starts where XCD x ends
  int next = 0;
  for (int x = 0; x < nx && x < nwg; ++x) {
    CHECK(xcd_order(x, nwg, nx) == next, "nwg %d nx %d: XCD %d starts at %d, not %d", nwg, nx, x, xcd_order(x, nwg, nx), next);
    next = last[x] + 1;
  }
  CHECK(next == nwg, "nwg %d nx %d: ranges end at %d", nwg, nx, next);
}

template <class N, int L>
static void check_block(const char* name) {
  using G = tgeo::Geo<N, L>;
  constexpr int NS = N::NS, OPS = N::OPS[L], SIN = N::SIN[L], LIN = N::LIN[L];
  const int rows = tgeo::gemm_rows<N>(L);
  const bool rowhead = G::HEAD && tgeo::rowhead<N>();
  if (L > 0) CHECK(N::LOUT[L - 1] == LIN, "%s block %d: input length", name, L);

  if (L == 0) {
    // block 1 reads x0: NS slots of X0ROWS rows behind x0_lead rows, kX0Trail rows after them
    const int lo = -tgeo::x0_lead<N>(), hi = NS * N::X0ROWS + tgeo::kX0Trail;
    for (int o = 0; o < rows; ++o) {
      // im2col: the row itself; else the lane groups h = 0..3 read rows o + 2h - PAD and the next one
      const int first = N::IM2COL ? o : o - G::PAD, last = N::IM2COL ? o : o + 2 * 3 - G::PAD + 1;
      CHECK(first >= lo && last < hi, "%s block 1 row %d reads x0 rows %d..%d", name, o, first, last);
      CHECK(o / OPS < NS, "%s block 1 row %d: past the last sample", name, o);
    }
  } else {
    const int lead = tgeo::lead_bytes<N>(), end = tgeo::max_act<N>() + tgeo::trail_bytes<N>();
    int o = 0;
    for (int s = 0; o < rows; ++s) {
      for (int t = 0; t < OPS && o < rows; ++t, ++o) {
        const int want = rowhead ? o : s * SIN + t;  // brute force: the t-th row of sample s's slot
        const int row = tgeo::slot_row<N>(L, o);
        CHECK(row == want, "%s block %d row %d -> slot row %d, not %d", name, L + 1, o, row, want);
        // (block 6 stores no rows, and both kernels mask its rows past the last sample out of the head)
        if (!N::P::kGuardsTail && !G::HEAD) CHECK(s < NS, "%s block %d row %d: past the last sample, unguarded", name, L + 1, o);
        for (int tap = N::T0[L]; tap < N::T1[L]; ++tap) {
          const int r = row + tap - G::PAD;
          CHECK(r * G::SI >= -lead && (r + 1) * G::SI <= end, "%s block %d row %d tap %d reads row %d", name, L + 1, o, tap, r);
        }
        // rows whose value is used: the LOUT stored rows (both rows of a pooled pair)
        const int used = G::POOL ? 2 * N::LOUT[L] : N::LOUT[L];
        if (s >= NS || t >= used) continue;
        CHECK(row >= s * SIN && row < (s + 1) * SIN, "%s block %d row %d outside its slot", name, L + 1, o);
        for (int tap = 0; tap < G::K; ++tap) {
          const int ti = t + tap - G::PAD;  // input step of this tap
          const bool valid = ti >= 0 && ti < LIN;
          if (tap < N::T0[L] || tap >= N::T1[L]) {
            CHECK(!valid, "%s block %d row %d: skipped tap %d reaches step %d", name, L + 1, o, tap, ti);
            continue;
          }
          const int r = row + tap - G::PAD;
          if (valid)
            CHECK(r == s * SIN + ti, "%s block %d row %d tap %d", name, L + 1, o, tap);
          else  // in front of the first slot, behind the last, or a slot's zero rows LIN .. SIN-1
            CHECK(r < 0 || r >= NS * SIN || r % SIN >= LIN, "%s block %d row %d tap %d: row %d is not zero", name, L + 1, o, tap, r);
        }
        if (!G::HEAD) {
          const int tout = G::POOL ? t >> 1 : t;
          CHECK(tout < G::SOUT, "%s block %d row %d stored outside its output slot", name, L + 1, o);
          CHECK((s * G::SOUT + tout + 1) * G::SO <= tgeo::max_act<N>(), "%s block %d row %d stored past the buffer", name, L + 1, o);
        }
      }
    }
  }
}

template <class N>
static int check_net(const char* name) {
  static_assert(tgeo::net_ok<N>(), "geometry");
  check_block<N, 0>(name);
  check_block<N, 1>(name);
  check_block<N, 2>(name);
  check_block<N, 3>(name);
  check_block<N, 4>(name);
  check_block<N, 5>(name);
  return 6;
}

int main() {
  int cases = 0;
  const int xcds[] = {1, 2, 4, 8};
  for (int nwg = 1; nwg <= 300; ++nwg)
    for (int nx : xcds) {
      check_order(nwg, nx);
      ++cases;
    }
  cases += check_net<tiled::PooledNet>("bf16 pooled");
  cases += check_net<tiled::Single30Net>("bf16 single30");
  cases += check_net<tiled3::PooledNet>("x3 pooled");
  cases += check_net<tiled3::Single30Net>("x3 single30");
  // the tables the four types share, and what each precision adds
  static_assert(tiled::PooledNet::NS == 8 && tiled::Single30Net::NS == 4 && tiled3::PooledNet::NS == 4 &&
                    tiled3::Single30Net::NS == 2,
                "samples per workgroup");
  static_assert(tgeo::max_act<tiled::PooledNet>() == 69632 && tgeo::max_act<tiled3::PooledNet>() == 67584, "max_act");
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
