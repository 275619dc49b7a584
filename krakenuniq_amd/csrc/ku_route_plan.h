// ku_route_plan.h -- the round planner of the owner-routed step (ku_mgpu_route.h): where a rank's slice of a batch is cut
// into rounds of whole reads.  Host C++ over the standard library and the status codes only: bin/route_plan_check runs
// it without a device (tests/test_route_plan.py).
//
// The slice holds nr reads over nb positions that start at p0 in the buffer; R rounds (every rank runs the same number: it
// owns bins in all of them).  A round ends on a read boundary: the first position of every round's first read.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "krakenuniq_amd.h"

namespace {
struct RoutePlanRound {
  uint64_t a = 0, sb = 0;   // first position (relative to the slice) and bytes to scan
  uint64_t ra = 0, rn = 0;  // the round's reads (relative to the slice's first read)
};

// A source of read offsets: int fetch(const uint64_t *idx, uint32_t n, uint64_t *out) puts the buffer offset of read idx[i]
// (relative to the slice's first read) into out[i] and returns a status.  A host array answers at once; for a device array
// every call is one round trip, so the planner asks for everything it wants to know at one time in one call.
struct RouteHostOffsets {
  const uint64_t *off;  // of the slice's first read
  int operator()(const uint64_t *idx, uint32_t n, uint64_t *out) const {
    for (uint32_t i = 0; i < n; ++i) out[i] = off[idx[i]];
    return KU_OK;
  }
};

// rounds[0 .. R), of RoutePlanRound or a type derived from it.  KU_EINVAL: the cuts do not ascend inside the slice (the
// reads are not in buffer order); a status of the source's is passed on.  No error text is set here.  On failure the
// rounds are empty ones.
template <class Round, class Source>
int ku_route_plan(uint64_t nr, uint64_t nb, uint64_t p0, uint32_t R, uint64_t round_pos, Source &&fetch, std::vector<Round> &rounds) {
  rounds.assign(R, Round{});
  std::vector<uint64_t> cut(R + 1, nb), rc(R + 1);
  cut[0] = 0;
  for (uint32_t i = 0; i <= R; ++i) rc[i] = nr * i / R;
  if (R > 1 && nr) {
    std::vector<uint64_t> idx, val(R);
    // cut[1 .. R) from the offsets of reads rc[1 .. R) (a round that starts behind the last read is empty); must ascend
    auto cuts_of_reads = [&]() -> int {
      idx.clear();
      for (uint32_t i = 1; i < R; ++i)
        if (rc[i] < nr) idx.push_back(rc[i]);
      if (!idx.empty())
        if (int st = fetch(idx.data(), (uint32_t)idx.size(), val.data())) return st;
      for (uint32_t i = 1, j = 0; i < R; ++i) cut[i] = rc[i] < nr ? val[j++] - p0 : nb;
      for (uint32_t i = 1; i < R; ++i)
        if (cut[i] < cut[i - 1] || cut[i] > nb) return KU_EINVAL;
      return KU_OK;
    };
    if (int st = cuts_of_reads()) return st;
    // Equal numbers of READS per round are equal numbers of positions only when the reads are about equally long.  With
    // contigs among short reads a round could hold far more than round_pos positions -- its queues more records than a
    // ticket can number.  Then the rounds are cut by POSITION: round i starts at the first read at or behind
    // i / R of the slice, found by a bisection over the offsets: R - 1 values per step, one fetch per step.
    uint64_t widest = 0;
    for (uint32_t i = 0; i < R; ++i) widest = std::max(widest, cut[i + 1] - cut[i]);
    if (widest > round_pos + round_pos / 2) {
      std::vector<uint64_t> lo(R, 0), hi(R, nr), target(R, 0);  // first read with offset >= target_i lies in [lo, hi]
      for (uint32_t i = 1; i < R; ++i) target[i] = p0 + nb / R * i;
      for (;;) {
        idx.clear();
        for (uint32_t i = 1; i < R; ++i)
          if (lo[i] < hi[i]) idx.push_back((lo[i] + hi[i]) / 2);
        if (idx.empty()) break;
        if (int st = fetch(idx.data(), (uint32_t)idx.size(), val.data())) return st;
        for (uint32_t i = 1, j = 0; i < R; ++i)
          if (lo[i] < hi[i]) {
            const uint64_t mid = (lo[i] + hi[i]) / 2;
            if (val[j++] < target[i]) lo[i] = mid + 1; else hi[i] = mid;
          }
      }
      for (uint32_t i = 1; i < R; ++i) rc[i] = lo[i] = std::max(lo[i], lo[i - 1]);
      if (int st = cuts_of_reads()) return st;
    }
  }
  for (uint32_t i = 0; i < R; ++i) static_cast<RoutePlanRound &>(rounds[i]) = {cut[i], cut[i + 1] - cut[i], rc[i], rc[i + 1] - rc[i]};
  return KU_OK;
}
}  // namespace
