// route_plan_check -- test aid for the routed step's round planner (ku_route_plan.h, tests/test_route_plan.py): host code, no GPU library.
//   route_plan_check P0 NB R ROUND_POS < offsets
// plans the rounds of one slice: its reads' buffer offsets come from standard input (decimal, white space between them),
// the slice holds NB positions from P0 on.  Prints, once for the host-array source and once for a batched source that
// counts its fetches (what a device array costs in round trips):
//   <source> status <status> fetches <n>
//   <a> <sb> <ra> <rn>          one line per round, when the status is 0
// Exit status 0 whatever the planner answers; 64 for a bad command line.
#include <cstdio>
#include <cstdlib>

#include "ku_route_plan.h"

namespace {
struct CountingOffsets {
  const std::vector<uint64_t> &off;
  uint32_t *fetches;
  int operator()(const uint64_t *idx, uint32_t n, uint64_t *out) const {
    ++*fetches;
    for (uint32_t i = 0; i < n; ++i) {
      if (idx[i] >= off.size()) return KU_ESTATE;  // the planner asked for a read the slice does not have
      out[i] = off[idx[i]];
    }
    return KU_OK;
  }
};

void print(const char *source, int st, uint32_t fetches, const std::vector<RoutePlanRound> &rounds) {
  printf("%s status %d fetches %u\n", source, st, fetches);
  if (st != KU_OK) return;
  for (const auto &x : rounds)
    printf("%llu %llu %llu %llu\n", (unsigned long long)x.a, (unsigned long long)x.sb, (unsigned long long)x.ra, (unsigned long long)x.rn);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 5) {
    fprintf(stderr, "Usage: route_plan_check P0 NB R ROUND_POS < offsets\n");
    return 64;
  }
  const uint64_t p0 = strtoull(argv[1], nullptr, 10), nb = strtoull(argv[2], nullptr, 10), round_pos = strtoull(argv[4], nullptr, 10);
  const uint32_t R = (uint32_t)strtoul(argv[3], nullptr, 10);
  if (R == 0) {
    fprintf(stderr, "route_plan_check: R must be at least 1\n");
    return 64;
  }
  std::vector<uint64_t> off;
  unsigned long long v;
  while (scanf("%llu", &v) == 1) off.push_back(v);
  std::vector<RoutePlanRound> rounds;
  int st = ku_route_plan(off.size(), nb, p0, R, round_pos, RouteHostOffsets{off.data()}, rounds);
  print("host", st, 0, rounds);
  uint32_t fetches = 0;
  st = ku_route_plan(off.size(), nb, p0, R, round_pos, CountingOffsets{off, &fetches}, rounds);
  print("batched", st, fetches, rounds);
  return 0;
}
