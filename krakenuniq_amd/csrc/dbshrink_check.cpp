// dbshrink_check -- test aid for db_shrink's arithmetic (ku_dbshrink_rule.h) and chunk plan (ku_dbshrink_budget.h;
// tests/test_db_shrink_host.py): host code, no GPU library.  This is where counts above 2^32 are exercised.
//   dbshrink_check < cases
// One case per line of standard input, decimal numbers with white space between them; one line of output per case:
//   src  KEY_CT N_OUT OFFSET j...        ->  src(j) of every j given (j < N_OUT)
//   S    KEY_CT N_OUT OFFSET x...        ->  S(x) of every x given (x <= KEY_CT)
//   all  KEY_CT N_OUT OFFSET             ->  src(0) .. src(N_OUT - 1), then "|", then S(0) .. S(KEY_CT)
//   plan KEY_CT N_OUT OFFSET BUDGET      ->  chunk_records offset_slice n_chunks, then "lo hi S(lo) S(hi)" of every chunk,
//                                            each behind a "|"
// A rule that ku_db_shrink_files would refuse (N_OUT of 0 or above KEY_CT, OFFSET of 0 or above the block size), a j or an
// x out of range, or a budget below the minimum prints "invalid".  Exit status 0; 64 for a line that cannot be read.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ku_dbshrink_budget.h"
#include "ku_dbshrink_rule.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    if (!(in >> what)) continue;
    uint64_t key_ct, n_out, offset;
    if (!(in >> key_ct >> n_out >> offset)) {
      fprintf(stderr, "dbshrink_check: cannot read '%s'\n", line.c_str());
      return 64;
    }
    std::vector<uint64_t> args;
    for (uint64_t v; in >> v;) args.push_back(v);
    if (!in.eof()) {
      fprintf(stderr, "dbshrink_check: cannot read '%s'\n", line.c_str());
      return 64;
    }
    if (!ku_shrink_rule_ok(key_ct, n_out, offset)) {
      printf("invalid\n");
      continue;
    }
    const KuShrinkRule r = ku_shrink_rule(key_ct, n_out, offset);
    bool ok = true;
    std::string out;
    auto put = [&](uint64_t v) { out += (out.empty() ? "" : " ") + std::to_string(v); };
    if (what == "src") {
      for (uint64_t j : args) {
        ok = ok && j < n_out;
        if (ok) put(ku_shrink_src(r, j));
      }
    } else if (what == "S") {
      for (uint64_t x : args) {
        ok = ok && x <= key_ct;
        if (ok) put(ku_shrink_S(r, x));
      }
    } else if (what == "all" && args.empty()) {
      for (uint64_t j = 0; j < n_out; ++j) put(ku_shrink_src(r, j));
      out += " |";
      for (uint64_t x = 0; x <= key_ct; ++x) put(ku_shrink_S(r, x));
    } else if (what == "plan" && args.size() == 1) {
      ok = args[0] >= 65536;  // KU_DBSHRINK_MIN_BYTES (include/krakenuniq_amd.h)
      if (ok) {
        const KuDbShrinkBudget b = ku_dbshrink_budget(args[0]);
        const uint64_t n_chunks = ku_dbshrink_chunks(key_ct, b.chunk_records);
        put(b.chunk_records);
        put(b.offset_slice);
        put(n_chunks);
        for (uint64_t c = 0; c < n_chunks; ++c) {
          uint64_t lo, hi;
          ku_dbshrink_chunk(key_ct, b.chunk_records, c, lo, hi);
          out += " |";
          put(lo);
          put(hi);
          put(ku_shrink_S(r, lo));
          put(ku_shrink_S(r, hi));
        }
      }
    } else {
      fprintf(stderr, "dbshrink_check: cannot read '%s'\n", line.c_str());
      return 64;
    }
    printf("%s\n", ok ? out.c_str() : "invalid");
  }
  return 0;
}
