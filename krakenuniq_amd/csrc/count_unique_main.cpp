// count_unique: HyperLogLog estimate of the distinct k-mers of a library on the GPU through ku_sketch_* -- the reference's
// count_unique (src/count_unique.cpp; scripts/build_db.sh:127, cat_library | count_unique -k K).  As there, every unambiguous
// FORWARD k-mer is hashed (no canonical form), the registers are dense whatever the input's size, and the number printed is
// min(windows observed, Ertl's estimate).  The input goes through the same stage as kmer_db's (plain, .gz / BGZF, .bz2).
//
// Differences from the reference: files may be named (it reads standard input only); -C sketches canonical k-mers; -v; a -p
// outside 4..18 is a usage error (64) where the reference aborts (134) on an uncaught exception; -t is accepted and ignored,
// also above the processor count, which the reference refuses (64).
#include <getopt.h>

#include <chrono>

#include "ku_tool.h"

const char *const ku_tool::name = "count_unique";
using ku_tool::exit_code_of;

static void usage(int code) {
  fprintf(stderr,
          "Usage: count_unique [-k 31] [-p 14] [-t n] [-C] [-v] [file ...]\n"
          "  Estimate the number of distinct k-mers in the input using HLL.\n"
          "Options:\n"
          "  -k #          Length of k-mers (1..31) [31]\n"
          "  -p INT        HLL precision (4..18) [14]\n"
          "  -t #          Number of threads (accepted; the work is done on the GPU)\n"
          "  -C            Count canonical k-mers (the reference counts forward ones)\n"
          "  -v            Verbose output: bytes, windows, seconds and MB/s\n"
          "  -h            Print this message\n"
          "Input: FASTA, plain or .gz / .bz2; '-' or no file reads standard input.  KU_DEVICE selects the GPU.\n");
  exit(code);
}

int main(int argc, char **argv) {
  long long k = 31, p = 14;
  bool canonical = false, verbose = false;
  int opt;
  while ((opt = getopt(argc, argv, "k:p:t:Cvh")) != -1) {
    switch (opt) {
      case 'k':
        k = atoll(optarg);
        if (k <= 0) fatal(EX_USAGE, "k can't be <= 0");
        if (k > 31) fatal(EX_USAGE, "k can't be > 31");
        break;
      case 'p':
        p = atoll(optarg);
        if (p < 4 || p > 18) fatal(EX_USAGE, "HLL precision out of range (-p 4..18)");
        break;
      case 't': if (atoll(optarg) <= 0) fatal(EX_USAGE, "can't use nonpositive thread count"); break;
      case 'C': canonical = true; break;
      case 'v': verbose = true; break;
      case 'h': usage(0); break;
      default: usage(EX_USAGE);
    }
  }
  bool from_stdin = false;
  const std::vector<std::string> inputs = ku_tool::input_list(argc, argv, optind, from_stdin);
  ku_tool::require_readable(inputs);

  ku_sketch *h = nullptr;
  int st = ku_sketch_open(ku_tool::device(), (uint32_t)k, (uint32_t)p, canonical ? KU_SKETCH_CANONICAL : 0u, 0, 1, 0, &h);
  if (st != KU_OK) fatal(exit_code_of(st), "%s", ku_last_error());
  auto check = [&](int status) { ku_tool::check(status, [&] { ku_sketch_close(h); }); };
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t n_records = 0, n_bytes = 0;
  ku_tool::for_each_record(inputs, [&](const std::string &, const char *seq, size_t len) {
    check(ku_sketch_add(h, seq, len));
    ++n_records;
    n_bytes += len;
  });
  uint64_t estimate = 0, windows = 0;
  check(ku_sketch_estimate(h, &estimate));
  if (verbose) check(ku_sketch_export(h, nullptr, &windows));
  ku_sketch_close(h);
  if (n_records == 0) fprintf(stderr, "count_unique: no sequence in the input\n");
  if (verbose) {
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "count_unique: %llu records, %llu bytes, %llu windows, %.3f s, %.1f MB/s\n", (unsigned long long)n_records,
            (unsigned long long)n_bytes, (unsigned long long)windows, s, s > 0 ? n_bytes / 1e6 / s : 0.0);
  }
  printf("%llu\n", (unsigned long long)estimate);
  return 0;
}
