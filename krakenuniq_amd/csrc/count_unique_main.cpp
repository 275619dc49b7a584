// count_unique: HyperLogLog estimate of the distinct k-mers of a library on the GPU through ku_sketch_* -- the reference's
// count_unique (src/count_unique.cpp; scripts/build_db.sh:127, cat_library | count_unique -k K).  As there, every unambiguous
// FORWARD k-mer is hashed (no canonical form), the registers are dense whatever the input's size, and the number printed is
// min(windows observed, Ertl's estimate).  The input goes through the same stage as kmer_db's (plain, .gz / BGZF, .bz2).
//
// Differences from the reference: files may be named (it reads standard input only); -C sketches canonical k-mers; -v; a -p
// outside 4..18 is a usage error (64) where the reference aborts (134) on an uncaught exception; -t is accepted and ignored,
// also above the processor count, which the reference refuses (64).
#include <getopt.h>
#include <sysexits.h>
#include <unistd.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/krakenuniq_amd.h"
#include "ku_seqio.h"
#include "ku_fasta.h"

void ku_seqio::fatal(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "count_unique: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(code);
}
using ku_seqio::fatal;

static int exit_code_of(int st) {
  switch (st) {
    case KU_EINVAL: return EX_USAGE;
    case KU_EDATA: return EX_DATAERR;
    case KU_ENOINPUT: return EX_NOINPUT;
    case KU_ENOMEM: return EX_OSERR;
    default: return EX_SOFTWARE;
  }
}

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
  std::vector<std::string> inputs;
  bool from_stdin = optind >= argc;
  for (int i = optind; i < argc; ++i) {
    if (strcmp(argv[i], "-") == 0) from_stdin = true;
    else inputs.push_back(argv[i]);
  }
  if (from_stdin && !inputs.empty()) fatal(EX_USAGE, "standard input cannot be combined with files");
  if (from_stdin) inputs.push_back("/dev/stdin");
  for (const std::string &path : inputs)
    if (access(path.c_str(), R_OK) != 0) fatal(EX_NOINPUT, "can't open %s", path.c_str());

  ku_sketch *h = nullptr;
  const char *dev_env = getenv("KU_DEVICE");
  int st = ku_sketch_open(dev_env ? atoi(dev_env) : 0, (uint32_t)k, (uint32_t)p, canonical ? KU_SKETCH_CANONICAL : 0u, 0, 1, 0, &h);
  if (st != KU_OK) fatal(exit_code_of(st), "%s", ku_last_error());
  auto check = [&](int status) {
    if (status == KU_OK) return;
    const std::string msg = ku_last_error();
    ku_sketch_close(h);
    fatal(exit_code_of(status), "%s", msg.c_str());
  };
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t n_records = 0, n_bytes = 0;
  for (const std::string &path : inputs) {
    ku_seqio::FastaRecords fa(path);
    std::string id;
    const char *seq;
    size_t len;
    while (fa.next(id, seq, len)) {
      check(ku_sketch_add(h, seq, len));
      ++n_records;
      n_bytes += len;
    }
  }
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
