// kmer_db: library FASTA -> sorted database.kdb + database.idx on the GPU through ku_kmerdb_*.  It stands where the
// reference's build runs Jellyfish 1 and db_sort (scripts/build_db.sh:140-146 and :201): no k-mer list is written in
// between, the values are 0 as after db_sort -z, and set_lcas follows as before.  The input goes through the same stage as
// set_lcas's -F file (plain, .gz / BGZF, .bz2); with -P above 1 it is read once per pass.  -P auto reads it once more,
// beforehand: one HyperLogLog sketch per range of the bin keys (ku_sketch_*) tells the smallest pass count that fits the budget.
#include <getopt.h>

#include <algorithm>

#include "ku_kmerdb_budget.h"
#include "ku_tool.h"

const char *const ku_tool::name = "kmer_db";
using ku_tool::exit_code_of;

// the output files once ku_kmerdb_open has created them: a fatal error of the input stage (an unreadable or corrupt library, in
// whichever pass; possibly on one of the reader's threads) must not leave an unfinished database behind
static std::string g_unfinished[2];
static void unlink_unfinished() {
  for (const std::string &path : g_unfinished)
    if (!path.empty()) unlink(path.c_str());
}

static void usage(int code) {
  fprintf(stderr,
          "Usage: kmer_db [-k 31] -n NT -o database.kdb -i database.idx [-P passes] [-s device_bytes(K/M/G)] [-t threads] [-v]\n"
          "               library.fa [more.fa ...]\n\n"
          "Options: (*mandatory)\n"
          "* -n #             Length of the minimizer bin keys (1..15)\n"
          "* -o filename      Output database (sorted, values 0: what db_sort -z writes)\n"
          "* -i filename      Output index\n"
          "  -k #             K-mer length (default 31; at most 31, at least -n)\n"
          "  -P #|auto        Passes over the input, each building a range of the bins (default 1; files only, no stdin).\n"
          "                   auto: the smallest power of two that fits -s, found by sketching the library first\n"
          "  -s #[K|M|G]      Device memory for collecting the k-mers (default: half of what is free)\n"
          "  -t #             Number of threads (accepted; the input stage sizes its own teams)\n"
          "  -v               Verbose output: per pass the windows, candidates, flushes and distinct k-mers\n"
          "  -h               Print this message\n\n"
          "Input: FASTA, plain or .gz / .bz2; '-' or no file reads standard input.  KU_DEVICE selects the GPU.\n");
  exit(code);
}

// -P auto: one sketch of the canonical k-mers per range of the bin keys (min(1024, 4^nt) ranges, p = 12), taken in a pass of its
// own and closed before the builder measures the free memory; then the smallest power-of-two pass count whose fullest pass
// fits the collection buffer of the budget with a tenth to spare (ku_sketch_plan_passes).  Without -s the budget is half of
// what is free when the builder opens: a handle opened for the purpose reports the capacity it got, and the build then asks
// for that budget by its size.
static long long plan_passes(int device, uint32_t k, uint32_t nt, const std::vector<std::string> &inputs,
                             const std::string &kdb_name, const std::string &idx_name, uint64_t &device_bytes, bool verbose) {
  const uint32_t p = 12, n_groups = (uint32_t)std::min<uint64_t>(1024, 1ull << (2 * nt));
  if (device_bytes && device_bytes < KU_KMERDB_MIN_BYTES) fatal(EX_USAGE, "the device budget is below the minimum of 64 KiB");
  ku_sketch *sk = nullptr;
  int st = ku_sketch_open(device, k, p, KU_SKETCH_CANONICAL, nt, n_groups, 0, &sk);
  if (st != KU_OK) fatal(exit_code_of(st), "%s", ku_last_error());
  auto check = [&](int status) { ku_tool::check(status, [&] { ku_sketch_close(sk); }); };
  ku_tool::for_each_record(inputs, [&](const std::string &, const char *seq, size_t len) { check(ku_sketch_add(sk, seq, len)); });
  std::vector<uint8_t> registers((size_t)n_groups << p);
  check(ku_sketch_export(sk, registers.data(), nullptr));
  ku_sketch_close(sk);
  if (device_bytes == 0) {
    ku_kmerdb *probe = nullptr;
    ku_kmerdb_stats got{};
    st = ku_kmerdb_open(device, k, nt, 1, 0, kdb_name.c_str(), idx_name.c_str(), &probe);
    if (st == KU_OK) st = ku_kmerdb_get_stats(probe, &got);
    const std::string msg = st == KU_OK ? "" : ku_last_error();
    ku_kmerdb_close(probe);  // (removes the two empty files again)
    if (st != KU_OK) fatal(exit_code_of(st), "%s", msg.c_str());
    device_bytes = got.capacity * 16 + got.segment_bytes;
  }
  const uint64_t usable = ku_kmerdb_budget(device_bytes).usable;
  uint32_t n_passes = 0;
  uint64_t fullest = 0;
  st = ku_sketch_plan_passes(registers.data(), n_groups, p, usable, &n_passes, &fullest);
  if (st != KU_OK)
    fatal(EX_SOFTWARE, "no pass count up to %u fits the device budget: %s (a larger -s)", n_groups, ku_last_error());
  if (verbose)
    fprintf(stderr, "kmer_db: planned passes: %u (fullest range ≈ %llu k-mers of %llu)\n", n_passes, (unsigned long long)fullest,
            (unsigned long long)usable);
  return n_passes;
}

int main(int argc, char **argv) {
  std::string kdb_name, idx_name;
  long long k = 31, nt = 0, passes = 1;
  uint64_t device_bytes = 0;
  bool verbose = false, auto_passes = false;
  if (argc < 2) usage(EX_USAGE);
  int opt;
  while ((opt = getopt(argc, argv, "k:n:o:i:P:s:t:vh")) != -1) {
    switch (opt) {
      case 'k': k = atoll(optarg); break;
      case 'n': nt = atoll(optarg); break;
      case 'o': kdb_name = optarg; break;
      case 'i': idx_name = optarg; break;
      case 'P':
        auto_passes = strcmp(optarg, "auto") == 0;
        passes = auto_passes ? 1 : atoll(optarg);
        break;
      case 's':
        if (!ku_tool::parse_bytes(optarg, device_bytes) || device_bytes == 0) fatal(EX_USAGE, "-s takes a positive size, such as 512M or 8G");
        break;
      case 't': if (atoll(optarg) <= 0) fatal(EX_USAGE, "can't use nonpositive thread count"); break;
      case 'v': verbose = true; break;
      case 'h': usage(0); break;
      default: usage(EX_USAGE);
    }
  }
  if (kdb_name.empty() || idx_name.empty() || nt == 0) usage(EX_USAGE);
  if (nt < 1 || nt > 15) fatal(EX_USAGE, "bin key length out of range (-n 1..15)");
  if (k < nt || k > 31) fatal(EX_USAGE, "k-mer length out of range (-k %lld..31)", nt);
  if (passes < 1 || passes > (1ll << (2 * nt))) fatal(EX_USAGE, "-P out of range (1..4^nt)");
  bool from_stdin = false;
  const std::vector<std::string> inputs = ku_tool::input_list(argc, argv, optind, from_stdin);
  if (from_stdin && auto_passes) fatal(EX_USAGE, "-P auto needs files: the input is read once per pass, standard input can be read only once");
  if (from_stdin && passes > 1) fatal(EX_USAGE, "-P %lld needs files: the input is read once per pass, standard input can be read only once", passes);

  // the outputs are created (and whatever was at their paths truncated) when the handle opens: not for an input that is not there
  ku_tool::require_readable(inputs);

  const int device = ku_tool::device();
  if (auto_passes) passes = plan_passes(device, (uint32_t)k, (uint32_t)nt, inputs, kdb_name, idx_name, device_bytes, verbose);

  ku_kmerdb *h = nullptr;
  int st = ku_kmerdb_open(device, (uint32_t)k, (uint32_t)nt, (uint32_t)passes, device_bytes, kdb_name.c_str(),
                          idx_name.c_str(), &h);
  if (st != KU_OK) fatal(exit_code_of(st), "%s", ku_last_error());
  g_unfinished[0] = kdb_name;
  g_unfinished[1] = idx_name;
  ku_tool::on_fatal = unlink_unfinished;
  auto check = [&](int status) { ku_tool::check(status, [&] { ku_kmerdb_close(h); }); };  // (the close removes the unfinished files)
  ku_kmerdb_stats stats{};
  for (long long p = 0; p < passes; ++p) {
    uint64_t n_records = 0;
    ku_tool::for_each_record(inputs, [&](const std::string &, const char *seq, size_t len) {
      check(ku_kmerdb_add(h, seq, len));
      ++n_records;
    });
    check(ku_kmerdb_end_pass(h));
    check(ku_kmerdb_get_stats(h, &stats));
    if (verbose)
      fprintf(stderr, "kmer_db: pass %lld/%lld: %llu records, %llu windows, %llu candidates, %llu flushes, %llu merge calls, %llu segments, %llu distinct k-mers\n",
              p + 1, passes, (unsigned long long)n_records, (unsigned long long)stats.windows, (unsigned long long)stats.candidates,
              (unsigned long long)stats.flushes, (unsigned long long)stats.merge_calls, (unsigned long long)stats.segments,
              (unsigned long long)stats.distinct);
  }
  uint64_t key_ct = 0;
  check(ku_kmerdb_finish(h, &key_ct));
  g_unfinished[0].clear();  // a database now
  g_unfinished[1].clear();
  check(ku_kmerdb_get_stats(h, &stats));
  ku_kmerdb_close(h);
  if (verbose)
    fprintf(stderr, "kmer_db: %llu distinct k-mers in all (buffer of %llu k-mers, segments of %llu bytes); scan %.3f s, sort and merge %.3f s, "
                    "bin order and output %.3f s\n",
            (unsigned long long)key_ct, (unsigned long long)stats.capacity, (unsigned long long)stats.segment_bytes, stats.scan_s,
            stats.flush_s, stats.end_pass_s);
  return 0;
}
