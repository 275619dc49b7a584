// db_shrink: drop-in for the reference's db_shrink (src/db_shrink.cpp), on the GPU through ku_db_shrink_files: keeps -n of a
// list's records, evenly spread, the one -O places before the end of each block.  With -i / -I the input is a sorted
// database and its index, and the output is a sorted database with its index, ready for classify: the db_sort that
// scripts/shrink_db.sh runs over the shrunk list is not needed.
#include <getopt.h>

#include "ku_tool.h"

const char *const ku_tool::name = "db_shrink";

static void usage(int code) {
  fprintf(stderr,
          "Usage: db_shrink [-O offset] [-i in.idx -I out.idx] [-s device_bytes(K/M/G)] [-v] <-d input db> <-o output db> <-n output count>\n\n"
          "Options: (*mandatory)\n"
          "* -d filename      Input list or database (Jellyfish-1 list format)\n"
          "* -o filename      Output list or database\n"
          "* -n #             Number of records to keep\n"
          "  -O #             Of every block, keep the record this many places before its end (default: 1, the last)\n"
          "  -i filename      Index of the input, a sorted database: with -I, the output is a sorted database too\n"
          "  -I filename      Output index (same minimizer length as the input's)\n"
          "  -s #[K|M|G]      Device memory for the run (default: half of what is free; at least 64K)\n"
          "  -v               Verbose output: one line of statistics\n"
          "  -h               Print this message\n\n"
          "KU_DEVICE selects the GPU.\n");
  exit(code);
}

int main(int argc, char **argv) {
  std::string in_name, out_name, in_idx, out_idx;
  uint64_t n_out = 0, offset = 1, device_bytes = 0;
  bool verbose = false;
  if (argc > 1 && strcmp(argv[1], "-h") == 0) usage(0);
  int opt;
  long long sig;
  while ((opt = getopt(argc, argv, "d:o:n:O:i:I:s:vh")) != -1) {
    switch (opt) {
      case 'n':
        sig = atoll(optarg);
        if (sig < 1) fatal(EX_USAGE, "output count must be positive");
        n_out = (uint64_t)sig;
        break;
      case 'd': in_name = optarg; break;
      case 'o': out_name = optarg; break;
      case 'O':
        sig = atoll(optarg);
        if (sig < 1) fatal(EX_USAGE, "offset count cannot be negative");
        offset = (uint64_t)sig;
        break;
      case 'i': in_idx = optarg; break;
      case 'I': out_idx = optarg; break;
      case 's':
        if (!ku_tool::parse_bytes(optarg, device_bytes) || device_bytes == 0) fatal(EX_USAGE, "-s takes a positive size, such as 512M or 8G");
        break;
      case 'v': verbose = true; break;
      case 'h': usage(0); break;
      default: usage(EX_USAGE);
    }
  }
  if (in_name.empty() || out_name.empty() || !n_out || optind != argc) usage(EX_USAGE);
  if (in_idx.empty() != out_idx.empty()) fatal(EX_USAGE, "-i and -I go together: the index of the input and the index to write");
  std::vector<std::string> inputs{in_name};
  if (!in_idx.empty()) inputs.push_back(in_idx);
  ku_tool::require_readable(inputs);  // (before anything is created at the output paths)

  ku_db_shrink_stats stats{};
  const int st = ku_db_shrink_files(ku_tool::device(), in_name.c_str(), in_idx.empty() ? nullptr : in_idx.c_str(), n_out, offset,
                                    device_bytes, out_name.c_str(), out_idx.empty() ? nullptr : out_idx.c_str(), &stats);
  ku_tool::check(st, [] {});
  if (verbose)
    fprintf(stderr, "db_shrink: %llu of %llu records written (blocks of %llu records, %llu of them one longer), %llu chunks (at most %llu "
                    "records each); read %.3f s, select %.3f s, output %.3f s\n",
            (unsigned long long)stats.key_ct_out, (unsigned long long)stats.key_ct_in, (unsigned long long)stats.block_size,
            (unsigned long long)stats.odd_blocks, (unsigned long long)stats.chunks, (unsigned long long)stats.chunk_records, stats.read_s,
            stats.select_s, stats.write_s);
  return 0;
}
