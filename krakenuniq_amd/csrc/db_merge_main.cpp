// db_merge: the union of sorted databases (database.kdb + database.idx pairs) as one sorted database, on the GPU through
// ku_db_merge_files.  It is what adding a library to a database needs: kmer_db over the new library, db_merge of the
// database and the result, set_lcas -F over the new library alone.  With -b the values of k-mers that several inputs hold
// are folded with lca(), so two databases that went through set_lcas apart can be combined as well.
#include <getopt.h>

#include "ku_tool.h"

const char *const ku_tool::name = "db_merge";
using ku_tool::exit_code_of;

static void usage(int code) {
  fprintf(stderr,
          "Usage: db_merge [-b taxDB] [-s device_bytes(K/M/G)] [-v] -o out.kdb -i out.idx  A.kdb A.idx  B.kdb B.idx [...]\n\n"
          "Options: (*mandatory)\n"
          "* -o filename      Output database\n"
          "* -i filename      Output index\n"
          "  -b filename      Taxonomy (taxDB): the values of a k-mer that several inputs hold are folded to their LCA.\n"
          "                   Without it such values have to be equal, or all but one of them 0\n"
          "  -s #[K|M|G]      Device memory for the merge (default: half of what is free; at least 64K)\n"
          "  -v               Verbose output: one line of statistics\n"
          "  -h               Print this message\n\n"
          "Input: 2 to 8 database / index pairs with the same k and minimizer length.  KU_DEVICE selects the GPU.\n");
  exit(code);
}

int main(int argc, char **argv) {
  std::string kdb_name, idx_name, taxdb_name;
  uint64_t device_bytes = 0;
  bool verbose = false;
  if (argc < 2) usage(EX_USAGE);
  int opt;
  while ((opt = getopt(argc, argv, "b:o:i:s:vh")) != -1) {
    switch (opt) {
      case 'b': taxdb_name = optarg; break;
      case 'o': kdb_name = optarg; break;
      case 'i': idx_name = optarg; break;
      case 's':
        if (!ku_tool::parse_bytes(optarg, device_bytes) || device_bytes == 0) fatal(EX_USAGE, "-s takes a positive size, such as 512M or 8G");
        break;
      case 'v': verbose = true; break;
      case 'h': usage(0); break;
      default: usage(EX_USAGE);
    }
  }
  if (kdb_name.empty() || idx_name.empty()) usage(EX_USAGE);
  const int n_args = argc - optind;
  if (n_args % 2 != 0 || n_args < 4) usage(EX_USAGE);
  if (n_args > 16) fatal(EX_USAGE, "at most 8 database / index pairs");
  std::vector<std::string> inputs(argv + optind, argv + argc);
  if (!taxdb_name.empty()) inputs.push_back(taxdb_name);
  ku_tool::require_readable(inputs);  // (before anything is created at the output paths)

  ku_tax *tax = nullptr;
  if (!taxdb_name.empty()) {
    const int st = ku_tax_open(taxdb_name.c_str(), &tax);
    if (st != KU_OK) fatal(exit_code_of(st), "%s", ku_last_error());
  }
  std::vector<const char *> kdbs, idxs;
  for (int i = optind; i < argc; i += 2) {
    kdbs.push_back(argv[i]);
    idxs.push_back(argv[i + 1]);
  }
  ku_db_merge_stats stats{};
  const int st = ku_db_merge_files(ku_tool::device(), kdbs.data(), idxs.data(), (uint32_t)kdbs.size(), tax, device_bytes,
                                   kdb_name.c_str(), idx_name.c_str(), &stats);
  ku_tool::check(st, [&] { ku_tax_close(tax); });
  ku_tax_close(tax);
  if (verbose)
    fprintf(stderr, "db_merge: %llu records written, %llu duplicates, %llu folded, %llu chunks (at most %llu records each); "
                    "upload %.3f s, merge %.3f s, output %.3f s\n",
            (unsigned long long)stats.key_ct, (unsigned long long)stats.duplicates, (unsigned long long)stats.folded,
            (unsigned long long)stats.chunks, (unsigned long long)stats.capacity, stats.upload_s, stats.merge_s, stats.write_s);
  return 0;
}
