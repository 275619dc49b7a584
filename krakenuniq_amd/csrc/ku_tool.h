// ku_tool.h -- what the database build programs share (db_sort, set_lcas, kmer_db, count_unique, db_merge, db_shrink): the fatal exit of the
// program and of its input stage, the exit code of a library status, the device to use, the size that -s takes, the list of input
// files, and the loop over their FASTA records.  Plain C++ over the C ABI, no HIP.
#pragma once
#include <sysexits.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/krakenuniq_amd.h"
#include "ku_seqio.h"
#include "ku_fasta.h"

namespace ku_tool {

extern const char *const name;        // defined by the program: "kmer_db"
inline void (*on_fatal)() = nullptr;  // the program's clean-up, first thing in fatal(): possibly on one of the reader's threads

inline int exit_code_of(int st) {
  switch (st) {
    case KU_EINVAL: return EX_USAGE;
    case KU_EDATA: return EX_DATAERR;
    case KU_ENOINPUT: return EX_NOINPUT;
    case KU_ENOMEM: return EX_OSERR;
    default: return EX_SOFTWARE;
  }
}

inline int device() {  // KU_DEVICE selects the GPU
  const char *dev_env = getenv("KU_DEVICE");
  return dev_env ? atoi(dev_env) : 0;
}

// a byte count with an optional K / M / G suffix (powers of 1024), as -s takes it
inline bool parse_bytes(const char *txt, uint64_t &out) {
  char *end = nullptr;
  const unsigned long long v = strtoull(txt, &end, 10);
  if (end == txt || *txt == '-') return false;
  uint64_t mul = 1;
  if (*end == 'K' || *end == 'k') mul = 1ull << 10, ++end;
  else if (*end == 'M' || *end == 'm') mul = 1ull << 20, ++end;
  else if (*end == 'G' || *end == 'g') mul = 1ull << 30, ++end;
  if (*end) return false;
  out = v * mul;
  return true;
}

}  // namespace ku_tool

// "<program>: <message>\n" on stderr, then exit(code); also what the input stage (ku_seqio.h) calls
inline void ku_seqio::fatal(int code, const char *fmt, ...) {
  if (ku_tool::on_fatal) ku_tool::on_fatal();
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "%s: ", ku_tool::name);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(code);
}
using ku_seqio::fatal;

namespace ku_tool {

// the inputs named by argv[first ..]: files, or standard input for '-' or for no argument at all
inline std::vector<std::string> input_list(int argc, char **argv, int first, bool &from_stdin) {
  std::vector<std::string> inputs;
  from_stdin = first >= argc;
  for (int i = first; i < argc; ++i) {
    if (strcmp(argv[i], "-") == 0) from_stdin = true;
    else inputs.push_back(argv[i]);
  }
  if (from_stdin && !inputs.empty()) fatal(EX_USAGE, "standard input cannot be combined with files");
  if (from_stdin) inputs.push_back("/dev/stdin");
  return inputs;
}

// an input that is not there is reported before any work is done (and before any output is created)
inline void require_readable(const std::vector<std::string> &inputs) {
  for (const std::string &path : inputs)
    if (access(path.c_str(), R_OK) != 0) fatal(EX_NOINPUT, "can't open %s", path.c_str());
}

// a failed library call ends the program; `close` releases the handle first (the error text is taken before it does)
template <typename Close>
void check(int status, Close close) {
  if (status == KU_OK) return;
  const std::string msg = ku_last_error();
  close();
  fatal(exit_code_of(status), "%s", msg.c_str());
}

// fn(id, seq, len) for every record of every input, in order
template <typename Fn>
void for_each_record(const std::vector<std::string> &inputs, Fn fn) {
  for (const std::string &path : inputs) {
    ku_seqio::FastaRecords fa(path);
    std::string id;
    const char *seq;
    size_t len;
    while (fa.next(id, seq, len)) fn(id, seq, len);
  }
}

}  // namespace ku_tool
