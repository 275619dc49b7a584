// ku_fasta.h -- the library FASTA of the database build tools (set_lcas, kmer_db), one record at a time through the
// classify executable's reader (ku_seqio.h): plain, .gz / BGZF and .bz2 files, line breaks inside a record removed.
#pragma once
#include <string>

#include "ku_seqio.h"

namespace ku_seqio {

struct FastaRecords {
  ku_seqio::Reader rd;
  ku_seqio::Batch bt;
  std::string header;
  explicit FastaRecords(const std::string &path) {
    bt.pinned = false;  // ku_setlcas_add / ku_kmerdb_add take ordinary host memory
    rd.open(path.c_str(), /*prefetch=*/true);
    rd.fastq = false;  // FastaReader regardless of the first byte (src/set_lcas.cpp:245,422)
  }
  ~FastaRecords() { bt.release(); }
  bool next(std::string &id, const char *&seq, size_t &len) {
    size_t n = 0, lo, hi;
    bt.clear();
    bt.begin_read();
    if (!ku_seqio::next_record(rd, bt, &header, nullptr, &n)) return false;
    bt.end_read();
    ku_seqio::split_id(header.data(), header.size(), lo, hi);
    id.assign(header, lo, hi - lo);
    seq = bt.seqs + bt.off.back();
    len = bt.len.back();
    return true;
  }
};

}  // namespace ku_seqio
