// ku_dbfiles.h -- the one writer of a database.kdb + database.idx pair (db_sort, kmer_db, db_merge, db_shrink, which also
// writes a list without an index; csrc/dbfiles_check.cpp runs it without a device).  Plain C++ and POSIX, no HIP: the caller brings the bytes from wherever they are.
//   database.kdb  a Jellyfish-1 list header as KrakenDB reads it (krakendb.cpp:60-78,177; key_ct at byte 48), then the records
//   database.idx  "KRAKIX2" or "KRAKIDX", the nt byte, then 4^nt + 1 offsets (make_index, krakendb.cpp:118-148)
// Files of a run that did not reach the end of finish() are not databases: none is left behind.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

inline bool write_all(int fd, const void *buf, size_t n) {
  const char *p = (const char *)buf;
  while (n) {
    ssize_t w = ::write(fd, p, n < ((size_t)1 << 30) ? n : ((size_t)1 << 30));
    if (w <= 0) return false;
    p += w;
    n -= (size_t)w;
  }
  return true;
}

// the zeroed header of a list of k-mers of key_bits bits with 4-byte values; finish() patches key_ct in
inline std::vector<uint8_t> ku_jflist_header(uint64_t key_bits) {
  const uint64_t val_len = 4;
  std::vector<uint8_t> hdr(72 + 2 * (4 + 8 * key_bits), 0);
  memcpy(hdr.data(), "JFLISTDN", 8);
  memcpy(hdr.data() + 8, &key_bits, 8);
  memcpy(hdr.data() + 16, &val_len, 8);
  return hdr;
}

// Every operation returns false on failure and leaves the text for KU_ENOINPUT in `error`; a failure is final (finish() does
// not succeed after one), and the files go when the object does.
struct KuDbFiles {
  std::string kdb_path, idx_path, error;
  int kdb_fd = -1, idx_fd = -1;
  bool made_kdb = false, made_idx = false;  // created here, and not yet a finished database
  bool bad = false;
  bool with_idx = true;  // false: a list without an index

  KuDbFiles() = default;
  KuDbFiles(const KuDbFiles &) = delete;
  KuDbFiles &operator=(const KuDbFiles &) = delete;
  ~KuDbFiles() { abandon(); }

  // creates and truncates both files
  bool open(const std::string &kdb, const std::string &idx) {
    kdb_path = kdb;
    idx_path = idx;
    made_kdb = (kdb_fd = ::open(kdb.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) >= 0;
    if (!made_kdb) return failed("can't write " + kdb_path);
    made_idx = (idx_fd = ::open(idx.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) >= 0;
    if (!made_idx) return failed("can't write " + idx_path);
    return true;
  }
  // a list without an index (db_shrink's list mode): creates and truncates the .kdb alone; begin() and finish() then leave
  // the index out, and append_offsets() fails
  bool open(const std::string &kdb) {
    kdb_path = kdb;
    with_idx = false;
    made_kdb = (kdb_fd = ::open(kdb.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) >= 0;
    return made_kdb || failed("can't write " + kdb_path);
  }
  // the database header as handed in; the index's magic (idx_type 1: KRAKIDX, else KRAKIX2) and its nt byte
  bool begin(const void *kdb_header, size_t n, uint32_t idx_type, uint32_t nt) {
    const uint8_t nt8 = (uint8_t)nt;
    if (!with_idx) return put(kdb_fd, kdb_path, kdb_header, n);
    return put(kdb_fd, kdb_path, kdb_header, n) && put(idx_fd, idx_path, idx_type == 1 ? "KRAKIDX" : "KRAKIX2", 7) &&
           put(idx_fd, idx_path, &nt8, 1);
  }
  bool append_records(const void *p, size_t bytes) { return put(kdb_fd, kdb_path, p, bytes); }
  bool append_offsets(const void *p, size_t bytes) { return put(idx_fd, idx_path, p, bytes); }
  // offsets[4^nt] = key_ct (make_index, krakendb.cpp:136-139); key_ct into the header (krakendb.cpp:72); both files closed.
  // True: every step of the run succeeded, and the files stay.
  bool finish(uint64_t key_ct) {
    if (with_idx) put(idx_fd, idx_path, &key_ct, 8);
    if (!bad && ::pwrite(kdb_fd, &key_ct, 8, 48) != 8) failed("write error on " + kdb_path);
    if (!bad && close_fd(idx_fd) != 0) failed("write error on " + idx_path);
    if (!bad && close_fd(kdb_fd) != 0) failed("write error on " + kdb_path);
    if (bad) return abandon(), false;
    made_kdb = made_idx = false;
    return true;
  }
  // closes what is open and removes what was created, unless finish() succeeded
  void abandon() {
    close_fd(kdb_fd);
    close_fd(idx_fd);
    if (made_kdb) ::unlink(kdb_path.c_str());
    if (made_idx) ::unlink(idx_path.c_str());
    made_kdb = made_idx = false;
  }

 private:
  static int close_fd(int &fd) {
    const int r = fd >= 0 ? ::close(fd) : 0;
    fd = -1;
    return r;
  }
  bool failed(const std::string &msg) {
    if (!bad) error = msg;
    bad = true;
    return false;
  }
  bool put(int fd, const std::string &path, const void *p, size_t n) {
    if (bad || fd < 0 || !write_all(fd, p, n)) return failed("write error on " + path);
    return true;
  }
};
