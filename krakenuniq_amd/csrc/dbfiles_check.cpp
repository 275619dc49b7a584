// dbfiles_check -- test aid for the database writer (ku_dbfiles.h, tests/test_dbfiles.py): host code, no GPU library.
//   dbfiles_check DIR
// runs the writer's cases inside DIR, which must exist, and prints one line per case: "<case> ok" or "<case> FAILED: <why>".
// Every path written lies inside DIR.  Exit status 0 when every case is ok.
#include <signal.h>
#include <sys/resource.h>
#include <sys/stat.h>

#include <cstdio>

#include "ku_dbfiles.h"

namespace {

bool exists(const std::string &p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}

int n_failed = 0;
void report(const char *name, bool ok, const std::string &why) {
  printf("%s %s%s%s\n", name, ok ? "ok" : "FAILED", ok ? "" : ": ", ok ? "" : why.c_str());
  if (!ok) ++n_failed;
}

// the small database of the test: nt = 2, k = 31 (key_len 8), thirteen records (the writer does not look at their order)
constexpr uint32_t NT = 2, K = 31, N_REC = 13, N_BINS = 16;
void small_db(std::vector<uint8_t> &recs, std::vector<uint64_t> &off) {
  recs.clear();
  for (uint32_t i = 0; i < N_REC; ++i) {
    const uint64_t key = 0x0123456789abcdefULL * (i + 1) & ((1ull << (2 * K)) - 1);
    const uint32_t val = 100 + i;
    const uint8_t *kp = (const uint8_t *)&key, *vp = (const uint8_t *)&val;
    recs.insert(recs.end(), kp, kp + 8);
    recs.insert(recs.end(), vp, vp + 4);
  }
  off.assign(N_BINS, N_REC);  // one record in each of the first thirteen bins (the closing offset is finish()'s)
  for (uint32_t b = 0; b < N_REC; ++b) off[b] = b;
}

bool write_run(KuDbFiles &f, const std::string &kdb, const std::string &idx, bool in_two_pieces) {
  std::vector<uint8_t> recs;
  std::vector<uint64_t> off;
  small_db(recs, off);
  const std::vector<uint8_t> hdr = ku_jflist_header(2 * K);
  if (!f.open(kdb, idx) || !f.begin(hdr.data(), hdr.size(), 2, NT)) return false;
  const size_t cut_r = in_two_pieces ? 5 * 12 : recs.size(), cut_o = in_two_pieces ? 7 : off.size();
  return f.append_records(recs.data(), cut_r) && f.append_records(recs.data() + cut_r, recs.size() - cut_r) &&
         f.append_offsets(off.data(), cut_o * 8) && f.append_offsets(off.data() + cut_o, (off.size() - cut_o) * 8);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "Usage: dbfiles_check DIR\n");
    return 64;
  }
  const std::string dir = argv[1];
  struct stat st;
  if (::stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) {
    fprintf(stderr, "dbfiles_check: %s is not a directory\n", dir.c_str());
    return 66;
  }

  {  // a complete run: complete.kdb / complete.idx stay (the test compares them with the model's files)
    KuDbFiles f;
    const bool ok = write_run(f, dir + "/complete.kdb", dir + "/complete.idx", true) && f.finish(N_REC);
    report("complete", ok && exists(dir + "/complete.kdb") && exists(dir + "/complete.idx"), f.error);
  }
  {  // destroyed before finish
    bool ok;
    {
      KuDbFiles f;
      ok = write_run(f, dir + "/abandoned.kdb", dir + "/abandoned.idx", false) && exists(dir + "/abandoned.kdb") && exists(dir + "/abandoned.idx");
    }
    report("abandoned", ok && !exists(dir + "/abandoned.kdb") && !exists(dir + "/abandoned.idx"), "files left behind, or never there");
  }
  {  // the index path is a directory: open fails, the .kdb created a moment before is gone, the directory is not
    const std::string idx_dir = dir + "/is_a_directory.idx";
    ::mkdir(idx_dir.c_str(), 0755);
    KuDbFiles f;
    const bool opened = f.open(dir + "/blocked.kdb", idx_dir);
    const bool text = f.error == "can't write " + idx_dir;
    f.abandon();
    report("index_is_a_directory", !opened && text && !exists(dir + "/blocked.kdb") && exists(idx_dir), "opened, wrong text (" + f.error + "), or files wrong");
  }
  {  // a write fails (file size limit of a few hundred bytes): the append says so, finish does not succeed, nothing is left
    struct rlimit old_lim, lim;
    getrlimit(RLIMIT_FSIZE, &old_lim);
    lim = old_lim;
    lim.rlim_cur = 300;
    signal(SIGXFSZ, SIG_IGN);
    setrlimit(RLIMIT_FSIZE, &lim);
    std::vector<uint8_t> recs;
    std::vector<uint64_t> off;
    small_db(recs, off);
    const std::vector<uint8_t> hdr = ku_jflist_header(2);  // 112 bytes: the header of a list of 1-mers fits under the limit
    KuDbFiles f;
    const bool begun = f.open(dir + "/limited.kdb", dir + "/limited.idx") && f.begin(hdr.data(), hdr.size(), 2, NT);
    const bool first = f.append_records(recs.data(), recs.size());   // 112 + 156 bytes
    const bool second = f.append_records(recs.data(), recs.size());  // ... + 156 > 300
    const bool text = f.error == "write error on " + dir + "/limited.kdb";
    const bool finished = f.finish(2 * N_REC);
    setrlimit(RLIMIT_FSIZE, &old_lim);
    report("write_fails", begun && first && !second && text, "the write went through or an earlier one did not, or wrong text (" + f.error + ")");
    report("finish_after_failure", !finished && !exists(dir + "/limited.kdb") && !exists(dir + "/limited.idx"), "finish succeeded, or files left behind");
  }
  return n_failed ? 1 : 0;
}
