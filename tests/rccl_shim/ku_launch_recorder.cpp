// Launch recorder (test infrastructure, never shipped): an LD_PRELOAD library that defines hipLaunchKernel, notes the name of
// every kernel launched through it and forwards the call to the HIP runtime's own hipLaunchKernel.  The kernel handle of a
// launch is the address of the kernel's host stub; the product library exports those stubs, so dladdr names them
// (ku_classify_short_kernel<2, true, 31, 15, false, 2, false> and so on, demangled here).  Used only in a child process that a
// test starts (tests/test_gpu_instances.py); the list is read and cleared through ku_rec_* from Python.
#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace {
std::mutex g_mu;
std::vector<std::string> g_names;
uint64_t g_total = 0;  // launches seen since the library was loaded (never cleared: proof that interposition works)
using launch_fn = hipError_t (*)(const void *, dim3, dim3, void **, size_t, hipStream_t);

// the HIP runtime's own entry point: the next definition in the global scope, or -- the usual case under PyTorch, which loads
// the runtime with RTLD_LOCAL -- the runtime the process has already loaded, found by its soname
launch_fn find_real_launch() {
  void *p = dlvsym(RTLD_NEXT, "hipLaunchKernel", "hip_4.2");
  if (!p) p = dlsym(RTLD_NEXT, "hipLaunchKernel");
  for (const char *so : {"libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"}) {
    if (p) break;
    if (void *h = dlopen(so, RTLD_LAZY | RTLD_NOLOAD)) {
      p = dlvsym(h, "hipLaunchKernel", "hip_4.2");
      if (!p) p = dlsym(h, "hipLaunchKernel");
    }
  }
  return reinterpret_cast<launch_fn>(p);
}
launch_fn real_launch() {
  static launch_fn fn = nullptr;
  if (!fn) fn = find_real_launch();  // (not cached while the runtime is not loaded yet)
  return fn;
}

std::string kernel_name(const void *f) {
  Dl_info info{};
  if (!dladdr(f, &info) || !info.dli_sname) return "?";
  int status = 0;
  char *d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
  std::string s = (status == 0 && d) ? d : info.dli_sname;
  std::free(d);
  if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);  // return type of a template function's demangled name
  const size_t paren = s.rfind('(');
  if (paren != std::string::npos && paren > 0) s.erase(paren);
  return s;
}
}  // namespace

extern "C" {
hipError_t hipLaunchKernel(const void *function_address, dim3 num_blocks, dim3 dim_blocks, void **args, size_t shared_mem_bytes,
                           hipStream_t stream) {
  launch_fn fn = real_launch();
  if (!fn) return hipErrorNotFound;
  {
    std::string name = kernel_name(function_address);
    std::lock_guard<std::mutex> lk(g_mu);
    g_names.push_back(std::move(name));
    ++g_total;
  }
  return fn(function_address, num_blocks, dim_blocks, args, shared_mem_bytes, stream);
}

uint64_t ku_rec_total() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_total;
}
uint64_t ku_rec_count() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_names.size();
}
// name of launch i (NUL-terminated, cut at cap - 1 bytes); returns its full length, 0 past the end
uint64_t ku_rec_get(uint64_t i, char *out, uint64_t cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (i >= g_names.size() || cap == 0) return 0;
  const std::string &s = g_names[i];
  const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
  std::memcpy(out, s.data(), n);
  out[n] = 0;
  return s.size();
}
void ku_rec_clear() {
  std::lock_guard<std::mutex> lk(g_mu);
  g_names.clear();
}
}
