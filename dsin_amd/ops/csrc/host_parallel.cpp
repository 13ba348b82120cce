// at::parallel_for for the host code that lives in the .hip sources. The
// HIP compiler's host pass is built without OpenMP, where ATen's
// parallel_for template degrades to a serial loop; this file is compiled by
// the host C++ compiler with -fopenmp (setup.py), so the loop really runs on
// ATen's intra-op threads.

#include <cstdint>
#include <functional>

#include <ATen/Parallel.h>

#if !defined(_OPENMP)
#error "host_parallel.cpp must be compiled with -fopenmp (see setup.py)"
#endif

namespace dsin {

void host_parallel_for(int64_t begin, int64_t end, int64_t grain,
                       const std::function<void(int64_t, int64_t)>& f) {
  at::parallel_for(begin, end, grain, f);
}

}  // namespace dsin
