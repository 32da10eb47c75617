// Host-side check of k_ivf_mark's index arithmetic (fp_internal.h: fp_ivf_nvec / fp_ivf_vec / fp_ivf_r0 / fp_ivf_keep and
// fp_ivf_lower_bound) against the scalar definitions.  No GPU: the helpers are __host__ __device__, this program runs them on the CPU.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I fast-plaid_amd/csrc \
//         tools/probe/ivf_vec_check.hip -o tools/probe/ivf_vec_check.out && tools/probe/ivf_vec_check.out
// 1. every range [lo, hi) with lo, hi in 0 .. 40: the vectors the walk loads are exactly those of the issue's definition (first at
//    lo & ~3, ((hi + 3) >> 2) - (lo >> 2) of them, none for hi <= lo), each entry of [lo, hi) is kept exactly once, nothing else is.
// 2. ascending lists of 0 .. 200 entries (all lengths to 40) at every start 0 .. 7 inside an array
//    padded by THREE entries (the sanitizer catches a load beyond them), every target: fp_ivf_lower_bound == std::lower_bound.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fp_internal.h"

int main() {
  long long checked = 0;
  for (long long lo = 0; lo <= 40; ++lo)
    for (long long hi = 0; hi <= 40; ++hi) {
      const uint32_t len = hi > lo ? (uint32_t)(hi - lo) : 0u;
      const uint32_t nv = fp_ivf_nvec(lo, len);
      const uint32_t want = hi > lo ? (uint32_t)(((hi + 3) >> 2) - (lo >> 2)) : 0u;
      if (nv != want) { printf("nvec lo %lld hi %lld: %u != %u\n", lo, hi, nv, want); return 1; }
      std::vector<int> seen(48, 0);
      for (uint32_t i = 0; i < nv; ++i) {
        const long long vi = fp_ivf_vec(lo, i);
        if (vi != (lo >> 2) + i || vi * 4 + 3 > ((hi + 3) & ~3ll) - 1) { printf("vector lo %lld hi %lld i %u: %lld\n", lo, hi, i, vi); return 1; }
        const int r0 = fp_ivf_r0(lo, i);
        for (int e = 0; e < 4; ++e)
          if (fp_ivf_keep(r0, e, len)) ++seen[vi * 4 + e];
      }
      for (long long x = 0; x < 48; ++x)
        if (seen[x] != (x >= lo && x < hi ? 1 : 0)) { printf("keep lo %lld hi %lld entry %lld: %d\n", lo, hi, x, seen[x]); return 1; }
      ++checked;
    }
  long long searches = 0;
  for (int n = 0; n <= 200; n += (n < 40 ? 1 : 23))
    for (int start = 0; start < 8; ++start)
      for (int step = 1; step <= 3; ++step) {
        int32_t* a = new int32_t[start + n + 3];   // (exactly the three entries of padding the kernel relies on)
        for (int i = 0; i < start + n + 3; ++i) a[i] = 1000000;   // before and behind the list: what a neighbouring list may hold
        for (int i = 0; i < n; ++i) a[start + i] = 10 + i * step;
        for (int32_t t = 0; t <= 10 + n * step + 2; ++t) {
          const long long got = fp_ivf_lower_bound(a, start, start + n, t);
          const long long ref = std::lower_bound(a + start, a + start + n, t) - a;
          if (got != ref) { printf("search n %d start %d step %d target %d: %lld != %lld\n", n, start, step, t, got, ref); return 1; }
          ++searches;
        }
        delete[] a;
      }
  printf("ivf_vec_check OK: %lld ranges, %lld searches\n", checked, searches);
  return 0;
}
