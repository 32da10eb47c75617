// The Lloyd update of fp_kmeans (include/fastplaid.h) on the device: data check, inverted index of the labels (count -> scan ->
// fill), exact per-cluster sums, and the finalise kernel (mean / reseed / cent16 / half square norms).  The assignment itself is
// fp_index_ops.hip's (fpk_assign_l2_narrow / fpk_assign_l2_exact).
//
// Exactness: every finite fp16 value is an integer multiple of 2^-24 (fp_f16_fixed), so a cluster's sum is an INTEGER sum --
// the same whatever the order of the additions, which is what makes the centroids reproducible from run to run and comparable
// bit for bit with the numpy model.  The caller has checked n * max|x| * 2^24 < 2^62: no partial sum leaves int64.  The partial
// sums of a list are combined with 64-bit INTEGER atomics (order-free); there is no float atomic anywhere.
#include <algorithm>

#include "fp_internal.h"

#include "fp_device.h"

// ---- data check ------------------------------------------------------------------------------------------------------------
// max over the data of |x| as fp16 bits (monotone in |x|; >= 0x7C00: inf or NaN).  Pairs of values per 32-bit load.
__global__ __launch_bounds__(256) void k_km_scan_data(const uint16_t* __restrict__ data, int64_t n_elems, uint32_t* __restrict__ stat) {
  const uint32_t* d32 = reinterpret_cast<const uint32_t*>(data);
  const int64_t n2 = n_elems >> 1;
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t v = d32[i];
    m = max(m, max(v & 0x7FFFu, (v >> 16) & 0x7FFFu));
  }
  if ((n_elems & 1) && blockIdx.x == 0 && threadIdx.x == 0) m = max(m, (uint32_t)(data[n_elems - 1] & 0x7FFF));
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m = max(m, shfl_xor_u32(m, s));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(stat, m);
}
void fpk_km_scan_data(const uint16_t* data, int64_t n_elems, uint32_t* stat, hipStream_t st) {
  if (n_elems <= 0) return;
  hipLaunchKernelGGL(k_km_scan_data, dim3(fp_grid_cap(std::min<int64_t>((n_elems / 2 + 255) / 256, 8192), 256)), dim3(256), 0, st, data, n_elems,
                     stat);
}

// ---- finalise --------------------------------------------------------------------------------------------------------------
// One wave per cluster, 4 clusters per workgroup.  Steps 1, 2, 5, 6 of the specification:
//   sums == nullptr  cent32[c] = (float)data[init_rows[c]]
//   cnt[c] > 0       cent32[c][d] = (float)(((double)S * 2^-24) / (double)cnt[c])   (S the int64 sum; every step round-to-nearest-even)
//   cnt[c] == 0      cent32[c] = (float)data[mix64(stream_key(seed, 0x6B6D0000 + it) + c) % n]
// then cent16 = RNE16(cent32) and hn[c] = 0.5f * the ascending-d fp32 chain of cent16[c][d]^2 (one lane walks it; a square of an
// fp16 value is exact in fp32, so mul + add == fma).  stat = {max|cent16|, max hn} as fp32 bits (both >= 0: bit order = value order).
#define KM_RESEED_STREAM 0x6B6D0000ull
__global__ __launch_bounds__(256) void k_km_finalise(const uint16_t* __restrict__ data, int64_t n, int D, int64_t K,
                                                     const int64_t* __restrict__ init_rows, const int64_t* __restrict__ sums,
                                                     const int32_t* __restrict__ cnt, uint64_t seed, int it, float* __restrict__ cent32,
                                                     uint16_t* __restrict__ cent16, float* __restrict__ half_sqnorm, uint32_t* __restrict__ stat) {
  __shared__ float row[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < K; base += (int64_t)gridDim.x * 4) {   // uniform over the workgroup
    const int64_t c = base + wave;
    float amax = 0.f;
    if (c < K) {
      int64_t src = -1;
      int32_t m = 0;
      if (!sums) {
        src = init_rows[c];
      } else {
        m = cnt[c];
        if (m <= 0) src = (int64_t)(mix64(stream_key(seed, KM_RESEED_STREAM + (uint64_t)it) + (uint64_t)c) % (uint64_t)n);
      }
      for (int d = lane; d < D; d += 64) {
        float v;
        if (src >= 0)
          v = (float)__builtin_bit_cast(half_t, data[src * D + d]);
        else
          v = (float)(((double)sums[c * D + d] * 5.9604644775390625e-08) / (double)m);
        const half_t h = (half_t)v;
        cent32[c * D + d] = v;
        cent16[c * D + d] = __builtin_bit_cast(uint16_t, h);
        row[wave][d] = (float)h;
        amax = fmaxf(amax, __builtin_fabsf((float)h));
      }
    }
    __syncthreads();
    if (c < K) {
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) amax = fmaxf(amax, __shfl_xor(amax, s, 64));
      if (lane == 0) {
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += row[wave][d] * row[wave][d];
        const float hn = 0.5f * acc;
        half_sqnorm[c] = hn;
        atomicMax(&stat[0], __float_as_uint(amax));
        atomicMax(&stat[1], __float_as_uint(hn));
      }
    }
    __syncthreads();   // row[] is rewritten by the next round
  }
}
void fpk_km_finalise(const uint16_t* data, int64_t n, int D, int64_t K, const int64_t* init_rows, const int64_t* sums, const int32_t* cnt,
                     uint64_t seed, int it, float* cent32, uint16_t* cent16, float* half_sqnorm, uint32_t* stat, hipStream_t st) {
  (void)hipMemsetAsync(stat, 0, 8, st);
  hipLaunchKernelGGL(k_km_finalise, dim3(fp_grid_cap((K + 3) / 4, 256)), dim3(256), 0, st, data, n, D, K, init_rows, sums, cnt, seed, it, cent32,
                     cent16, half_sqnorm, stat);
}

// ---- inverted index of the labels ---------------------------------------------------------------------------------------------
// (every label is a centroid index: the assignment kernels write nothing else once the overflowed chunks have been redone)
__global__ __launch_bounds__(256) void k_km_count(const int32_t* __restrict__ labels, int64_t n, int32_t* __restrict__ cnt) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    atomicAdd(&cnt[labels[t]], 1);
  }
}
// exclusive scan of cnt by ONE workgroup of 1024 (K is a centroid count: 2^17 is 128 rounds): cursor[c] = where list c starts
__global__ __launch_bounds__(1024) void k_km_scan(const int32_t* __restrict__ cnt, int64_t K, int32_t* __restrict__ cursor) {
  __shared__ int32_t wt[16];
  int32_t carry = 0;
  for (int64_t base = 0; base < K; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int32_t v = i < K ? cnt[i] : 0;
    int32_t total;
    const int32_t incl = fp_block_scan_incl<int32_t>(v, wt, &total);
    if (i < K) cursor[i] = carry + incl - v;
    carry += total;
  }
}
__global__ __launch_bounds__(256) void k_km_fill(const int32_t* __restrict__ labels, int64_t n, int32_t* __restrict__ cursor,
                                                 int32_t* __restrict__ members) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    members[atomicAdd(&cursor[labels[t]], 1)] = (int32_t)t;
  }
}
void fpk_km_index(const int32_t* labels, int64_t n, int64_t K, int32_t* cnt, int32_t* cursor, int32_t* members, hipStream_t st) {
  (void)hipMemsetAsync(cnt, 0, (size_t)K * 4, st);
  const unsigned blocks = fp_grid_cap((n + 255) / 256, 256);
  hipLaunchKernelGGL(k_km_count, dim3(blocks), dim3(256), 0, st, labels, n, cnt);
  hipLaunchKernelGGL(k_km_scan, dim3(1), dim3(1024), 0, st, cnt, K, cursor);
  hipLaunchKernelGGL(k_km_fill, dim3(blocks), dim3(256), 0, st, labels, n, cursor, members);
}

// ---- exact per-cluster sums ---------------------------------------------------------------------------------------------------
// The member array is the clusters' lists back to back.  One wave takes a slice of KM_SLICE consecutive entries -- so a list of any
// length is shared by as many waves as it has slices, and a run of tiny lists by one -- reads each member's whole row (2 * D
// contiguous bytes; lane l holds dims l, l + 64, ..), accumulates in int64 registers while the cluster stays the same and adds
// the partial sum to sums[c] when it changes: at most (n / KM_SLICE + K) * D integer atomics in all.
#define KM_SLICE 128
__global__ __launch_bounds__(256) void k_km_sum(const uint16_t* __restrict__ data, int D, const int32_t* __restrict__ labels,
                                                const int32_t* __restrict__ members, int64_t total,
                                                unsigned long long* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t nslice = (total + KM_SLICE - 1) / KM_SLICE;
  bool live[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) live[j] = lane + 64 * j < D;
  for (int64_t sl = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); sl < nslice; sl += (int64_t)gridDim.x * 4) {
    const int64_t p0 = sl * KM_SLICE;
    const int cntp = total - p0 < KM_SLICE ? (int)(total - p0) : KM_SLICE;
    // the slice's members and their clusters, two per lane, handed round by lane shuffles
    int32_t mt[2], mc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = h * 64 + lane;
      mt[h] = q < cntp ? members[p0 + q] : 0;
      mc[h] = q < cntp ? labels[mt[h]] : -1;
    }
    long long acc[4] = {0, 0, 0, 0};
    int32_t cur = -1;
    auto flush = [&]() {
      if (cur >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (live[j] && acc[j] != 0) atomicAdd(&sums[(int64_t)cur * D + lane + 64 * j], (unsigned long long)acc[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = 0;
    };
    for (int i0 = 0; i0 < cntp; i0 += 4) {
      int32_t c[4];
      uint16_t x[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u;   // < KM_SLICE: cntp <= KM_SLICE and i0 is a multiple of 4
        const int32_t tt = __shfl(i < 64 ? mt[0] : mt[1], i & 63, 64);
        const int32_t cc = __shfl(i < 64 ? mc[0] : mc[1], i & 63, 64);
        c[u] = i < cntp ? cc : -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[u][j] = (c[u] >= 0 && live[j]) ? data[(int64_t)tt * D + lane + 64 * j] : (uint16_t)0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c[u] < 0) continue;
        if (c[u] != cur) {
          flush();
          cur = c[u];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += fp_f16_fixed(x[u][j]);
      }
    }
    flush();
  }
}
void fpk_km_sum(const uint16_t* data, int64_t n, int D, int64_t K, const int32_t* labels, const int32_t* members, int64_t* sums,
                hipStream_t st) {
  (void)hipMemsetAsync(sums, 0, (size_t)K * D * 8, st);
  const int64_t nslice = (n + KM_SLICE - 1) / KM_SLICE;
  hipLaunchKernelGGL(k_km_sum, dim3(fp_grid_cap((nslice + 3) / 4, 256)), dim3(256), 0, st, data, D, labels, members, n,
                     reinterpret_cast<unsigned long long*>(sums));
}

__global__ void k_km_widen_counts(const int32_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[i];
}
void fpk_km_widen_counts(const int32_t* cnt, int64_t* out, int64_t K, hipStream_t st) {
  hipLaunchKernelGGL(k_km_widen_counts, dim3(fp_grid_cap((K + 255) / 256, 256)), dim3(256), 0, st, cnt, out, K);
}
