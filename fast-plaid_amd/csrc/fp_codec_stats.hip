// The device part of fp_residual_stats (include/fastplaid.h) that is not the assignment: the fp16 residuals of a chunk against
// its tokens' centroids, their exact per-dim magnitude sums, the tokens' residual norms, and the 65 536-bin histogram of the
// residuals' bit patterns the codec's quantiles are read from.  The codes are fp_index_ops.hip's (fpk_assign_codes).
//
// Nothing here depends on scheduling: the sums and the histogram are integers (64-bit atomics in global memory, 32- and 64-bit
// integer atomics in LDS), and a token's norm is ONE lane's ascending-d fp32 chain of exact fp16 x fp16 squares (mul + add == fma).
#include <algorithm>

#include "fp_internal.h"

#include "fp_device.h"

// ---- k_residual_tile -------------------------------------------------------------------------------------------------------------
// One workgroup of 256 walks tiles of RS_TOK tokens in K-slices of RS_KS dims (128 bytes per row).  The waves are specialised:
//   waves 1 .. 3 (192 producers): thread -> 16-byte unit (p & 7) of rows (p >> 3) + 24 k, k = 0 .. 2.  Eight consecutive lanes read
//     one row's whole 128-byte line of x and of the gathered centroid row, subtract with packed fp16 (one fp32 subtraction rounded
//     once: fp_selftest_arith out[1]), write r to the residual buffer (the same coalescing) and to the LDS tile, and add
//     |fixed(r)| of their (up to three) rows, summed in registers first, into the workgroup's per-dim int64 sums in LDS.
//   wave 0 (the chain): lane = token.  It walks the staged slice in ascending d with 16-byte LDS reads and carries each token's
//     fp32 chain across the slices in a register.
// Two LDS tiles and ONE barrier per slice: behind barrier s the chain reads tile s & 1 while the producers fill tile (s + 1) & 1;
// they reach tile s & 1 again only behind barrier s + 1, which the chain wave joins after it has finished slice s.
// Row pitch RS_PITCH = 144 bytes: the chain's 16-byte reads of 64 consecutive rows are conflict-free (fp_outliers.hip derives it).
// A dim that is not a multiple of 8 (legal up to 256) has rows that do not start on 16-byte boundaries: the producers then load
// and store the unit's elements one by one -- a branch that is uniform over the launch; everything behind the load is shared.
// Tokens past T and dims past D are masked: never loaded, stored as zeros in LDS (a zero adds nothing to a sum or a chain), and
// never written to the residual buffer.  The LDS sums live across all the tiles of a workgroup and leave with one 64-bit global
// atomic per dim at the end.
#define RS_TOK 64
#define RS_KS 64
#define RS_PITCH 144
#define RS_MAX_DIM 1024
#define RS_PROD 192   // producer threads
#define RS_ROWS 3     // rows a producer owns per slice: (p >> 3) + 24 k

__device__ __forceinline__ uint32_t rs_sub2(uint32_t a, uint32_t b) { return h2_as_u32(u32_as_h2(a) - u32_as_h2(b)); }
__device__ __forceinline__ int64_t rs_abs_fixed(uint32_t h) { return fp_f16_fixed((uint16_t)(h & 0x7FFFu)); }

__global__ __launch_bounds__(256) void k_residual_tile(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent, int64_t C,
                                                       int D, const int32_t* __restrict__ codes, uint16_t* __restrict__ res,
                                                       unsigned long long* __restrict__ abs_sum, float* __restrict__ norms /*nullable*/,
                                                       int64_t* __restrict__ codes64 /*nullable*/) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[2][RS_TOK * RS_PITCH];
  __shared__ unsigned long long asum[RS_MAX_DIM];
  __shared__ int32_t lab[RS_TOK];   // the tile's codes, -1: no such token
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool vec = (D & 7) == 0;
  const int nslice = (D + RS_KS - 1) / RS_KS;
  const int64_t ntile = (T + RS_TOK - 1) / RS_TOK;
  for (int d = tid; d < D; d += 256) asum[d] = 0ull;
  for (int64_t ti = blockIdx.x; ti < ntile; ti += gridDim.x) {   // uniform over the workgroup
    const int64_t t0 = ti * RS_TOK;
    if (wave == 0) {
      const int64_t t = t0 + lane;
      int32_t c = -1;
      if (t < T) {
        c = codes[t];
        if (c < 0 || (int64_t)c >= C) c = 0;   // never, behind the assignment: no row outside the table is read whatever comes
        if (codes64) codes64[t] = c;
      }
      lab[lane] = c;
    }
    __syncthreads();   // lab[] (and, before the first tile, the zeroed sums); the chain of the tile before is finished
    float chain = 0.f;
    for (int s = 0; s < nslice; ++s) {
      unsigned char* buf = tile[s & 1];
      if (wave != 0) {
        const int p = tid - 64, unit = p & 7, r0 = p >> 3;
        const int d = s * RS_KS + 8 * unit;
        uint32_t xw[RS_ROWS][4], yw[RS_ROWS][4];
#pragma unroll
        for (int k = 0; k < RS_ROWS; ++k) {
          const int row = r0 + 24 * k;
          const int32_t c = row < RS_TOK ? lab[row] : -1;
#pragma unroll
          for (int j = 0; j < 4; ++j) xw[k][j] = yw[k][j] = 0u;
          if (c >= 0 && d < D) {
            const uint16_t* __restrict__ x = emb + (t0 + row) * D + d;
            const uint16_t* __restrict__ y = cent + (int64_t)c * D + d;
            if (vec) {
              const uint4 xv = *reinterpret_cast<const uint4*>(x), yv = *reinterpret_cast<const uint4*>(y);
              xw[k][0] = xv.x, xw[k][1] = xv.y, xw[k][2] = xv.z, xw[k][3] = xv.w;
              yw[k][0] = yv.x, yw[k][1] = yv.y, yw[k][2] = yv.z, yw[k][3] = yv.w;
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (d + j < D) {
                  xw[k][j >> 1] |= (uint32_t)x[j] << (16 * (j & 1));
                  yw[k][j >> 1] |= (uint32_t)y[j] << (16 * (j & 1));
                }
            }
          }
        }
        int64_t mag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < RS_ROWS; ++k) {
          const int row = r0 + 24 * k;
          if (row >= RS_TOK) continue;
          uint32_t rw[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            rw[j] = rs_sub2(xw[k][j], yw[k][j]);   // a masked element: +0 - +0 = +0
            mag[2 * j] += rs_abs_fixed(rw[j]);
            mag[2 * j + 1] += rs_abs_fixed(rw[j] >> 16);
          }
          *reinterpret_cast<uint4*>(buf + row * RS_PITCH + 16 * unit) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
          if (lab[row] >= 0 && d < D) {
            uint16_t* __restrict__ o = res + (t0 + row) * D + d;
            if (vec) {
              *reinterpret_cast<uint4*>(o) = make_uint4(rw[0], rw[1], rw[2], rw[3]);
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (d + j < D) o[j] = (uint16_t)(rw[j >> 1] >> (16 * (j & 1)));
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (d + j < D && mag[j]) atomicAdd(&asum[d + j], (unsigned long long)mag[j]);
      }
      __syncthreads();
      if (wave == 0 && norms) {
        const int nu = (min(RS_KS, D - s * RS_KS) + 7) >> 3;   // the chain stops at D (the last unit's tail holds zeros)
        for (int u = 0; u < nu; ++u) {
          const uint4 v = *reinterpret_cast<const uint4*>(buf + lane * RS_PITCH + 16 * u);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float f0 = (float)__builtin_bit_cast(half_t, (uint16_t)(w[j] & 0xFFFFu));
            const float f1 = (float)__builtin_bit_cast(half_t, (uint16_t)(w[j] >> 16));
            chain += f0 * f0;
            chain += f1 * f1;
          }
        }
      }
    }
    if (wave == 0 && norms && t0 + lane < T) norms[t0 + lane] = __builtin_sqrtf(chain);
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256)
    if (asum[d]) atomicAdd(&abs_sum[d], asum[d]);
}

void fpk_residual_tile(const uint16_t* emb, int64_t T, const uint16_t* cent, int64_t C, int D, const int32_t* codes, uint16_t* res,
                       int64_t* abs_sum, float* norms, int64_t* codes64, hipStream_t st) {
  if (T <= 0 || D < 1 || D > RS_MAX_DIM) return;
  // a few tiles per workgroup: the LDS sums leave once per workgroup, not once per tile
  const unsigned blocks = fp_grid_cap(std::min<int64_t>((T + RS_TOK - 1) / RS_TOK, 2048), 256);
  hipLaunchKernelGGL(k_residual_tile, dim3(blocks), dim3(256), 0, st, emb, T, cent, C, D, codes, res,
                     reinterpret_cast<unsigned long long*>(abs_sum), norms, codes64);
}

// ---- k_hist16 ----------------------------------------------------------------------------------------------------------------------
// hist[b] += #{ i : vals[i] == b } for the n fp16 bit patterns of a residual buffer.  A workgroup keeps the 32 768 bins of ONE sign
// (blockIdx.y) as uint32 in 128 KB of LDS and reads the whole buffer, 16 bytes per thread and step: reading it twice is the price
// of bins that never leave LDS until the end, when the non-zero ones go out with 64-bit global atomics.  n <= 2^30 per launch, so
// a bin cannot wrap.  The n & 7 values behind the last whole unit are read one by one.
#define H16_BINS 32768
#define H16_THREADS 1024
__device__ __forceinline__ void h16_add2(uint32_t* bins, uint32_t w, uint32_t sign) {
  if (((w >> 15) & 1u) == sign) atomicAdd(&bins[w & 0x7FFFu], 1u);
  if ((w >> 31) == sign) atomicAdd(&bins[(w >> 16) & 0x7FFFu], 1u);
}
__global__ __launch_bounds__(H16_THREADS) void k_hist16(const uint16_t* __restrict__ vals, int64_t n, unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t h16_bins[];
  const uint32_t sign = blockIdx.y;
  for (int i = threadIdx.x; i < H16_BINS; i += H16_THREADS) h16_bins[i] = 0u;
  __syncthreads();
  const int64_t nu = n >> 3;
  const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(vals);
  for (int64_t u = (int64_t)blockIdx.x * H16_THREADS + threadIdx.x; u < nu; u += (int64_t)gridDim.x * H16_THREADS) {
    const uint4 v = v4[u];
    h16_add2(h16_bins, v.x, sign);
    h16_add2(h16_bins, v.y, sign);
    h16_add2(h16_bins, v.z, sign);
    h16_add2(h16_bins, v.w, sign);
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 7)) {
    const uint32_t h = vals[nu * 8 + threadIdx.x];
    if ((h >> 15) == sign) atomicAdd(&h16_bins[h & 0x7FFFu], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H16_BINS; i += H16_THREADS) {
    const uint32_t c = h16_bins[i];
    if (c) atomicAdd(&hist[(sign << 15) | (uint32_t)i], (unsigned long long)c);
  }
}

int fpk_hist16(const uint16_t* vals, int64_t n, int64_t* hist, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > (1ll << 30)) return -2;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -3;
  const int64_t tiles = ((n >> 3) + H16_THREADS - 1) / H16_THREADS;   // steps of one workgroup over the whole buffer
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cus, tiles));
  static std::atomic<uint64_t> ok{0};
  fp_allow_big_lds((const void*)k_hist16, ok, H16_BINS * 4);
  hipLaunchKernelGGL(k_hist16, dim3(gx, 2), dim3(H16_THREADS), H16_BINS * 4, st, vals, n, reinterpret_cast<unsigned long long*>(hist));
  return 0;
}
