// The device part of fp_centroid_outliers (include/fastplaid.h) that is not the assignment: half square norms of the centroids,
// the squared distance of every token to its nearest centroid with the threshold flag, and the ordered compaction of the flagged
// rows (per-tile counts -> scan -> write).  The labels are fp_index_ops.hip's (fpk_assign_l2_narrow / fpk_assign_l2_exact).
//
// Every sum is an ascending-d fp32 chain of exact fp16 x fp16 products (mul + add == fma), the compaction's order is the row
// order whatever the scheduling, and there is no float atomic: the two maxima are combined as fp32 BITS of values >= 0.
#include <algorithm>

#include "fp_internal.h"

#include "fp_device.h"

#define OUT_TILE 256   // tokens per compaction tile = threads per workgroup

// hn[c] = 0.5f * chain of cent[c][d]^2 (k_km_finalise's definition), stat = {max|cent|, max hn} as fp32 bits (k_assign_thr_l2's input)
__global__ __launch_bounds__(256) void k_out_prepare(const uint16_t* __restrict__ cent, int64_t C, int D, float* __restrict__ half_sqnorm,
                                                     uint32_t* __restrict__ stat) {
  for (int64_t base = (int64_t)blockIdx.x * 256; base < C; base += (int64_t)gridDim.x * 256) {   // uniform over the workgroup
    const int64_t c = base + threadIdx.x;
    float amax = 0.f, hn = 0.f;
    if (c < C) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) {
        const float v = (float)__builtin_bit_cast(half_t, cent[c * D + d]);
        acc += v * v;
        amax = fmaxf(amax, __builtin_fabsf(v));
      }
      hn = 0.5f * acc;
      half_sqnorm[c] = hn;
    }
    uint32_t a = __float_as_uint(amax), b = __float_as_uint(hn);   // both >= 0: bit order = value order
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      a = max(a, shfl_xor_u32(a, s));
      b = max(b, shfl_xor_u32(b, s));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMax(&stat[0], a);
      atomicMax(&stat[1], b);
    }
  }
}
void fpk_out_prepare(const uint16_t* cent, int64_t C, int D, float* half_sqnorm, uint32_t* stat, hipStream_t st) {
  (void)hipMemsetAsync(stat, 0, 8, st);
  hipLaunchKernelGGL(k_out_prepare, dim3(fp_grid_cap((C + 255) / 256, 256)), dim3(256), 0, st, cent, C, D, half_sqnorm, stat);
}

// One thread per token, one tile of OUT_TILE consecutive tokens per workgroup round:
//   s = fl32(chain(x_t . cent_c) - hn[c]), c = labels[t];  sqdist[t] = fl32(chain(x_t^2) - 2 s);  flag[t] = sqdist[t] > thr
// (2 s is exact, so the last line rounds once however it is contracted).  tilecnt[tile] = the tile's flagged tokens.
__global__ __launch_bounds__(OUT_TILE) void k_outlier_dist(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent,
                                                           int64_t C, int D, const float* __restrict__ half_sqnorm,
                                                           const int32_t* __restrict__ labels, float thr, float* __restrict__ sqdist,
                                                           int64_t* __restrict__ nearest /*nullable*/, uint8_t* __restrict__ flag,
                                                           int32_t* __restrict__ tilecnt) {
  __shared__ int32_t wcnt[OUT_TILE / 64];
  const int64_t ntile = (T + OUT_TILE - 1) / OUT_TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {   // uniform over the workgroup
    const int64_t t = tile * OUT_TILE + threadIdx.x;
    bool out = false;
    if (t < T) {
      const int32_t c = labels[t];
      float sd = __uint_as_float(0x7FC00000u);
      if (c >= 0 && (int64_t)c < C) {   // always, once an overflowed chunk has been through the exact kernel
        const uint16_t* __restrict__ x = emb + t * D;
        const uint16_t* __restrict__ y = cent + (int64_t)c * D;
        float dot = 0.f, x2 = 0.f;
        if ((D & 7) == 0) {   // rows of 16-byte vectors; the chain order is the same
          for (int d = 0; d < D; d += 8) {
            const uint4 xv = *reinterpret_cast<const uint4*>(x + d), yv = *reinterpret_cast<const uint4*>(y + d);
            const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w}, yw[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float x0 = (float)__builtin_bit_cast(half_t, (uint16_t)(xw[j] & 0xFFFFu));
              const float x1 = (float)__builtin_bit_cast(half_t, (uint16_t)(xw[j] >> 16));
              const float y0 = (float)__builtin_bit_cast(half_t, (uint16_t)(yw[j] & 0xFFFFu));
              const float y1 = (float)__builtin_bit_cast(half_t, (uint16_t)(yw[j] >> 16));
              dot += x0 * y0;
              x2 += x0 * x0;
              dot += x1 * y1;
              x2 += x1 * x1;
            }
          }
        } else {
          for (int d = 0; d < D; ++d) {
            const float xf = (float)__builtin_bit_cast(half_t, x[d]), yf = (float)__builtin_bit_cast(half_t, y[d]);
            dot += xf * yf;
            x2 += xf * xf;
          }
        }
        const float s = dot - half_sqnorm[c];
        sd = x2 - 2.0f * s;
      }
      sqdist[t] = sd;
      if (nearest) nearest[t] = c;
      out = sd > thr;
      flag[t] = out ? 1 : 0;
    }
    const unsigned long long b = __ballot(out);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (int32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
      int32_t n = 0;
#pragma unroll
      for (int w = 0; w < OUT_TILE / 64; ++w) n += wcnt[w];
      tilecnt[tile] = n;
    }
    __syncthreads();   // wcnt[] is rewritten by the next round
  }
}

// exclusive scan of the tile counts by ONE workgroup of 1024 (a chunk of 2^20 tokens has 4096 tiles: 4 rounds); *count = the total
__global__ __launch_bounds__(1024) void k_out_scan(const int32_t* __restrict__ tilecnt, int64_t ntile, int32_t* __restrict__ tileoff,
                                                   int32_t* __restrict__ count) {
  __shared__ int32_t wt[16];
  int32_t carry = 0;
  for (int64_t base = 0; base < ntile; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int32_t v = i < ntile ? tilecnt[i] : 0;
    int32_t total;
    const int32_t incl = fp_block_scan_incl<int32_t>(v, wt, &total);
    if (i < ntile) tileoff[i] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

// rows[tileoff[tile] + rank inside the tile] = row0 + t for every flagged token: ascending, and < *count <= T entries are written
__global__ __launch_bounds__(OUT_TILE) void k_out_write(const uint8_t* __restrict__ flag, int64_t T, int64_t row0,
                                                        const int32_t* __restrict__ tileoff, int64_t* __restrict__ rows) {
  __shared__ int32_t wt[OUT_TILE / 64];
  const int64_t ntile = (T + OUT_TILE - 1) / OUT_TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {   // uniform over the workgroup
    const int64_t t = tile * OUT_TILE + threadIdx.x;
    const int32_t v = (t < T && flag[t]) ? 1 : 0;
    const int32_t incl = fp_block_scan_incl<int32_t>(v, wt);
    if (v) rows[(int64_t)tileoff[tile] + incl - 1] = row0 + t;
  }
}

size_t fpk_outliers_tiles(int64_t T) { return (size_t)((T + OUT_TILE - 1) / OUT_TILE); }

void fpk_outliers_chunk(const uint16_t* emb, int64_t T, int64_t row0, const uint16_t* cent, int64_t C, int D, const float* half_sqnorm,
                        const int32_t* labels, float thr, float* sqdist, int64_t* nearest, uint8_t* flag, int32_t* tilecnt, int32_t* tileoff,
                        int32_t* count, int64_t* rows, hipStream_t st) {
  if (T <= 0) return;
  const int64_t ntile = (int64_t)fpk_outliers_tiles(T);
  const unsigned blocks = fp_grid_cap(ntile, OUT_TILE);
  hipLaunchKernelGGL(k_outlier_dist, dim3(blocks), dim3(OUT_TILE), 0, st, emb, T, cent, C, D, half_sqnorm, labels, thr, sqdist, nearest, flag,
                     tilecnt);
  hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, st, tilecnt, ntile, tileoff, count);
  hipLaunchKernelGGL(k_out_write, dim3(blocks), dim3(OUT_TILE), 0, st, flag, T, row0, tileoff, rows);
}
