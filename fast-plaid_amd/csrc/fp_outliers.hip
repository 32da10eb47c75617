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

// ---- chains through LDS (dims above 256) ---------------------------------------------------------------------------------------
// A chain's order is the arithmetic contract, so one thread walks one row; what a workgroup can share is the LOADS.  With one
// thread per row reading global memory, the lanes of a wave sit a whole row apart (2 KB at dim 1024): every load instruction
// touches 64 cache lines.  The sliced kernels below walk a tile of OUT_TILE rows in K-slices of OUT_KS dims (128 bytes per row):
// the workgroup stages the slice of every row into LDS with 16-byte loads, eight consecutive lanes reading one row's whole
// 128-byte line, then thread i walks row i's slice from LDS in ascending d, its fp32 accumulators kept in registers across slices.
//
// LDS row pitch OUT_PITCH = 144 bytes (128 + one 16-byte unit) = 36 banks of 4 bytes.  The chain reads unit u of row i with one
// 16-byte LDS read at 144 i + 16 u: over consecutive lanes the first bank is 36 i = 4 (9 i), and 9 is odd, so any 2^k consecutive
// lanes start at 2^k different multiples of 4 modulo 4 * 2^k -- the 16 lanes a 16-byte read serves per pass cover the 64 banks once
// each (the same holds for 8 lanes over 32 banks): no conflict.  The staging stores are not free of them: the two rows a pass
// of 16 lanes writes lie 36 banks apart, so the second row's last unit wraps onto the first row's first (one unit in sixteen
// waits); a pitch that frees the stores (128 mod 256) would make the reads 8-way.  Single-buffered: two workgroups per CU fit
// (73 728 B for two staged arrays) and fill each other's staging gaps.
#define OUT_KS 64                 // dims per K-slice
#define OUT_PITCH 144             // bytes per staged row slice
#define OUT_STAGE_BYTES (OUT_TILE * OUT_PITCH)

// Stages dims [d0, d0 + OUT_KS) of OUT_TILE rows: src(r) is row r's first element, or nullptr for a row that does not exist.
// Thread -> unit (tid & 7) of rows (tid >> 3) + 32 k, k = 0 .. 7; the eight loads are issued before the first LDS store.  Units at
// or past D (a short last slice) and absent rows are stored as zeros and never loaded; the chains stop at D and do not read them.
// D is a multiple of 8 and every row starts on a 16-byte boundary.
template <typename Src>
__device__ __forceinline__ void out_stage_slice(unsigned char* __restrict__ lds, Src src, int d0, int D) {
  const int unit = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  const int d = d0 + 8 * unit;
  uint4 v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint16_t* p = src(r0 + 32 * k);
    v[k] = (p && d < D) ? *reinterpret_cast<const uint4*>(p + d) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) *reinterpret_cast<uint4*>(lds + (r0 + 32 * k) * OUT_PITCH + 16 * unit) = v[k];
}
__device__ __forceinline__ void out_unit_floats(const uint4 v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = (float)__builtin_bit_cast(half_t, (uint16_t)(w[j] & 0xFFFFu));
    f[2 * j + 1] = (float)__builtin_bit_cast(half_t, (uint16_t)(w[j] >> 16));
  }
}

// hn[c] = 0.5f * chain of cent[c][d]^2 (k_km_finalise's definition), stat = {max|cent|, max hn} as fp32 bits (k_assign_thr_l2's input)
__device__ __forceinline__ void out_prepare_finish(int64_t c, int64_t C, float acc, float amax, float* __restrict__ half_sqnorm,
                                                   uint32_t* __restrict__ stat) {
  float hn = 0.f;
  if (c < C) {
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
__global__ __launch_bounds__(256) void k_out_prepare(const uint16_t* __restrict__ cent, int64_t C, int D, float* __restrict__ half_sqnorm,
                                                     uint32_t* __restrict__ stat) {
  for (int64_t base = (int64_t)blockIdx.x * 256; base < C; base += (int64_t)gridDim.x * 256) {   // uniform over the workgroup
    const int64_t c = base + threadIdx.x;
    float amax = 0.f, acc = 0.f;
    if (c < C) {
      for (int d = 0; d < D; ++d) {
        const float v = (float)__builtin_bit_cast(half_t, cent[c * D + d]);
        acc += v * v;
        amax = fmaxf(amax, __builtin_fabsf(v));
      }
    }
    out_prepare_finish(c, C, acc, amax, half_sqnorm, stat);
  }
}
// the same through LDS: D a multiple of 8; OUT_STAGE_BYTES of dynamic LDS
__global__ __launch_bounds__(OUT_TILE) void k_out_prepare_sl(const uint16_t* __restrict__ cent, int64_t C, int D,
                                                             float* __restrict__ half_sqnorm, uint32_t* __restrict__ stat) {
  extern __shared__ __attribute__((aligned(16))) unsigned char out_lds[];
  for (int64_t base = (int64_t)blockIdx.x * OUT_TILE; base < C; base += (int64_t)gridDim.x * OUT_TILE) {   // uniform over the workgroup
    const int64_t c = base + threadIdx.x;
    float amax = 0.f, acc = 0.f;
    for (int d0 = 0; d0 < D; d0 += OUT_KS) {
      out_stage_slice(out_lds, [&](int r) { return base + r < C ? cent + (base + r) * D : nullptr; }, d0, D);
      __syncthreads();
      if (c < C) {
        const int nu = min(OUT_KS, D - d0) >> 3;   // the chain stops at D
        for (int u = 0; u < nu; ++u) {
          float f[8];
          out_unit_floats(*reinterpret_cast<const uint4*>(out_lds + threadIdx.x * OUT_PITCH + 16 * u), f);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            acc += f[j] * f[j];
            amax = fmaxf(amax, __builtin_fabsf(f[j]));
          }
        }
      }
      __syncthreads();   // the slice is overwritten by the next one
    }
    out_prepare_finish(c, C, acc, amax, half_sqnorm, stat);
  }
}
// FP_TEST=out_staged=0 (A/B runs): dims above 256 through the one-thread-per-row kernels too; the bits are the same
static bool out_staged(int D) {
  static const bool on = fp_test_opt("out_staged", 1) != 0;
  return on && D > 256 && (D & 7) == 0;
}
void fpk_out_prepare(const uint16_t* cent, int64_t C, int D, float* half_sqnorm, uint32_t* stat, hipStream_t st) {
  (void)hipMemsetAsync(stat, 0, 8, st);
  const dim3 grid(fp_grid_cap((C + 255) / 256, 256));
  if (out_staged(D))
    hipLaunchKernelGGL(k_out_prepare_sl, grid, dim3(OUT_TILE), OUT_STAGE_BYTES, st, cent, C, D, half_sqnorm, stat);
  else
    hipLaunchKernelGGL(k_out_prepare, grid, dim3(256), 0, st, cent, C, D, half_sqnorm, stat);
}

// what follows a token's chains: the outputs of row t (sd is NaN for a label outside [0, C)), the flag, and the tile's count
__device__ __forceinline__ void out_tile_finish(int64_t t, int64_t T, int64_t tile, int32_t c, float sd, float thr, float* __restrict__ sqdist,
                                                int64_t* __restrict__ nearest, uint8_t* __restrict__ flag, int32_t* __restrict__ tilecnt,
                                                int32_t* wcnt /*LDS [OUT_TILE / 64]*/) {
  bool out = false;
  if (t < T) {
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
    int32_t c = -1;
    float sd = __uint_as_float(0x7FC00000u);
    if (t < T) {
      c = labels[t];
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
    }
    out_tile_finish(t, T, tile, c, sd, thr, sqdist, nearest, flag, tilecnt, wcnt);
  }
}

// The same through LDS (D a multiple of 8, 2 * OUT_STAGE_BYTES of dynamic LDS): per K-slice the tile's token slices and the slices
// of their labels' centroid rows are staged side by side, then thread i walks both in ascending d -- dot and x2 are the chains of
// k_outlier_dist, step for step, and everything after them is its epilogue.  A token past T or with a label outside [0, C) stages
// zeros and walks nothing.
__global__ __launch_bounds__(OUT_TILE) void k_outlier_dist_sl(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent,
                                                              int64_t C, int D, const float* __restrict__ half_sqnorm,
                                                              const int32_t* __restrict__ labels, float thr, float* __restrict__ sqdist,
                                                              int64_t* __restrict__ nearest /*nullable*/, uint8_t* __restrict__ flag,
                                                              int32_t* __restrict__ tilecnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char out_lds[];
  __shared__ int32_t wcnt[OUT_TILE / 64];
  __shared__ int32_t lab[OUT_TILE];   // the tile's labels, -1: no centroid row to stage
  unsigned char* xs = out_lds;
  unsigned char* ys = out_lds + OUT_STAGE_BYTES;
  const int64_t ntile = (T + OUT_TILE - 1) / OUT_TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {   // uniform over the workgroup
    const int64_t t0 = tile * OUT_TILE, t = t0 + threadIdx.x;
    const int32_t c = t < T ? labels[t] : -1;
    const bool ok = c >= 0 && (int64_t)c < C;   // always for t < T, once an overflowed chunk has been through the exact kernel
    lab[threadIdx.x] = ok ? c : -1;
    __syncthreads();
    float dot = 0.f, x2 = 0.f;
    for (int d0 = 0; d0 < D; d0 += OUT_KS) {
      out_stage_slice(xs, [&](int r) { return lab[r] >= 0 ? emb + (t0 + r) * D : nullptr; }, d0, D);
      out_stage_slice(ys, [&](int r) { return lab[r] >= 0 ? cent + (int64_t)lab[r] * D : nullptr; }, d0, D);
      __syncthreads();
      if (ok) {
        const int nu = min(OUT_KS, D - d0) >> 3;   // the chains stop at D
        for (int u = 0; u < nu; ++u) {
          float x[8], y[8];
          out_unit_floats(*reinterpret_cast<const uint4*>(xs + threadIdx.x * OUT_PITCH + 16 * u), x);
          out_unit_floats(*reinterpret_cast<const uint4*>(ys + threadIdx.x * OUT_PITCH + 16 * u), y);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            dot += x[j] * y[j];
            x2 += x[j] * x[j];
          }
        }
      }
      __syncthreads();   // the slices are overwritten by the next ones, lab[] by the next tile
    }
    float sd = __uint_as_float(0x7FC00000u);
    if (ok) {
      const float s = dot - half_sqnorm[c];
      sd = x2 - 2.0f * s;
    }
    out_tile_finish(t, T, tile, c, sd, thr, sqdist, nearest, flag, tilecnt, wcnt);
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
  if (out_staged(D)) {
    static std::atomic<uint64_t> ok{0};
    fp_allow_big_lds((const void*)k_outlier_dist_sl, ok, 2 * OUT_STAGE_BYTES);
    hipLaunchKernelGGL(k_outlier_dist_sl, dim3(blocks), dim3(OUT_TILE), 2 * OUT_STAGE_BYTES, st, emb, T, cent, C, D, half_sqnorm, labels, thr,
                       sqdist, nearest, flag, tilecnt);
  } else {
    hipLaunchKernelGGL(k_outlier_dist, dim3(blocks), dim3(OUT_TILE), 0, st, emb, T, cent, C, D, half_sqnorm, labels, thr, sqdist, nearest, flag,
                       tilecnt);
  }
  hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(1024), 0, st, tilecnt, ntile, tileoff, count);
  hipLaunchKernelGGL(k_out_write, dim3(blocks), dim3(OUT_TILE), 0, st, flag, T, row0, tileoff, rows);
}
