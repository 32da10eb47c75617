// Token-score matrices (search.rs:651-653, :668-686) and reconstruct_embeddings (embeddings.rs:12-69) for every dim and q_len an
// index accepts: k_token_scores_tile and k_reconstruct_units.  Both read the token's stored norm (FpIndexDev::norms, the
// reference's ascending-k chain, taken once at index creation) instead of walking that chain on one lane, and both decode a
// token in 8-dim units exactly as the MaxSim repair kernels do: e = h(c + w) by the packed fp16 add, e^ = h(fl32(e / n)) by the
// compensated reciprocal (norm_pair2; fp_selftest_arith proves both equal to the reference's formulation).  The kernels they
// replace on the default path (k_token_scores / k_reconstruct, fp_index_ops.hip) stay reachable under FP_TEST=tok_tiled=0.
// This file is compiled without packed fp32 instructions (csrc/Makefile): the chains below are single v_fma_f32 steps.
#include "fp_internal.h"

#include "fp_device.h"

bool fpk_tok_tiled() { static const bool on = fp_test_opt("tok_tiled", 1) != 0; return on; }

// Unit u (dims 8u .. 8u + 7) of one stored token, decoded and normalised, as four packed fp16 pairs.  cp / rp: the token's
// centroid and residual rows; lut: the byte -> weights table [256][8 / NBITS] (LDS or global); r_hi + r_lo: recip2 of its norm.
template <int NBITS>
__device__ __forceinline__ void tok_unit(const uint16_t* __restrict__ cp, const uint8_t* __restrict__ rp, int u, int nu, int native,
                                         const uint16_t* lut, float r_hi, float r_lo, uint32_t (&e)[4]) {
  constexpr int PB = 8 / NBITS;
  const uint4 v = *reinterpret_cast<const uint4*>(cp + 8 * u);
  e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
  const uint8_t* bp = rp + (native ? fp_resid_native_unit(u, nu) : u) * NBITS;   // the unit's NBITS residual bytes
  uint32_t rw[2] = {0u, 0u};
  if constexpr (NBITS == 1) rw[0] = bp[0];
  else if constexpr (NBITS == 2) rw[0] = *reinterpret_cast<const uint16_t*>(bp);
  else if constexpr (NBITS == 4) rw[0] = *reinterpret_cast<const uint32_t*>(bp);
  else { const uint2 w = *reinterpret_cast<const uint2*>(bp); rw[0] = w.x; rw[1] = w.y; }
#pragma unroll
  for (int kk = 0; kk < NBITS; ++kk) {   // byte kk holds the dims [kk * PB, kk * PB + PB) of the unit
    const uint32_t byte = (rw[kk >> 2] >> (8 * (kk & 3))) & 0xFFu;
    if constexpr (PB >= 2) {
#pragma unroll
      for (int j = 0; j < PB / 2; ++j) {
        const uint32_t wv = *reinterpret_cast<const uint32_t*>(&lut[byte * PB + 2 * j]);
        const int ei = kk * (PB / 2) + j;
        e[ei] = h2_as_u32(u32_as_h2(e[ei]) + u32_as_h2(wv));
      }
    } else if ((kk & 1) == 0) {   // nbits 8: two bytes make one packed register
      const uint32_t byte1 = (rw[(kk + 1) >> 2] >> (8 * ((kk + 1) & 3))) & 0xFFu;
      const uint32_t wv = (uint32_t)lut[byte] | ((uint32_t)lut[byte1] << 16);
      e[kk / 2] = h2_as_u32(u32_as_h2(e[kk / 2]) + u32_as_h2(wv));
    }
  }
  norm_pair2(e[0], e[1], r_hi, r_lo);
  norm_pair2(e[2], e[3], r_hi, r_lo);
}

// eight fp16 values (four packed pairs) widened to fp32 into column `col` of a k-major [.][64] LDS slice, rows k .. k + 7
__device__ __forceinline__ void tok_spread(float* __restrict__ dst, const uint32_t (&e)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const h2 v = u32_as_h2(e[p]);
    dst[(2 * p) * 64] = (float)v.x;
    dst[(2 * p + 1) * 64] = (float)v.y;
  }
}

// ---- token scores ----------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per tile = (hit, 64 stored tokens, 64 query rows); the host lists the tiles {hit, first token, first
// query row} while it sizes the output (fp_token_scores), so a ragged batch launches no empty workgroup and the grid does not
// depend on the longest document; a grid-stride loop takes tile counts beyond one dispatch.  The contraction is walked in slices of
// TOK_KS = 64 dims: per slice the 64 tokens are decoded (thread = one token x two units) and the 64 query rows widened into two
// k-major fp32 LDS slices [64][64] (32 KiB together, whatever dim and q_len are), then thread (tx, ty) runs 64 chain steps on its
// 4 tokens x 4 query rows: one 16-byte LDS read of its tokens, one 16-byte broadcast read of its rows, 16 v_fma_f32.  The 16
// accumulators live in registers across the slices, so each output is ONE chain acc = fma(e^_k, q_k, acc) over ascending k from
// +0 -- the reference's order (products of fp16 pairs are exact in fp32).  Operands are fp32 in LDS so that the compiler has no
// fp16 pair to fold into a dot instruction.  Tokens / rows past the document / query are clamped to the tile's first one: they
// compute a valid chain that is not stored.
#define TOK_KS 64
template <int NBITS>
__global__ __launch_bounds__(256) void k_token_scores_tile(const uint16_t* __restrict__ cent, const uint16_t* __restrict__ lut_g,
                                                           const int32_t* __restrict__ codes, const uint16_t* __restrict__ norms,
                                                           const uint8_t* __restrict__ resid, const int64_t* __restrict__ doc_off,
                                                           const uint16_t* __restrict__ perm, int D, int native,
                                                           const uint16_t* __restrict__ queries /*[nq][Q][D]*/, int Q,
                                                           const int32_t* __restrict__ hit_query, const int32_t* __restrict__ hit_pid,
                                                           const int64_t* __restrict__ out_off, const int32_t* __restrict__ tiles /*[n_tiles][3]*/,
                                                           int64_t n_tiles, uint16_t* __restrict__ out) {
  constexpr int PB = 8 / NBITS;
  __shared__ __attribute__((aligned(16))) float Es[TOK_KS * 64];   // [k][token]
  __shared__ __attribute__((aligned(16))) float Qs[TOK_KS * 64];   // [k][query row]
  __shared__ __attribute__((aligned(4))) uint16_t slut[256 * PB];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;      // chain role: tokens 4 tx .. 4 tx + 3, query rows 4 ty .. 4 ty + 3
  const int dt = tid & 63, du0 = tid >> 6;     // staging role: token / query row dt, units du0 and du0 + 4 of the slice
  for (int i = tid; i < 256 * PB; i += 256) slut[i] = lut_g[i];
  const int nu = D >> 3, pr = nu * NBITS;
  for (int64_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const int h = tiles[3 * ti], s0 = tiles[3 * ti + 1], j0 = tiles[3 * ti + 2];
    const int32_t pid = hit_pid[h];
    const int64_t t0 = doc_off[pid];
    const int len = (int)(doc_off[pid + 1] - t0);
    const int64_t t = t0 + (s0 + dt < len ? s0 + dt : s0);
    const uint16_t* cp = cent + (int64_t)codes[t] * D;
    const uint8_t* rp = resid + t * pr;
    float r_hi, r_lo;
    recip2((float)__builtin_bit_cast(half_t, norms[t]), r_hi, r_lo);
    const uint16_t* qp = queries + ((int64_t)hit_query[h] * Q + (j0 + dt < Q ? j0 + dt : j0)) * D;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int u0 = 0; u0 < nu; u0 += TOK_KS / 8) {
      const int nus = nu - u0 < TOK_KS / 8 ? nu - u0 : TOK_KS / 8;   // units of this slice
      __syncthreads();   // the previous slice's chain steps are done (first pass: slut is filled)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int du = du0 + 4 * i;
        if (du < nus) {
          uint32_t e[4];
          tok_unit<NBITS>(cp, rp, u0 + du, nu, native, slut, r_hi, r_lo, e);
          tok_spread(Es + du * 8 * 64 + dt, e);
          const uint4 qv = *reinterpret_cast<const uint4*>(qp + 8 * (u0 + du));
          const uint32_t qe[4] = {qv.x, qv.y, qv.z, qv.w};
          tok_spread(Qs + du * 8 * 64 + dt, qe);
        }
      }
      __syncthreads();
      for (int kk = 0; kk < nus * 8; kk += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float4 a = *reinterpret_cast<const float4*>(Es + (kk + k) * 64 + 4 * tx);
          const float4 b = *reinterpret_cast<const float4*>(Qs + (kk + k) * 64 + 4 * ty);
          const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
        }
      }
    }
    uint16_t* o = out + out_off[h];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = s0 + 4 * tx + i;
      if (s >= len) continue;
      const int torig = perm ? (int)perm[t0 + s] : s;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int jj = j0 + 4 * ty + j;
        if (jj < Q) o[(int64_t)jj * len + torig] = __builtin_bit_cast(uint16_t, (half_t)acc[i][j]);
      }
    }
  }
}

void fpk_token_scores_tile(const FpIndexDev& ix, const uint16_t* queries, int Q, const int32_t* hit_query, const int32_t* hit_pid,
                           const int64_t* out_off, const int32_t* tiles, int64_t n_tiles, uint16_t* out, hipStream_t st) {
  if (n_tiles <= 0) return;
  const dim3 grid(fp_grid_cap(n_tiles, 256));
#define TOK_LAUNCH(NB_)                                                                                                              \
  hipLaunchKernelGGL((k_token_scores_tile<NB_>), grid, dim3(256), 0, st, ix.centroids, ix.lut, ix.codes, ix.norms, ix.residuals,    \
                     ix.doc_off, ix.perm, ix.dim, ix.resid_native, queries, Q, hit_query, hit_pid, out_off, tiles, n_tiles, out)
  switch (ix.nbits) {
    case 1: TOK_LAUNCH(1); break;
    case 2: TOK_LAUNCH(2); break;
    case 4: TOK_LAUNCH(4); break;
    default: TOK_LAUNCH(8); break;
  }
#undef TOK_LAUNCH
}

// ---- reconstruct_embeddings -------------------------------------------------------------------------------------------------
// One wave per token, four tokens per workgroup; lane l takes the units l, l + 64, ... and stores (float)e^ as 32-byte runs.  No
// LDS (the weight table is read through the cache), no chain, no limit below the index's own dim <= 1024.
template <int NBITS>
__global__ __launch_bounds__(256) void k_reconstruct_units(const uint16_t* __restrict__ cent, const uint16_t* __restrict__ lut,
                                                           const int32_t* __restrict__ codes, const uint16_t* __restrict__ norms,
                                                           const uint8_t* __restrict__ resid, int D, int native,
                                                           const int64_t* __restrict__ tok_idx, int64_t n, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int nu = D >> 3, pr = nu * NBITS;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
    const int64_t t = tok_idx[r];
    const uint16_t* cp = cent + (int64_t)codes[t] * D;
    const uint8_t* rp = resid + t * pr;
    float r_hi, r_lo;
    recip2((float)__builtin_bit_cast(half_t, norms[t]), r_hi, r_lo);
    for (int u = lane; u < nu; u += 64) {
      uint32_t e[4];
      tok_unit<NBITS>(cp, rp, u, nu, native, lut, r_hi, r_lo, e);
      float4 lo, hi;
      lo.x = (float)u32_as_h2(e[0]).x; lo.y = (float)u32_as_h2(e[0]).y; lo.z = (float)u32_as_h2(e[1]).x; lo.w = (float)u32_as_h2(e[1]).y;
      hi.x = (float)u32_as_h2(e[2]).x; hi.y = (float)u32_as_h2(e[2]).y; hi.z = (float)u32_as_h2(e[3]).x; hi.w = (float)u32_as_h2(e[3]).y;
      float4* op = reinterpret_cast<float4*>(out + r * D + 8 * u);
      op[0] = lo;
      op[1] = hi;
    }
  }
}

void fpk_reconstruct_units(const FpIndexDev& ix, const int64_t* tok_idx, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return;
  const dim3 grid(fp_grid_cap((n + 3) / 4, 256));
#define REC_LAUNCH(NB_)                                                                                                            \
  hipLaunchKernelGGL((k_reconstruct_units<NB_>), grid, dim3(256), 0, st, ix.centroids, ix.lut, ix.codes, ix.norms, ix.residuals,  \
                     ix.dim, ix.resid_native, tok_idx, n, out)
  switch (ix.nbits) {
    case 1: REC_LAUNCH(1); break;
    case 2: REC_LAUNCH(2); break;
    case 4: REC_LAUNCH(4); break;
    default: REC_LAUNCH(8); break;
  }
#undef REC_LAUNCH
}
