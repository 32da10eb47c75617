// Kernels beside the search path (stage map: fp_kernels.hip): k_narrow, k_ivf_check_sorted, k_reconstruct (embeddings.rs),
// k_token_scores (search.rs:668-686), k_assign_* / k_quantize_pack (index/create.rs:148-184, :404-428), the exhaustive
// arithmetic self-test.
#include <algorithm>
#include <atomic>

#include "fp_internal.h"

#include "fp_device.h"

// ============================================================================================
// misc
// ============================================================================================
// bad (may be null): counts the entries outside [0, limit) -- a code that is no centroid, a list entry that is no document
__global__ void k_narrow(const int64_t* __restrict__ in, int32_t* __restrict__ out, int64_t n, int64_t add, int64_t limit, uint32_t* __restrict__ bad) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = in[i];
    if (bad && (v < 0 || v >= limit)) atomicAdd(bad, 1u);
    out[i] = (int32_t)(v + add);
  }
}
void fpk_narrow_i64_i32(const int64_t* in, int32_t* out, int64_t n, int64_t add, hipStream_t st, int64_t limit, uint32_t* bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_narrow, dim3(fp_grid_cap((n + 255) / 256, 256)), dim3(256), 0, st, in, out, n, add, limit, bad);
}

// the IVF lists as construct_index receives them: *flag != 0 when some list is not strictly ascending (the reference sorts and
// de-duplicates the gathered ids per query, search.rs:538-541, so it takes any order; S3's range cut needs ascending lists).
// One wave per list.
__global__ __launch_bounds__(256) void k_ivf_check_sorted(const int64_t* __restrict__ off, const int32_t* __restrict__ pids, int64_t P,
                                                          uint32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  for (int64_t list = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); list < P; list += (int64_t)gridDim.x * 4) {
    const int64_t beg = off[list], end = off[list + 1];
    bool bad = false;
    for (int64_t i = beg + lane; i + 1 < end; i += 64) bad |= pids[i] >= pids[i + 1];
    if (bad) atomicOr(flag, 1u);
  }
}
void fpk_ivf_check_sorted(const int64_t* off, const int32_t* pids, int64_t P, uint32_t* flag, hipStream_t st) {
  if (P <= 0) return;
  hipLaunchKernelGGL(k_ivf_check_sorted, dim3(fp_grid_cap((P + 3) / 4, 256)), dim3(256), 0, st, off, pids, P, flag);
}

// reconstruct_embeddings (embeddings.rs:12-69): decompress rows to fp32.  One 64-thread
// block per token; the fp32 sum of squares is taken in ascending-dim order by one lane so
// the result is bit-identical to the CPU reference order.
__global__ __launch_bounds__(64) void k_reconstruct(const uint16_t* __restrict__ cent, const uint16_t* __restrict__ lut,
                                                    const int32_t* __restrict__ codes, const uint8_t* __restrict__ resid, int D,
                                                    int nbits, const int64_t* __restrict__ tok_idx, float* __restrict__ out, int native) {
  __shared__ float e[512];
  __shared__ float nrm;
  const int64_t t = tok_idx[blockIdx.x];
  const int pb = 8 / nbits, pr = D * nbits / 8;
  const int32_t code = codes[t];
  for (int d = threadIdx.x; d < D; d += 64) {
    const int byte = resid[t * pr + fp_resid_pos(d / pb, nbits, D / 8, native)];
    const half_t w = __builtin_bit_cast(half_t, lut[byte * pb + d % pb]);
    const half_t c = __builtin_bit_cast(half_t, cent[(int64_t)code * D + d]);
    e[d] = (float)(half_t)((float)w + (float)c);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ss = 0.f;
    for (int d = 0; d < D; ++d) ss += e[d] * e[d];
    nrm = (float)(half_t)__builtin_sqrtf(ss);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 64) out[(int64_t)blockIdx.x * D + d] = (float)(half_t)(e[d] / nrm);
}

void fpk_reconstruct(const FpIndexDev& ix, const int64_t* tok_idx, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_reconstruct, dim3((unsigned)n), dim3(64), 0, st, ix.centroids, ix.lut, ix.codes, ix.residuals, ix.dim, ix.nbits,
                     tok_idx, out, ix.resid_native);
}

// token-score matrices (search.rs:651-653, :668-686): one 64-thread block per hit.  Per token: decompress exactly like
// k_reconstruct (ascending fp32 norm chain), then lane j takes query token j (loop for q_len > 64): ascending-k fp32
// chain, one rounding to fp16 -- the CPU reference's order, so the matrices are bit-identical to the oracle.
__global__ __launch_bounds__(64) void k_token_scores(const uint16_t* __restrict__ cent, const uint16_t* __restrict__ lut,
                                                     const int32_t* __restrict__ codes, const uint8_t* __restrict__ resid,
                                                     const int64_t* __restrict__ doc_off, const uint16_t* __restrict__ perm, int D, int nbits,
                                                     const uint16_t* __restrict__ queries /*[nq][Q][D]*/, int Q,
                                                     const int32_t* __restrict__ hit_query, const int32_t* __restrict__ hit_pid,
                                                     const int64_t* __restrict__ out_off, uint16_t* __restrict__ out, int native) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* qs = reinterpret_cast<float*>(smem);          // [Q][D] the hit's query as fp32
  float* e = qs + (size_t)Q * D;                       // [D]
  __shared__ float nrm;
  const int h = blockIdx.x;
  const int32_t pid = hit_pid[h];
  const uint16_t* q = queries + (int64_t)hit_query[h] * Q * D;
  for (int i = threadIdx.x; i < Q * D; i += 64) qs[i] = (float)__builtin_bit_cast(half_t, q[i]);
  const int64_t t0 = doc_off[pid];
  const int len = (int)(doc_off[pid + 1] - t0);
  const int pb = 8 / nbits, pr = D * nbits / 8;
  uint16_t* o = out + out_off[h];
  for (int s = 0; s < len; ++s) {
    const int64_t t = t0 + s;
    const int32_t code = codes[t];
    __syncthreads();  // e / nrm of the previous token are no longer read
    for (int d = threadIdx.x; d < D; d += 64) {
      const int byte = resid[t * pr + fp_resid_pos(d / pb, nbits, D / 8, native)];
      const half_t w = __builtin_bit_cast(half_t, lut[byte * pb + d % pb]);
      const half_t c = __builtin_bit_cast(half_t, cent[(int64_t)code * D + d]);
      e[d] = (float)(half_t)((float)w + (float)c);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float ss = 0.f;
      for (int d = 0; d < D; ++d) ss += e[d] * e[d];
      nrm = (float)(half_t)__builtin_sqrtf(ss);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 64) e[d] = (float)(half_t)(e[d] / nrm);
    __syncthreads();
    const int torig = perm ? (int)perm[t] : s;
    for (int j = threadIdx.x; j < Q; j += 64) {
      const float* qq = qs + (size_t)j * D;
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc += e[d] * qq[d];   // products of two fp16 values are exact in fp32: mul+add == fma
      o[(int64_t)j * len + torig] = __builtin_bit_cast(uint16_t, (half_t)acc);
    }
  }
}

int fpk_token_scores(const FpIndexDev& ix, const uint16_t* queries, int Q, const int32_t* hit_query, const int32_t* hit_pid, int64_t n_hits,
                     const int64_t* out_off, uint16_t* out, hipStream_t st) {
  if (n_hits <= 0) return 0;
  const size_t lds = ((size_t)Q * ix.dim + ix.dim) * sizeof(float);
  if (lds > 150 * 1024) return -1;
  static std::atomic<uint64_t> lds_ok{0};
  fp_allow_big_lds((const void*)k_token_scores, lds_ok, 152 * 1024);
  for (int64_t h0 = 0; h0 < n_hits; h0 += 0x7FFFFF00ll / 64) {   // grid.x * 64 threads must stay below 2^32
    const int64_t nh = std::min<int64_t>(n_hits - h0, 0x7FFFFF00ll / 64);
    hipLaunchKernelGGL(k_token_scores, dim3((unsigned)nh), dim3(64), lds, st, ix.centroids, ix.lut, ix.codes, ix.residuals, ix.doc_off, ix.perm,
                       ix.dim, ix.nbits, queries, Q, hit_query + h0, hit_pid + h0, out_off + h0, out, ix.resid_native);
  }
  return 0;
}

// ============================================================================================
// index creation, device part (create.rs:148-184, :404-428)
// ============================================================================================
// Nearest centroid, EXACT: the reference takes argmax over h(fp32 dot) of an ATen half matmul, whose fp32 sum runs in
// ascending k; an MFMA contraction sums in another order, which moves ~0.05 % of the fp16-rounded scores by an ulp and
// would flip the argmax between near-tied centroids.  Codes are integers and must be identical, so this kernel keeps
// one ascending-k fp32 chain per (token, centroid): 64 tokens x 64 centroids per tile, 4x4 outputs per thread, operands
// in LDS as fp32.  Ties go to the lowest centroid index (torch.argmax: first maximal value).
// L2 = true (k-means assignment): score = dot - half_sqnorm[c] compared in fp32 instead of the fp16-rounded dot.
template <bool L2>
__global__ __launch_bounds__(256) void k_assign_exact(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent,
                                                      int64_t C, const float* __restrict__ half_sqnorm, int32_t* __restrict__ codes, int D) {
  // any dim (runtime): As / Bs [64][D + 1] fp32 and best_s [64][16] in dynamic LDS
  extern __shared__ __attribute__((aligned(16))) unsigned char xsm[];
  const int ld = D + 1;
  float* As_ = reinterpret_cast<float*>(xsm);
  float* Bs_ = As_ + 64 * ld;
  unsigned long long (*best_s)[16] = reinterpret_cast<unsigned long long (*)[16]>(xsm + (size_t)2 * 64 * ld * 4);
#define As(r, d) As_[(r) * ld + (d)]
#define Bs(r, d) Bs_[(r) * ld + (d)]
  const int tid = threadIdx.x;
  const int tr = tid >> 4, tc = tid & 15;       // 16 x 16 threads, 4 rows x 4 cols each
  const int64_t t0 = (int64_t)blockIdx.x * 64;
  for (int i = tid; i < 64 * D; i += 256) {
    const int r = i / D, d = i % D;
    As(r, d) = (t0 + r < T) ? (float)__builtin_bit_cast(half_t, emb[(t0 + r) * D + d]) : 0.f;
  }
  unsigned long long best[4] = {0ull, 0ull, 0ull, 0ull};
  for (int64_t c0 = 0; c0 < C; c0 += 64) {
    __syncthreads();
    for (int i = tid; i < 64 * D; i += 256) {
      const int r = i / D, d = i % D;
      Bs(r, d) = (c0 + r < C) ? (float)__builtin_bit_cast(half_t, cent[(c0 + r) * D + d]) : 0.f;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kk = 0; kk < D; ++kk) {   // ascending k: each accumulator is the reference's chain (products of fp16 pairs are exact in fp32)
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As(tr * 4 + i, kk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs(tc + 16 * j, kk);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + tc + 16 * j;
        if (c < C) {
          uint32_t ord;
          if constexpr (L2) {
            const uint32_t fb = __float_as_uint(acc[i][j] - half_sqnorm[c]);
            ord = fb ^ ((fb >> 31) ? 0xFFFFFFFFu : 0x80000000u);   // order-preserving key of an fp32 value
          } else {
            ord = mono16(__builtin_bit_cast(uint16_t, (half_t)acc[i][j]));
          }
          const unsigned long long key = ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)c);
          best[i] = key > best[i] ? key : best[i];   // higher score, then lower index
        }
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) best_s[tr * 4 + i][tc] = best[i];
  __syncthreads();
  if (tid < 64 && t0 + tid < T) {
    unsigned long long m = 0ull;
    for (int j = 0; j < 16; ++j) m = best_s[tid][j] > m ? best_s[tid][j] : m;
    codes[t0 + tid] = (int32_t)(0xFFFFFFFFu - (uint32_t)(m & 0xFFFFFFFFull));
  }
#undef As
#undef Bs
}
static size_t assign_exact_lds(int D) { return (size_t)2 * 64 * (D + 1) * 4 + 64 * 16 * 8; }
#define ASSIGN_MAX_DIM 256   // 2 x 64 x (D+1) fp32 operand tiles + 8 KiB must fit the 160 KiB of LDS

// ---- MFMA fast path of the nearest-centroid search, still exact -------------------------------------------------------
// The exact kernel above runs at 30 TFLOP/s.  MFMA sums in another order, so its scores cannot decide near-ties; but they
// can NARROW the search: pass 1 finds, per token, the maximum MFMA score m; pass 2 collects every centroid whose MFMA score
// is within one fp16 ulp (plus twice the worst-case summation error) of m -- the true argmax of the fp16-rounded exact
// scores is always among them (see k_assign_thr) -- and k_assign_recheck evaluates only those (1-2 per token, at most
// ASSIGN_CAP) with the ascending-k chain and the first-index tie rule.  A token that collects more than ASSIGN_CAP
// candidates (many near-duplicate centroids) sends the whole chunk back to the exact kernel.
// L2 = true (k-means assignment, fpk_assign_l2_narrow): the score is fl32(MFMA dot - half_sqnorm[c]); pass 1 / pass 2 / the
// re-check work on that value and the threshold is k_assign_thr_l2's.
#define ASSIGN_CAP 8
template <int D, int PASS, bool L2>
__global__ __launch_bounds__(256) void k_assign_mfma(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent, int64_t C,
                                                     float* __restrict__ tmax /*PASS 1 out*/, const float* __restrict__ thr /*PASS 2 in*/,
                                                     int32_t* __restrict__ ccnt, int32_t* __restrict__ ccand,
                                                     const float* __restrict__ half_sqnorm /*L2 only*/) {
  constexpr int CH = D / 8;
  constexpr int ROWB = D * 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Ts = smem;               // [128 tokens][ROWB]
  unsigned char* Cs = smem + 128 * ROWB;  // [128 centroids][ROWB]
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * 128;
  const int wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5;
  for (int i = tid; i < 128 * CH; i += 256) {
    const int row = i / CH, j = i % CH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t0 + row < T) v = *reinterpret_cast<const uint4*>(emb + (t0 + row) * D + j * 8);
    *reinterpret_cast<uint4*>(Ts + row * ROWB + ((j ^ (row & (CH - 1))) * 16)) = v;
  }
  // per-lane state over this lane's centroid columns: running maxima (pass 1) or the thresholds of its 32 token rows (pass 2)
  float st[2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (PASS == 1) {
        st[a][r] = -INFINITY;
      } else {
        const int64_t t = t0 + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        st[a][r] = (t < T) ? thr[t] : INFINITY;
      }
    }
  for (int64_t c0 = 0; c0 < C; c0 += 128) {
    __syncthreads();
    for (int i = tid; i < 128 * CH; i += 256) {
      const int row = i / CH, j = i % CH;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c0 + row < C) v = *reinterpret_cast<const uint4*>(cent + (c0 + row) * D + j * 8);
      *reinterpret_cast<uint4*>(Cs + row * ROWB + ((j ^ (row & (CH - 1))) * 16)) = v;
    }
    __syncthreads();
    f16v acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      h8 af[2], bf[2];
      const int j = ks * 2 + hi;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int rq = wr * 64 + t * 32 + l31;
        const int rc = wc * 64 + t * 32 + l31;
        af[t] = *reinterpret_cast<const h8*>(Ts + rq * ROWB + ((j ^ (rq & (CH - 1))) * 16));
        bf[t] = *reinterpret_cast<const h8*>(Cs + rc * ROWB + ((j ^ (rc & (CH - 1))) * 16));
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t c = c0 + wc * 64 + b * 32 + l31;
      if (c >= C) continue;
      float hn = 0.f;
      if constexpr (L2) hn = half_sqnorm[c];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[a][b][r];
          if constexpr (L2) v -= hn;
          if (PASS == 1) {
            st[a][r] = fmaxf(st[a][r], v);
          } else if (v >= st[a][r]) {
            const int64_t t = t0 + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const int pos = atomicAdd(&ccnt[t], 1);
            if (pos < ASSIGN_CAP) ccand[t * ASSIGN_CAP + pos] = (int32_t)c;
          }
        }
    }
  }
  if (PASS == 1) {
    __shared__ float red[2][128];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = st[a][r];
#pragma unroll
        for (int s = 1; s < 32; s <<= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
        if (l31 == 0) red[wc][wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi] = v;
      }
    __syncthreads();
    if (tid < 128 && t0 + tid < T) tmax[t0 + tid] = fmaxf(red[0][tid], red[1][tid]);
  }
}

// thr[t] = m - (two fp16 ulps at |m| + twice the worst-case fp32 summation error of a D-term dot product of this token).
// Why the true winner w is collected: h is monotone, so exact_w > exact_c - ulp16 for every c (else h(exact_c) > h(exact_w));
// with c* = argmax of the MFMA scores and |mfma - exact| <= eps:  mfma_w >= exact_w - eps > exact_c* - ulp16 - eps >= m - ulp16 - 2 eps.
__global__ void k_assign_thr(const uint16_t* __restrict__ emb, int64_t T, int D, float cmaxabs, const float* __restrict__ tmax,
                             float* __restrict__ thr, int32_t* __restrict__ ccnt) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    float l1 = 0.f;
    for (int d = 0; d < D; ++d) l1 += __builtin_fabsf((float)__builtin_bit_cast(half_t, emb[t * D + d]));
    const float m = tmax[t];
    const float ulp2 = __builtin_fmaxf(__builtin_fabsf(m), 6.103515625e-05f) * 0.001953125f;   // 2^-9 |m|  >= 2 ulp16
    const float eps2 = l1 * cmaxabs * (float)D * 1.1920929e-07f * 2.0f;                          // 2 * D * 2^-23 * sum|x_k| max|c|
    thr[t] = m - (ulp2 + eps2);
    ccnt[t] = 0;
  }
}

// The L2 form (k-means): score_c = fl32(dot_c - hn_c), compared in fp32.  thr[t] = M - 2 delta, M the maximum of the MFMA scores.
// Why the exact winner w is collected.  Write e_c for the ascending chain, a_c for the MFMA sum, s_c = fl32(e_c - hn_c) for the
// exact score and m_c = fl32(a_c - hn_c) for the MFMA score.  |a_c - e_c| <= eps = D 2^-23 l1(x) max|c| (two summation orders of
// the same D exact products, each within (D - 1) 2^-24 sum|products| of the true sum: the figure k_assign_thr uses).  A rounded
// difference r = fl32(z) has |r - z| <= 2^-24 |r| (a subnormal difference is exact), and every score satisfies
// |score| <= B = (l1(x) max|c| + max hn)(1 + 2^-16), so |m_c - s_c| <= delta = eps + 2^-23 B.  With c* the argmax of the MFMA
// scores, s_w >= s_c* (w wins the exact comparison), hence
//   m_w >= s_w - delta >= s_c* - delta >= m_c* - 2 delta = M - 2 delta.
// There is no fp16-ulp term: nothing is rounded to fp16 before the comparison.  The kernel takes 2^-22 B in place of 2^-23 B,
// which covers B's factor, the rounding of thr itself (<= 2^-24 B) and of the l1 chain (relative D 2^-24, against the 1 / D
// that D in place of D - 1 leaves in eps).  stat: {max|cent16|, max hn} as fp32 bits, reduced on the device by k_km_finalise
// (both change with every Lloyd iteration).
__global__ void k_assign_thr_l2(const uint16_t* __restrict__ emb, int64_t T, int D, const uint32_t* __restrict__ stat,
                                const float* __restrict__ tmax, float* __restrict__ thr, int32_t* __restrict__ ccnt) {
  const float cmaxabs = __uint_as_float(stat[0]), hnmax = __uint_as_float(stat[1]);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    float l1 = 0.f;
    for (int d = 0; d < D; ++d) l1 += __builtin_fabsf((float)__builtin_bit_cast(half_t, emb[t * D + d]));
    const float dotmax = l1 * cmaxabs;
    const float eps = dotmax * (float)D * 1.1920929e-07f;            // D * 2^-23 * sum|x_k| max|c|
    const float rnd = (dotmax + hnmax) * 2.3841858e-07f;             // 2^-22 B
    thr[t] = tmax[t] - 2.0f * (eps + rnd);
    ccnt[t] = 0;
  }
}

// exact evaluation of the collected candidates; codes[t] = -1 when the candidate list overflowed
template <bool L2>
__global__ void k_assign_recheck(const uint16_t* __restrict__ emb, int64_t T, const uint16_t* __restrict__ cent, int D,
                                 const int32_t* __restrict__ ccnt, const int32_t* __restrict__ ccand, int32_t* __restrict__ codes,
                                 int32_t* __restrict__ overflow, const float* __restrict__ half_sqnorm /*L2 only*/) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
    const int n = ccnt[t];
    if (n > ASSIGN_CAP || n < 1) {   // n < 1 cannot happen (the maximum itself passes its threshold) unless a score is NaN
      codes[t] = -1;
      atomicAdd(overflow, 1);
      continue;
    }
    unsigned long long best = 0ull;
    for (int i = 0; i < n; ++i) {
      const int32_t c = ccand[t * ASSIGN_CAP + i];
      float acc = 0.f;
      for (int d = 0; d < D; ++d)
        acc += (float)__builtin_bit_cast(half_t, emb[t * D + d]) * (float)__builtin_bit_cast(half_t, cent[(int64_t)c * D + d]);
      uint32_t ord;
      if constexpr (L2) {
        const uint32_t fb = __float_as_uint(acc - half_sqnorm[c]);
        ord = fb ^ ((fb >> 31) ? 0xFFFFFFFFu : 0x80000000u);   // k_assign_exact<true>'s key
      } else {
        ord = mono16(__builtin_bit_cast(uint16_t, (half_t)acc));
      }
      const unsigned long long key = ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)c);
      best = key > best ? key : best;
    }
    codes[t] = (int32_t)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull));
  }
}

// residual quantisation + packing: one thread per output byte
__global__ __launch_bounds__(256) void k_quantize_pack(const uint16_t* __restrict__ emb, const uint16_t* __restrict__ cent,
                                                       const int32_t* __restrict__ codes, const uint16_t* __restrict__ cutoffs, int D, int nbits,
                                                       int64_t T, uint8_t* __restrict__ out, int64_t* __restrict__ codes64) {
  const int pr = D * nbits / 8, per = 8 / nbits, ncut = (1 << nbits) - 1;
  const int64_t total = T * pr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = g / pr;
    const int bi = (int)(g % pr);
    const int32_t code = codes[t];
    if (bi == 0) codes64[t] = code;
    unsigned byte = 0;
    for (int v = 0; v < per; ++v) {
      const int d = bi * per + v;
      const float e = (float)__builtin_bit_cast(half_t, emb[t * D + d]);
      const float c = (float)__builtin_bit_cast(half_t, cent[(int64_t)code * D + d]);
      const half_t r = (half_t)(e - c);   // fp16 subtraction == fp32 subtraction rounded once
      int bucket = 0;
      for (int i = 0; i < ncut; ++i) bucket += ((float)__builtin_bit_cast(half_t, cutoffs[i]) < (float)r) ? 1 : 0;
      // bits of `bucket` LSB first, appended to the big-endian bit stream
      for (int kbit = 0; kbit < nbits; ++kbit) byte = (byte << 1) | ((bucket >> kbit) & 1u);
    }
    out[g] = (uint8_t)byte;
  }
}

// scratch: tmax / thr f32 [T], ccnt i32 [T], ccand i32 [T * ASSIGN_CAP], overflow i32 [1]  (all inside `work`, see fpk_compress_work_bytes)
size_t fpk_compress_work_bytes(int64_t T) { return (size_t)T * (4 + 4 + 4 + 4 * ASSIGN_CAP) + 64; }

// pass 1 -> threshold -> pass 2 -> re-check of one chunk on `st` (D 64 or 128); *overflow is zeroed first and counts the tokens
// whose candidate list overflowed.  L2: the k-means score (half_sqnorm, stat = k_assign_thr_l2's device-side maxima)
static int32_t* assign_work_overflow(void* work, int64_t T) { return reinterpret_cast<int32_t*>(static_cast<char*>(work) + (size_t)T * (12 + 4 * ASSIGN_CAP)); }
template <int D, bool L2>
static void assign_narrow_d(const uint16_t* emb, int64_t T, const uint16_t* cent, int64_t C, float cmaxabs, const uint32_t* stat,
                            const float* half_sqnorm, int32_t* codes32, void* work, int32_t* overflow, hipStream_t st) {
  float* tmax = static_cast<float*>(work);
  float* thr = tmax + T;
  int32_t* ccnt = reinterpret_cast<int32_t*>(thr + T);
  int32_t* ccand = ccnt + T;
  const unsigned mblocks = (unsigned)((T + 127) / 128);
  const unsigned tblocks = fp_grid_cap((T + 255) / 256, 256);
  const size_t lds = (size_t)2 * 128 * D * 2;
  (void)hipMemsetAsync(overflow, 0, 4, st);
  if (D == 128) {
    static std::atomic<uint64_t> ok1{0}, ok2{0};
    fp_allow_big_lds((const void*)k_assign_mfma<D, 1, L2>, ok1, 80 * 1024);
    fp_allow_big_lds((const void*)k_assign_mfma<D, 2, L2>, ok2, 80 * 1024);
  }
  hipLaunchKernelGGL((k_assign_mfma<D, 1, L2>), dim3(mblocks), dim3(256), lds, st, emb, T, cent, C, tmax, (const float*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, half_sqnorm);
  if (L2)
    hipLaunchKernelGGL(k_assign_thr_l2, dim3(tblocks), dim3(256), 0, st, emb, T, D, stat, tmax, thr, ccnt);
  else
    hipLaunchKernelGGL(k_assign_thr, dim3(tblocks), dim3(256), 0, st, emb, T, D, cmaxabs, tmax, thr, ccnt);
  hipLaunchKernelGGL((k_assign_mfma<D, 2, L2>), dim3(mblocks), dim3(256), lds, st, emb, T, cent, C, (float*)nullptr, thr, ccnt, ccand, half_sqnorm);
  hipLaunchKernelGGL((k_assign_recheck<L2>), dim3(tblocks), dim3(256), 0, st, emb, T, cent, D, ccnt, ccand, codes32, overflow, half_sqnorm);
}
template <bool L2>
static void assign_narrow(const uint16_t* emb, int64_t T, const uint16_t* cent, int64_t C, int D, float cmaxabs, const uint32_t* stat,
                          const float* half_sqnorm, int32_t* codes32, void* work, int32_t* overflow, hipStream_t st) {
  if (D == 128)
    assign_narrow_d<128, L2>(emb, T, cent, C, cmaxabs, stat, half_sqnorm, codes32, work, overflow, st);
  else
    assign_narrow_d<64, L2>(emb, T, cent, C, cmaxabs, stat, half_sqnorm, codes32, work, overflow, st);
}

static int assign_codes(const uint16_t* emb, int64_t T, const uint16_t* cent, int64_t C, int D, float cmaxabs, int32_t* codes32, void* work,
                        hipStream_t st) {
  static const int impl_env = fp_test_opt("assign_exact", 0) != 0 ? 1 : 0;   // the all-VALU exact kernel only (tools/bench_compress.py)
  const unsigned eblocks = fp_grid_cap((T + 63) / 64, 256);
  if ((int64_t)eblocks * 64 < T) return -2;   // callers chunk far below this
  auto exact = [&]() {
    static std::atomic<uint64_t> ok{0};
    fp_allow_big_lds((const void*)k_assign_exact<false>, ok, 160 * 1024);
    hipLaunchKernelGGL((k_assign_exact<false>), dim3(eblocks), dim3(256), assign_exact_lds(D), st, emb, T, cent, C, (const float*)nullptr, codes32, D);
  };
  if (D < 1 || D > ASSIGN_MAX_DIM) return -1;
  if (impl_env || !work || C < 256 || (D != 128 && D != 64)) {   // tiny tables: the exact kernel is as fast; the MFMA narrowing is built for dim 64 / 128
    exact();
    return 0;
  }
  int32_t* overflow = assign_work_overflow(work, T);
  assign_narrow<false>(emb, T, cent, C, D, cmaxabs, nullptr, nullptr, codes32, work, overflow, st);
  int32_t h_over = 0;
  if (hipMemcpyAsync(&h_over, overflow, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -3;
  if (h_over > 0) exact();   // a token met more than ASSIGN_CAP near-tied centroids: the whole chunk goes through the exact kernel
  return 0;
}

int fpk_compress(const uint16_t* emb, int64_t T, const uint16_t* cent, int64_t C, int D, int nbits, const uint16_t* cutoffs, float cmaxabs,
                 int32_t* codes32, int64_t* codes64, uint8_t* out, void* work, hipStream_t st) {
  if (T <= 0) return 0;
  if (int rc = assign_codes(emb, T, cent, C, D, cmaxabs, codes32, work, st)) return rc;
  const int64_t total = T * (D * nbits / 8);
  hipLaunchKernelGGL(k_quantize_pack, dim3(fp_grid_cap((total + 255) / 256, 256)), dim3(256), 0, st, emb, cent, codes32, cutoffs, D, nbits, T, out,
                     codes64);
  return 0;
}

__global__ void k_widen_i32(const int32_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[i];
}

int fpk_assign_l2_exact(const uint16_t* emb, int64_t T, const uint16_t* cent, const float* half_sqnorm, int64_t C, int D, int32_t* codes32,
                        hipStream_t st) {
  if (T <= 0) return 0;
  const unsigned blocks = fp_grid_cap((T + 63) / 64, 256);
  if ((int64_t)blocks * 64 < T) return -2;
  if (D < 1 || D > ASSIGN_MAX_DIM) return -1;
  static std::atomic<uint64_t> ok{0};
  fp_allow_big_lds((const void*)k_assign_exact<true>, ok, 160 * 1024);
  hipLaunchKernelGGL((k_assign_exact<true>), dim3(blocks), dim3(256), assign_exact_lds(D), st, emb, T, cent, C, half_sqnorm, codes32, D);
  return 0;
}

// k-means assignment of one chunk with the MFMA narrowing (fp_kmeans): labels for dim 64 / 128 and C >= 256, nothing read back.
// Returns 1 when the chunk took the narrowing -- the caller reads *overflow after the stream has drained and sends a chunk with a
// non-zero count through fpk_assign_l2_exact -- 0 when it went straight to the exact kernel, < 0 as fpk_assign_l2.
int fpk_assign_l2_narrow(const uint16_t* emb, int64_t T, const uint16_t* cent, const float* half_sqnorm, const uint32_t* stat, int64_t C, int D,
                         int32_t* codes32, void* work, int32_t* overflow, hipStream_t st) {
  static const int exact_env = fp_test_opt("assign_exact", 0) != 0 ? 1 : 0;
  if (T <= 0) return 0;
  if (exact_env || !work || C < 256 || (D != 128 && D != 64)) return fpk_assign_l2_exact(emb, T, cent, half_sqnorm, C, D, codes32, st);
  if ((T + 127) / 128 > 0x7FFFFFll) return -2;
  assign_narrow<true>(emb, T, cent, C, D, 0.f, stat, half_sqnorm, codes32, work, overflow, st);
  return 1;
}

int fpk_assign_l2(const uint16_t* emb, int64_t T, const uint16_t* cent, const float* half_sqnorm, int64_t C, int D, int32_t* codes32,
                  int64_t* codes64, hipStream_t st) {
  if (T <= 0) return 0;
  if (int rc = fpk_assign_l2_exact(emb, T, cent, half_sqnorm, C, D, codes32, st)) return rc;
  hipLaunchKernelGGL(k_widen_i32, dim3(fp_grid_cap((T + 255) / 256, 256)), dim3(256), 0, st, codes32, codes64, T);
  return 0;
}

// ============================================================================================
// arithmetic self-test: the two shortcuts the MaxSim kernel takes must equal the reference
// formulation (fp32 op + one rounding to fp16) for EVERY pair of fp16 bit patterns.
//   out[0]: REACHABLE pairs (n >= 0, |e| <= n(1+2^-9): a component never exceeds its vector's
//           norm) where h(quot2(e, 1/n as r_hi + r_lo)) != h(fl32(e / n))          -- must be 0
//   out[2]: (informational) the same for the single product h(fl32(e * fl32(1/n)))
//   out[3]: (informational) mismatches of quot2 over ALL pairs (unreachable specials such as
//           e = inf with finite n give inf - inf = NaN instead of inf)
//   out[1]: pairs where (packed fp16 add)(a, b)  != h(fl32(a + b))
// NaN results compare equal to NaN.
// ============================================================================================
__device__ __forceinline__ bool same_h(half_t a, half_t b) {
  uint16_t x = __builtin_bit_cast(uint16_t, a), y = __builtin_bit_cast(uint16_t, b);
  bool nx = (x & 0x7FFF) > 0x7C00, ny = (y & 0x7FFF) > 0x7C00;
  bool zx = (x & 0x7FFF) == 0, zy = (y & 0x7FFF) == 0;  // +0 == -0 (e = -0 gives +0: same dot products)
  return (nx && ny) || (zx && zy) || x == y;
}
__global__ __launch_bounds__(256) void k_selftest_arith(unsigned long long* __restrict__ out) {
  const uint16_t nb = (uint16_t)blockIdx.x;
  const half_t n = __builtin_bit_cast(half_t, nb);
  const float nf = (float)n;
  float r_hi, r_lo;
  recip2(nf, r_hi, r_lo);
  // reachable domain of the MaxSim kernel: n = h(sqrt(sum e_k^2)) >= 0 and no component can
  // exceed its own vector's norm by more than the fp16 rounding of n
  const bool n_ok = !(nb & 0x8000) || (nb & 0x7FFF) > 0x7C00;  // n >= +0, or NaN
  unsigned long long bad_dom = 0, bad_add = 0, bad_plain = 0, bad_all = 0;
  for (uint32_t eb = threadIdx.x * 2; eb < 65536u; eb += 512u) {
    const h2 e = u32_as_h2(eb | ((eb + 1u) << 16));
    uint32_t ea = h2_as_u32(e), eb2 = h2_as_u32(e);
    norm_pair2(ea, eb2, r_hi, r_lo);  // the exact code path of k_maxsim (both registers must agree)
    const h2 qq = u32_as_h2(ea);
    const half_t q0 = qq.x, q1 = (ea == eb2) ? qq.y : (half_t)__builtin_nanf("");
    const half_t d0 = (half_t)((float)e.x / nf), d1 = (half_t)((float)e.y / nf);
    const bool m0 = !same_h(q0, d0), m1 = !same_h(q1, d1);
    bad_all += m0 + m1;
    const bool dom0 = n_ok && !(__builtin_fabsf((float)e.x) > nf * 1.001953125f);
    const bool dom1 = n_ok && !(__builtin_fabsf((float)e.y) > nf * 1.001953125f);
    if (m0 && dom0) {
      ++bad_dom;
      unsigned long long slot = atomicAdd(&out[4], 1ull);
      if (slot < 11) out[5 + slot] = (unsigned long long)(eb & 0xFFFF) | ((unsigned long long)nb << 16) |
                                     ((unsigned long long)__builtin_bit_cast(uint16_t, q0) << 32) |
                                     ((unsigned long long)__builtin_bit_cast(uint16_t, d0) << 48);
    }
    bad_dom += (m1 && dom1);
    bad_plain += (dom0 && !same_h((half_t)((float)e.x * r_hi), d0));
    bad_plain += (dom1 && !same_h((half_t)((float)e.y * r_hi), d1));
    const h2 nn = {n, n};
    const h2 sum = e + nn;
    bad_add += !same_h(sum.x, (half_t)((float)e.x + nf));
    bad_add += !same_h(sum.y, (half_t)((float)e.y + nf));
  }
  if (bad_dom) atomicAdd(&out[0], bad_dom);
  if (bad_add) atomicAdd(&out[1], bad_add);
  if (bad_plain) atomicAdd(&out[2], bad_plain);
  if (bad_all) atomicAdd(&out[3], bad_all);
}
void fpk_selftest_arith(unsigned long long* out_dev, hipStream_t st) {
  hipLaunchKernelGGL(k_selftest_arith, dim3(65536), dim3(256), 0, st, out_dev);
}
