// The stand-alone index-build operators of the C ABI (include/fastplaid.h): fp_compress, fp_assign_l2, fp_kmeans,
// fp_centroid_outliers and fp_residual_stats, with their *_last_* queries.  Host code only: the kernels are behind the fpk_* launchers of fp_internal.h
// (fp_index_ops.hip, fp_kmeans.hip, fp_outliers.hip, fp_codec_stats.hip).  Every operator follows one plan -- validate, select the device, a private
// stream, a handful of device buffers, upload, chunks of at most 2^20 rows, download -- and BuildCall owns what that plan acquires.
#include "../../include/fastplaid.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "fp_host.h"
#include "fp_internal.h"

// ------------------------------------------------------------------------------------------
// one operator call: its stream, device buffers and events; the destructor releases them on every way out
// ------------------------------------------------------------------------------------------
// Buffers are allocated at exactly the bytes asked for (the engine's grow-only DevBuf pads by an eighth: fp_kmeans checks its
// footprint against the free memory, so what it adds up is what is allocated).  A buffer of zero bytes is not allocated and
// stays a null pointer.  BCHK(x), in an operator whose call is `bc`: a HIP failure ends the operator through bc.hip_failed.
#define BCHK(x)                                                                                        \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return bc.hip_failed(e_, #x);                                                \
  } while (0)

namespace {   // (the types of this file stay out of the library's symbol table)
struct BuildCall {
  const char* const op;   // the operator's name, for messages
  const bool enomem;      // hipErrorOutOfMemory is reported as FP_ENOMEM (else FP_EHIP, like every other HIP failure)
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;

  BuildCall(const char* op_, bool enomem_) : op(op_), enomem(enomem_) {}
  BuildCall(const BuildCall&) = delete;
  BuildCall& operator=(const BuildCall&) = delete;
  ~BuildCall() {
    for (void* p : mem) (void)hipFree(p);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
    if (clear_error) (void)hipGetLastError();   // a failed call's error is reported once, by this call: it does not stay behind
  }

  // the device part starts here: nothing before this touches the runtime
  int open(int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fp_fail(FP_EHIP, "no HIP device available (this library has no CPU path)");
    if (device_id < 0 || device_id >= ndev) return fp_fail(FP_EINVAL, "device index out of range");
    HIPCHK(fp_set_device(device_id));
    return FP_OK;
  }
  int hip_failed(hipError_t e, const char* at) {
    clear_error = true;
    return fp_fail(enomem && e == hipErrorOutOfMemory ? FP_ENOMEM : FP_EHIP,
                   std::string("HIP error in ") + op + ": " + hipGetErrorString(e) + " at " + at);
  }
  hipError_t create_events(size_t n) {
    ev.resize(n, nullptr);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < n && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    return e;
  }
  // device memory the Dev buffers declared so far ask for, as fp_kmeans counts it: 256 bytes on top of each for the allocator
  size_t footprint() const {
    size_t need = 0;
    for (const auto& w : wanted) need += w.second + 256;
    return need;
  }
  // every Dev declared so far, in the order of the declarations
  hipError_t hip_malloc_all() {
    for (const auto& w : wanted) {
      if (w.second == 0) continue;
      void* p = nullptr;
      const hipError_t e = hipMalloc(&p, w.second);
      if (e != hipSuccess) return e;
      mem.push_back(p);
      *w.first = p;
    }
    return hipSuccess;
  }
  // us[s] += the microseconds between ev[s] and ev[s + 1] (both reached), s < n
  hipError_t add_elapsed_us(int64_t* us, int n) {
    for (int s = 0; s < n; ++s) {
      float ms = 0.f;
      const hipError_t e = hipEventElapsedTime(&ms, ev[s], ev[s + 1]);
      if (e != hipSuccess) return e;
      us[s] += (int64_t)(ms * 1000.f + 0.5f);
    }
    return hipSuccess;
  }

 private:
  template <typename T> friend struct Dev;
  std::vector<std::pair<void**, size_t>> wanted;   // {where hip_malloc_all() puts the pointer, bytes}
  std::vector<void*> mem;
  bool clear_error = false;
};

// a device buffer of a call: declared with its size, a T* once the call's hip_malloc_all() has run
template <typename T>
struct Dev {
  Dev(BuildCall& bc, size_t bytes) { bc.wanted.push_back({&p, bytes}); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  operator T*() const { return static_cast<T*>(p); }

 private:
  void* p = nullptr;
};

// figures of the calling thread's last call of an operator, readable after the call (the *_last_* queries)
template <typename T, int N>
struct LastFigures {
  T v[N];
  int have;   // 0: the last call failed (or there was none); else what the operator publishes with its figures
  int publish(const T* src, int have_) {   // the last step of a call that succeeded
    for (int i = 0; i < N; ++i) v[i] = src[i];
    have = have_;
    return FP_OK;
  }
  int read(T* out, int cap) const {
    for (int i = 0; i < std::min(cap, N); ++i) out[i] = v[i];
    return have;
  }
};
}   // namespace

// dims of the nearest-centroid assignment (fp_index_ops.hip): [1, 256], and every multiple of 8 up to 1024
static bool assign_dim_accepted(int32_t dim) { return dim >= 1 && (dim <= 256 || (dim <= 1024 && dim % 8 == 0)); }
// what fpk_km_scan_data leaves: the largest (bits & 0x7FFF) of the fp16 values it read; an infinity or a NaN is 0x7C00 or more
static bool holds_non_finite(uint32_t max_abs_bits) { return max_abs_bits >= 0x7C00u; }

// ------------------------------------------------------------------------------------------
// index creation, device part (create.rs:148-184, :404-428)
// ------------------------------------------------------------------------------------------
enum { CP_CHUNKS, CP_NARROWED, CP_FALLBACK, CP_US_ASSIGN, CP_US_PACK, CP_CAND_SUM, CP_CAND_MAX, CP_N };
static thread_local LastFigures<int64_t, CP_N> g_cp;   // have = 1: the figures are those of a call that succeeded
extern "C" int fp_compress_last_counts(int64_t* out, int cap) {
  if (!out || cap < 0) return 0;
  return g_cp.read(out, cap);
}

extern "C" int fp_compress(int device_id, const uint16_t* centroids, int64_t C, int32_t dim, int32_t nbits, const uint16_t* cutoffs,
                           const uint16_t* emb, int64_t T, int64_t* out_codes, uint8_t* out_res) {
  g_cp = {};
  if (!centroids || !cutoffs || C < 1 || T < 0 || (T > 0 && (!emb || !out_codes || !out_res))) return fp_fail(FP_EINVAL, "bad argument");
  if (!(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8)) return fp_fail(FP_EINVAL, "nbits must divide 8 (1, 2, 4 or 8)");
  if (!assign_dim_accepted(dim) || (dim * nbits) % 8 != 0)
    return fp_fail(FP_EUNSUPPORTED, "fp_compress: dim must be in [1, 256] or a multiple of 8 up to 1024, with dim * nbits a multiple of 8");
  if (C >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "too many centroids");
  BuildCall bc("fp_compress", false);
  if (int rc = bc.open(device_id)) return rc;
  int64_t cp[CP_N] = {0, 0, 0, 0, 0, 0, 0};
  if (T == 0) return g_cp.publish(cp, 1);
  const int pr = dim * nbits / 8;
  const int64_t CHUNK = 1ll << 20;   // tokens per pass
  const int64_t cap = std::min<int64_t>(T, CHUNK);
  float cmaxabs = 0.f;   // bounds the MFMA summation error in the assignment (fp16 -> float by hand: no device needed)
  for (int64_t i = 0; i < C * dim; ++i) {
    const uint16_t hbits = centroids[i] & 0x7FFF;
    const int ex = hbits >> 10, ma = hbits & 0x3FF;
    const float v = ex == 0 ? std::ldexp((float)ma, -24) : (ex == 31 ? INFINITY : std::ldexp((float)(ma | 0x400), ex - 25));
    if (v > cmaxabs) cmaxabs = v;
  }
  Dev<uint16_t> d_cent(bc, (size_t)C * dim * 2), d_cut(bc, 1024);   // up to 255 cutoffs (nbits = 8)
  Dev<uint16_t> d_emb(bc, (size_t)cap * dim * 2);
  Dev<int32_t> d_c32(bc, (size_t)cap * 4);
  Dev<int64_t> d_c64(bc, (size_t)cap * 8);
  Dev<uint8_t> d_out(bc, (size_t)cap * pr);
  Dev<void> d_work(bc, fpk_compress_work_bytes(cap));
  BCHK(hipStreamCreateWithFlags(&bc.st, hipStreamNonBlocking));
  BCHK(bc.create_events(3));
  BCHK(bc.hip_malloc_all());
  hipStream_t st = bc.st;
  BCHK(hipMemcpyAsync(d_cent, centroids, (size_t)C * dim * 2, hipMemcpyHostToDevice, st));
  BCHK(hipMemcpyAsync(d_cut, cutoffs, (size_t)((1 << nbits) - 1) * 2, hipMemcpyHostToDevice, st));
  for (int64_t t0 = 0; t0 < T; t0 += CHUNK) {
    const int64_t n = std::min<int64_t>(CHUNK, T - t0);
    BCHK(hipMemcpyAsync(d_emb, emb + t0 * dim, (size_t)n * dim * 2, hipMemcpyHostToDevice, st));
    int64_t how[4] = {0, 0, 0, 0};
    if (fpk_compress(d_emb, n, d_cent, C, dim, nbits, d_cut, cmaxabs, d_c32, d_c64, d_out, d_work, st, how, bc.ev.data()))
      return fp_fail(FP_EUNSUPPORTED, "dim");
    BCHK(hipMemcpyAsync(out_codes + t0, d_c64, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(out_res + t0 * pr, d_out, (size_t)n * pr, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    ++cp[CP_CHUNKS];
    cp[CP_NARROWED] += how[0];
    cp[CP_FALLBACK] += how[1];
    cp[CP_CAND_SUM] += how[2];
    cp[CP_CAND_MAX] = std::max(cp[CP_CAND_MAX], how[3]);
    BCHK(bc.add_elapsed_us(&cp[CP_US_ASSIGN], 2));
  }
  return g_cp.publish(cp, 1);
}

extern "C" int fp_assign_l2(int device_id, const uint16_t* centroids, const float* half_sqnorm, int64_t C, int32_t dim, const uint16_t* emb,
                            int64_t T, int64_t* out_labels) {
  if (!centroids || !half_sqnorm || C < 1 || T < 0 || (T > 0 && (!emb || !out_labels))) return fp_fail(FP_EINVAL, "bad argument");
  if (!assign_dim_accepted(dim)) return fp_fail(FP_EUNSUPPORTED, "fp_assign_l2: dim must be in [1, 256] or a multiple of 8 up to 1024");
  if (C >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "too many centroids");
  BuildCall bc("fp_assign_l2", false);
  if (int rc = bc.open(device_id)) return rc;
  if (T == 0) return FP_OK;
  const int64_t CHUNK = 1ll << 20;
  const int64_t cap = std::min<int64_t>(T, CHUNK);
  Dev<uint16_t> d_cent(bc, (size_t)C * dim * 2);
  Dev<float> d_hn(bc, (size_t)C * 4);
  Dev<uint16_t> d_emb(bc, (size_t)cap * dim * 2);
  Dev<int32_t> d_c32(bc, (size_t)cap * 4);
  Dev<int64_t> d_c64(bc, (size_t)cap * 8);
  BCHK(hipStreamCreateWithFlags(&bc.st, hipStreamNonBlocking));
  BCHK(bc.hip_malloc_all());
  hipStream_t st = bc.st;
  BCHK(hipMemcpyAsync(d_cent, centroids, (size_t)C * dim * 2, hipMemcpyHostToDevice, st));
  BCHK(hipMemcpyAsync(d_hn, half_sqnorm, (size_t)C * 4, hipMemcpyHostToDevice, st));
  for (int64_t t0 = 0; t0 < T; t0 += CHUNK) {
    const int64_t n = std::min<int64_t>(CHUNK, T - t0);
    BCHK(hipMemcpyAsync(d_emb, emb + t0 * dim, (size_t)n * dim * 2, hipMemcpyHostToDevice, st));
    if (fpk_assign_l2(d_emb, n, d_cent, d_hn, C, dim, d_c32, d_c64, st)) return fp_fail(FP_EUNSUPPORTED, "dim");
    BCHK(hipMemcpyAsync(out_labels + t0, d_c64, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
  }
  return FP_OK;
}

// k-means trainer (fastplaid.h fp_kmeans): the sample goes up once, every Lloyd iteration runs on the device; per iteration only the
// chunks' overflow counters of the MFMA narrowing come back (a chunk with a non-zero counter is assigned again by the exact kernel).
enum { KM_UPLOAD, KM_ASSIGN, KM_INDEX, KM_SUM, KM_FINALISE, KM_NARROWED, KM_FALLBACK, KM_N };   // five times, two chunk counts
static thread_local LastFigures<float, KM_N> g_km;   // have = iterations the figures of the last call cover (0: none)
extern "C" int fp_kmeans_last_timings(float* ms, int cap) { return g_km.read(ms, cap); }

extern "C" int fp_kmeans(int device_id, const uint16_t* data, int64_t n, int32_t dim, int64_t k, int32_t niter, const int64_t* init_rows,
                         uint64_t seed, float* out_centroids, int64_t* out_counts) {
  g_km.have = 0;
  if (!data || !init_rows || !out_centroids || n < 1 || k < 1 || niter < 0) return fp_fail(FP_EINVAL, "bad argument");
  if (!assign_dim_accepted(dim)) return fp_fail(FP_EUNSUPPORTED, "fp_kmeans: dim must be in [1, 256] or a multiple of 8 up to 1024");
  if (k > n) return fp_fail(FP_EINVAL, "fp_kmeans: fewer training points (" + std::to_string(n) + ") than centroids (" + std::to_string(k) + ")");
  if (n >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "fp_kmeans: more than 2^31-2 training points");
  for (int64_t c = 0; c < k; ++c)
    if (init_rows[c] < 0 || init_rows[c] >= n) return fp_fail(FP_EINVAL, "fp_kmeans: init_rows[" + std::to_string(c) + "] outside [0, n)");
  BuildCall bc("fp_kmeans", true);
  if (int rc = bc.open(device_id)) return rc;
  const int64_t chunk_opt = (int64_t)fp_test_opt("kmeans_chunk", 0);   // tests: a chunk boundary inside a few thousand points
  const int64_t CHUNK = std::min<int64_t>(n, chunk_opt > 0 ? chunk_opt : (1ll << 20));
  const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
  const bool timed = niter > 0 && niter <= 64;
  const size_t kd = (size_t)k * dim;
  Dev<uint16_t> d_data(bc, (size_t)n * dim * 2);
  Dev<int64_t> d_init(bc, (size_t)k * 8);
  Dev<int32_t> labels(bc, (size_t)n * 4), d_mem(bc, (size_t)n * 4);
  Dev<float> d_c32(bc, kd * 4);
  Dev<uint16_t> d_c16(bc, kd * 2);
  Dev<float> d_hn(bc, (size_t)k * 4);
  Dev<int64_t> d_sums(bc, kd * 8);
  Dev<int32_t> d_cnt(bc, (size_t)k * 4), d_cur(bc, (size_t)k * 4);
  Dev<int64_t> d_cnt64(bc, (size_t)k * 8);
  Dev<void> d_work(bc, fpk_compress_work_bytes(CHUNK));
  Dev<int32_t> d_over(bc, (size_t)nchunk * 4);
  Dev<uint32_t> stat(bc, 64);   // [0..1] {max|cent16|, max hn} of the iteration, [4] max |x| bits of the data
  const size_t need = bc.footprint();
  size_t mfree = 0, mtotal = 0;
  BCHK(hipMemGetInfo(&mfree, &mtotal));
  if (need > mfree)
    return fp_fail(FP_ENOMEM, "fp_kmeans: the sample and its work buffers need " + std::to_string(need) + " bytes of device memory, " +
                                  std::to_string(mfree) + " are free");
  BCHK(hipStreamCreateWithFlags(&bc.st, hipStreamNonBlocking));
  BCHK(bc.hip_malloc_all());
  if (timed) BCHK(bc.create_events(2 + 5 * (size_t)niter));   // 2 around the upload, 5 per iteration
  hipStream_t st = bc.st;
  std::vector<hipEvent_t>& ev = bc.ev;
  if (timed) BCHK(hipEventRecord(ev[0], st));
  BCHK(hipMemsetAsync(stat, 0, 64, st));
  BCHK(hipMemcpyAsync(d_data, data, (size_t)n * dim * 2, hipMemcpyHostToDevice, st));
  BCHK(hipMemcpyAsync(d_init, init_rows, (size_t)k * 8, hipMemcpyHostToDevice, st));
  fpk_km_scan_data(d_data, n * dim, stat + 4, st);
  uint32_t h_xmax = 0;
  BCHK(hipMemcpyAsync(&h_xmax, stat + 4, 4, hipMemcpyDeviceToHost, st));
  if (timed) BCHK(hipEventRecord(ev[1], st));
  BCHK(hipStreamSynchronize(st));
  BCHK(hipGetLastError());
  if (holds_non_finite(h_xmax)) return fp_fail(FP_EINVAL, "fp_kmeans: the data holds a value that is not finite");
  // exact sums in int64 units of 2^-24: refuse what could leave 2^62
  if ((unsigned __int128)n * (unsigned __int128)fp_f16_fixed((uint16_t)h_xmax) >= ((unsigned __int128)1 << 62))
    return fp_fail(FP_EUNSUPPORTED, "fp_kmeans: n * max|x| * 2^24 >= 2^62 (the exact fixed-point sums could overflow)");
  fpk_km_finalise(d_data, n, dim, k, d_init, nullptr, nullptr, seed, 0, d_c32, d_c16, d_hn, stat, st);
  std::vector<int32_t> h_over((size_t)nchunk, 0);
  int64_t n_narrowed = 0, n_fallback = 0;   // chunk assignments through the MFMA narrowing / of those, sent on to the exact kernel
  for (int it = 0; it < niter; ++it) {
    hipEvent_t* e = timed ? &ev[2 + 5 * (size_t)it] : nullptr;
    if (e) BCHK(hipEventRecord(e[0], st));
    BCHK(hipMemsetAsync(d_over, 0, (size_t)nchunk * 4, st));
    bool narrowed = false;
    for (int64_t ci = 0; ci < nchunk; ++ci) {
      const int64_t t0 = ci * CHUNK, nn = std::min<int64_t>(CHUNK, n - t0);
      const int rc = fpk_assign_l2_narrow(d_data + t0 * dim, nn, d_c16, d_hn, stat, k, dim, labels + t0, d_work, d_over + ci, st);
      if (rc < 0) return fp_fail(FP_EUNSUPPORTED, "fp_kmeans: assignment chunk (" + std::to_string(rc) + ")");
      narrowed |= rc == 1;
      n_narrowed += rc == 1;
    }
    if (narrowed) {   // the fallback flags: the only thing that returns to the host between iterations
      BCHK(hipMemcpyAsync(h_over.data(), d_over, (size_t)nchunk * 4, hipMemcpyDeviceToHost, st));
      BCHK(hipStreamSynchronize(st));
      for (int64_t ci = 0; ci < nchunk; ++ci) {
        if (h_over[(size_t)ci] == 0) continue;   // else: a point met more than ASSIGN_CAP near-tied centroids
        ++n_fallback;
        const int64_t t0 = ci * CHUNK, nn = std::min<int64_t>(CHUNK, n - t0);
        if (fpk_assign_l2_exact(d_data + t0 * dim, nn, d_c16, d_hn, k, dim, labels + t0, st))
          return fp_fail(FP_EUNSUPPORTED, "fp_kmeans: assignment chunk");
      }
    }
    if (e) BCHK(hipEventRecord(e[1], st));
    fpk_km_index(labels, n, k, d_cnt, d_cur, d_mem, st);
    if (e) BCHK(hipEventRecord(e[2], st));
    fpk_km_sum(d_data, n, dim, k, labels, d_mem, d_sums, st);
    if (e) BCHK(hipEventRecord(e[3], st));
    fpk_km_finalise(d_data, n, dim, k, nullptr, d_sums, d_cnt, seed, it, d_c32, d_c16, d_hn, stat, st);
    if (e) BCHK(hipEventRecord(e[4], st));
    BCHK(hipGetLastError());
  }
  BCHK(hipMemcpyAsync(out_centroids, d_c32, kd * 4, hipMemcpyDeviceToHost, st));
  if (out_counts) {
    if (niter > 0) {
      fpk_km_widen_counts(d_cnt, d_cnt64, k, st);
      BCHK(hipMemcpyAsync(out_counts, d_cnt64, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    } else {
      memset(out_counts, 0, (size_t)k * 8);
    }
  }
  BCHK(hipStreamSynchronize(st));
  BCHK(hipGetLastError());
  if (timed) {
    float ms[KM_N] = {0.f, 0.f, 0.f, 0.f, 0.f, (float)n_narrowed, (float)n_fallback}, x = 0.f;
    BCHK(hipEventElapsedTime(&ms[KM_UPLOAD], ev[0], ev[1]));
    for (int it = 0; it < niter; ++it)
      for (int s = 0; s < 4; ++s) {
        BCHK(hipEventElapsedTime(&x, ev[2 + 5 * (size_t)it + s], ev[3 + 5 * (size_t)it + s]));
        ms[KM_ASSIGN + s] += x;
      }
    g_km.publish(ms, niter);
  }
  return FP_OK;
}

// Outliers of a centroid table (fastplaid.h fp_centroid_outliers): the centroids go up once, the embeddings in chunks; per chunk
// the overflow counter of the MFMA narrowing, the data check and the outlier count come back, then that many rows.
enum { CO_CHUNKS, CO_NARROWED, CO_FALLBACK, CO_US_UPLOAD, CO_US_ASSIGN, CO_US_OUTLIER, CO_US_DOWNLOAD, CO_N };
static thread_local LastFigures<int64_t, CO_N> g_co;   // have = 1: the figures are those of a call that succeeded
extern "C" int fp_centroid_outliers_last_counts(int64_t* out, int cap) { return g_co.read(out, cap); }

extern "C" int fp_centroid_outliers(int device_id, const uint16_t* centroids, int64_t C, int32_t dim, const uint16_t* emb, int64_t T,
                                    float threshold_sq, int64_t* out_rows, int64_t* out_count, float* out_sqdist, int64_t* out_nearest) {
  g_co.have = 0;
  if (!out_count) return fp_fail(FP_EINVAL, "bad argument");
  *out_count = 0;
  if (!centroids || C < 1 || T < 0 || (T > 0 && (!emb || !out_rows))) return fp_fail(FP_EINVAL, "bad argument");
  if (!(threshold_sq >= 0.f)) return fp_fail(FP_EINVAL, "fp_centroid_outliers: threshold_sq must be a number >= 0");
  if (!assign_dim_accepted(dim))
    return fp_fail(FP_EUNSUPPORTED, "fp_centroid_outliers: dim must be in [1, 256] or a multiple of 8 up to 1024");
  if (C >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "too many centroids");
  BuildCall bc("fp_centroid_outliers", true);
  if (int rc = bc.open(device_id)) return rc;
  int64_t co[CO_N] = {0, 0, 0, 0, 0, 0, 0};
  if (T == 0) return g_co.publish(co, 1);
  const int64_t chunk_opt = (int64_t)fp_test_opt("outlier_chunk", 0);   // tests: chunk boundaries inside a few thousand tokens
  const int64_t CHUNK = std::min<int64_t>(T, chunk_opt > 0 ? chunk_opt : (1ll << 20));
  const size_t ntile = fpk_outliers_tiles(CHUNK);
  Dev<uint16_t> d_cent(bc, (size_t)C * dim * 2);
  Dev<float> d_hn(bc, (size_t)C * 4);
  Dev<uint16_t> d_emb(bc, (size_t)CHUNK * dim * 2);
  Dev<int32_t> labels(bc, (size_t)CHUNK * 4);
  Dev<float> d_sq(bc, (size_t)CHUNK * 4);
  Dev<int64_t> d_near(bc, out_nearest ? (size_t)CHUNK * 8 : 0);
  Dev<uint8_t> d_flag(bc, (size_t)CHUNK);
  Dev<int32_t> d_tcnt(bc, ntile * 4), d_toff(bc, ntile * 4);
  Dev<int64_t> d_rows(bc, (size_t)CHUNK * 8);
  Dev<void> d_work(bc, fpk_compress_work_bytes(CHUNK));
  // stat: [0..1] {max|cent|, max hn} (k_assign_thr_l2's input), [4] max |x| bits of the centroids, then of the embeddings so far,
  // [8] the chunk's overflow counter, [9] its outlier count
  Dev<uint32_t> stat(bc, 64);
  BCHK(hipStreamCreateWithFlags(&bc.st, hipStreamNonBlocking));
  BCHK(bc.hip_malloc_all());
  BCHK(bc.create_events(5));
  hipStream_t st = bc.st;
  std::vector<hipEvent_t>& ev = bc.ev;
  BCHK(hipMemsetAsync(stat, 0, 64, st));
  BCHK(hipMemcpyAsync(d_cent, centroids, (size_t)C * dim * 2, hipMemcpyHostToDevice, st));
  fpk_km_scan_data(d_cent, C * dim, stat + 4, st);
  fpk_out_prepare(d_cent, C, dim, d_hn, stat, st);
  uint32_t h_max = 0;
  BCHK(hipMemcpyAsync(&h_max, stat + 4, 4, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  BCHK(hipGetLastError());
  if (holds_non_finite(h_max)) return fp_fail(FP_EINVAL, "fp_centroid_outliers: the centroids hold a value that is not finite");
  int64_t total = 0;
  for (int64_t t0 = 0; t0 < T; t0 += CHUNK) {
    const int64_t n = std::min<int64_t>(CHUNK, T - t0);
    BCHK(hipEventRecord(ev[0], st));
    BCHK(hipMemcpyAsync(d_emb, emb + t0 * dim, (size_t)n * dim * 2, hipMemcpyHostToDevice, st));
    fpk_km_scan_data(d_emb, n * dim, stat + 4, st);
    BCHK(hipEventRecord(ev[1], st));
    const int rc = fpk_assign_l2_narrow(d_emb, n, d_cent, d_hn, stat, C, dim, labels, d_work, reinterpret_cast<int32_t*>(stat + 8), st);
    if (rc < 0) return fp_fail(FP_EUNSUPPORTED, "fp_centroid_outliers: assignment chunk (" + std::to_string(rc) + ")");
    uint32_t h_chk[5] = {0, 0, 0, 0, 0};   // [0] max |x| bits, [4] overflow counter (zero when the chunk did not take the narrowing)
    BCHK(hipMemcpyAsync(h_chk, stat + 4, sizeof(h_chk), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    if (holds_non_finite(h_chk[0])) return fp_fail(FP_EINVAL, "fp_centroid_outliers: the embeddings hold a value that is not finite");
    ++co[CO_CHUNKS];
    co[CO_NARROWED] += rc == 1;
    if (rc == 1 && h_chk[4] != 0) {   // a token met more than ASSIGN_CAP near-tied centroids: the whole chunk goes through the exact kernel
      ++co[CO_FALLBACK];
      if (fpk_assign_l2_exact(d_emb, n, d_cent, d_hn, C, dim, labels, st)) return fp_fail(FP_EUNSUPPORTED, "fp_centroid_outliers: assignment chunk");
    }
    BCHK(hipEventRecord(ev[2], st));
    fpk_outliers_chunk(d_emb, n, t0, d_cent, C, dim, d_hn, labels, threshold_sq, d_sq, d_near, d_flag, d_tcnt, d_toff,
                       reinterpret_cast<int32_t*>(stat + 9), d_rows, st);
    BCHK(hipEventRecord(ev[3], st));
    int32_t h_cnt = 0;
    BCHK(hipMemcpyAsync(&h_cnt, stat + 9, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    BCHK(hipGetLastError());
    if (h_cnt < 0 || h_cnt > n) return fp_fail(FP_EHIP, "fp_centroid_outliers: outlier count outside the chunk");
    if (h_cnt > 0) BCHK(hipMemcpyAsync(out_rows + total, d_rows, (size_t)h_cnt * 8, hipMemcpyDeviceToHost, st));
    if (out_sqdist) BCHK(hipMemcpyAsync(out_sqdist + t0, d_sq, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (out_nearest) BCHK(hipMemcpyAsync(out_nearest + t0, d_near, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    BCHK(hipEventRecord(ev[4], st));
    BCHK(hipStreamSynchronize(st));
    total += h_cnt;
    BCHK(bc.add_elapsed_us(&co[CO_US_UPLOAD], 4));
  }
  *out_count = total;
  return g_co.publish(co, 1);
}

// Residual statistics for codec training (fastplaid.h fp_residual_stats): fp_compress's plan with the packing replaced by the
// residual kernels of fp_codec_stats.hip.  The histogram and the per-dim sums stay on the device across the chunks and come back
// once; codes and norms come back per chunk.
extern "C" int fp_residual_stats(int device_id, const uint16_t* centroids, int64_t C, int32_t dim, const uint16_t* emb, int64_t T,
                                 int64_t* out_codes, int64_t* out_hist, int64_t* out_abs_sum, float* out_norms) {
  if (!centroids || !out_hist || !out_abs_sum || C < 1 || T < 0 || (T > 0 && !emb)) return fp_fail(FP_EINVAL, "bad argument");
  if (!assign_dim_accepted(dim)) return fp_fail(FP_EUNSUPPORTED, "fp_residual_stats: dim must be in [1, 256] or a multiple of 8 up to 1024");
  if (C >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "too many centroids");
  BuildCall bc("fp_residual_stats", false);
  if (int rc = bc.open(device_id)) return rc;
  memset(out_hist, 0, 65536 * sizeof(int64_t));
  memset(out_abs_sum, 0, (size_t)dim * sizeof(int64_t));
  if (T == 0) return FP_OK;
  const int64_t CHUNK = 1ll << 20;   // tokens per pass: at most 2^30 residuals, the bound of one fpk_hist16 launch
  const int64_t cap = std::min<int64_t>(T, CHUNK);
  Dev<uint16_t> d_cent(bc, (size_t)C * dim * 2);
  Dev<uint16_t> d_emb(bc, (size_t)cap * dim * 2), d_res(bc, (size_t)cap * dim * 2);
  Dev<int32_t> d_c32(bc, (size_t)cap * 4);
  Dev<int64_t> d_c64(bc, out_codes ? (size_t)cap * 8 : 0);
  Dev<float> d_norm(bc, out_norms ? (size_t)cap * 4 : 0);
  Dev<int64_t> d_hist(bc, 65536 * 8), d_abs(bc, (size_t)dim * 8);
  Dev<void> d_work(bc, fpk_compress_work_bytes(cap));
  Dev<uint32_t> stat(bc, 64);   // [0] max |x| bits of the centroids, [1] of the embeddings so far
  BCHK(hipStreamCreateWithFlags(&bc.st, hipStreamNonBlocking));
  BCHK(bc.hip_malloc_all());
  hipStream_t st = bc.st;
  BCHK(hipMemsetAsync(stat, 0, 64, st));
  BCHK(hipMemsetAsync(d_hist, 0, 65536 * 8, st));
  BCHK(hipMemsetAsync(d_abs, 0, (size_t)dim * 8, st));
  BCHK(hipMemcpyAsync(d_cent, centroids, (size_t)C * dim * 2, hipMemcpyHostToDevice, st));
  fpk_km_scan_data(d_cent, C * dim, stat, st);
  uint32_t h_max[2] = {0, 0};
  BCHK(hipMemcpyAsync(h_max, stat, 4, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  BCHK(hipGetLastError());
  if (holds_non_finite(h_max[0])) return fp_fail(FP_EINVAL, "fp_residual_stats: the centroids hold a value that is not finite");
  // max |centroid element| bounds the MFMA summation error in the assignment: the value fp_compress takes on the host
  const float cmaxabs = std::ldexp((float)fp_f16_fixed((uint16_t)h_max[0]), -24);
  for (int64_t t0 = 0; t0 < T; t0 += CHUNK) {
    const int64_t n = std::min<int64_t>(CHUNK, T - t0);
    BCHK(hipMemcpyAsync(d_emb, emb + t0 * dim, (size_t)n * dim * 2, hipMemcpyHostToDevice, st));
    fpk_km_scan_data(d_emb, n * dim, stat + 1, st);
    BCHK(hipMemcpyAsync(h_max + 1, stat + 1, 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    BCHK(hipGetLastError());
    if (holds_non_finite(h_max[1])) return fp_fail(FP_EINVAL, "fp_residual_stats: the embeddings hold a value that is not finite");
    // exact sums in int64 units of 2^-24, |r| <= |x| + |c|: refuse what could leave 2^62 (the maximum so far only grows, so the
    // last chunk decides with the maximum over all the data)
    const unsigned __int128 reach = (unsigned __int128)fp_f16_fixed((uint16_t)h_max[0]) + (unsigned __int128)fp_f16_fixed((uint16_t)h_max[1]);
    if ((unsigned __int128)T * reach >= ((unsigned __int128)1 << 62))
      return fp_fail(FP_EUNSUPPORTED, "fp_residual_stats: n_tokens * (max|x| + max|c|) * 2^24 >= 2^62 (the exact fixed-point sums could overflow)");
    if (int rc = fpk_assign_codes(d_emb, n, d_cent, C, dim, cmaxabs, d_c32, d_work, st))
      return rc == -3 ? bc.hip_failed(hipGetLastError(), "fpk_assign_codes") : fp_fail(FP_EUNSUPPORTED, "fp_residual_stats: assignment chunk (" + std::to_string(rc) + ")");
    fpk_residual_tile(d_emb, n, d_cent, C, dim, d_c32, d_res, d_abs, d_norm, d_c64, st);
    if (int rc = fpk_hist16(d_res, n * dim, d_hist, st))
      return rc == -3 ? bc.hip_failed(hipGetLastError(), "fpk_hist16") : fp_fail(FP_EUNSUPPORTED, "fp_residual_stats: histogram chunk (" + std::to_string(rc) + ")");
    if (out_codes) BCHK(hipMemcpyAsync(out_codes + t0, d_c64, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (out_norms) BCHK(hipMemcpyAsync(out_norms + t0, d_norm, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    BCHK(hipGetLastError());
  }
  BCHK(hipMemcpyAsync(out_hist, d_hist, 65536 * 8, hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(out_abs_sum, d_abs, (size_t)dim * 8, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  BCHK(hipGetLastError());
  if (out_hist[0x7C00] != 0 || out_hist[0xFC00] != 0) return fp_fail(FP_EINVAL, "fp_residual_stats: a residual overflows fp16");
  return FP_OK;
}
