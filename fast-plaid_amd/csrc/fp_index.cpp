// The life of an fp_index (include/fastplaid.h): construction from host arrays (load.rs:124-186: upload + re-layout) or as a
// synthetic device-generated corpus, destruction, the getters, and the read-back of its arrays (fp_index_read_doc,
// fp_index_read_ivf, fp_index_ivf_total, fp_index_export).  Host code only: the kernels are behind the fpk_* / fps_* launchers of
// fp_internal.h.  Who frees what: the index its device buffers and pooled scratches (~fp_index), an IndexBuild the construction
// stream and the index until it is handed over, a DevTmp one step's temporary.  No path frees by hand.
#include "../../include/fastplaid.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fp_host.h"

// ------------------------------------------------------------------------------------------
// ownership
// ------------------------------------------------------------------------------------------
template <typename T>
hipError_t fp_index::alloc(T** p, size_t alloc_bytes, int64_t counted) {
  void* q = nullptr;
  const hipError_t e = hipMalloc(&q, alloc_bytes);
  if (e == hipSuccess) *p = adopt(static_cast<T*>(q), counted);
  return e;
}
template <typename T>
T* fp_index::adopt(T* p, int64_t counted) {
  if (p) {
    owned.push_back(static_cast<void*>(p));
    bytes += counted;
  }
  return p;
}
fp_index::~fp_index() {
  (void)fp_set_device(device);
  for (Scratch* s : pool) fp_delete_scratch(s);
  for (void* p : owned) (void)hipFree(p);
}
extern "C" void fp_index_destroy(fp_index* ix) { delete ix; }

// n entries (at least one) with 64 bytes of slack behind them -- vector loads may touch past the end -- all of it counted
template <typename T>
static hipError_t dev_alloc(fp_index* ix, T** p, size_t n) {
  const size_t bytes = (n ? n : 1) * sizeof(T) + 64;
  return ix->alloc(p, bytes, (int64_t)bytes);
}

namespace {   // (the types of this file stay out of the library's symbol table)
// a device temporary of one construction step: freed on every way out of its scope
struct DevTmp {
  void* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

// one index construction: the index until it is handed over, and the stream everything is enqueued on.  A creator that returns
// early (HIPCHK, LCHK, a refusal) leaves the index to ~IndexBuild, which frees what was built so far.
struct IndexBuild {
  std::unique_ptr<fp_index> ix;
  hipStream_t st = nullptr;
  explicit IndexBuild(int device) : ix(new fp_index()) { ix->device = device; }
  ~IndexBuild() {
    ix.reset();
    if (st) (void)hipStreamDestroy(st);
  }
  int open(const uint16_t* centroids, const uint16_t* bucket_weights, int32_t** codes, uint8_t** residuals);
  int hand_over(fp_index** out) {
    HIPCHK(hipStreamSynchronize(st));
    prepay_legacy_stream();
    *out = ix.release();
    return FP_OK;
  }
};
}   // namespace

// a HIP failure of a named step of finish_layout ends it: LCHK("token norms", hipStreamSynchronize(st))
static int step_failed(hipError_t e, const char* step) {
  return fp_fail(FP_EHIP, std::string("HIP error: ") + hipGetErrorString(e) + " (" + step + ")");
}
#define LCHK(step, x)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return step_failed(e_, step);                                                \
  } while (0)

// ------------------------------------------------------------------------------------------
// index construction (load.rs:124-186)
// ------------------------------------------------------------------------------------------
static void build_lut_host(int nbits, const uint16_t* weights, std::vector<uint16_t>& lut) {
  // residual_codec.rs:83-140 folded: byte -> rev_map -> idx_lookup[rev][j] -> weights
  const int per = 8 / nbits, mask = (1 << nbits) - 1;
  lut.assign((size_t)256 * per, 0);
  for (int v = 0; v < 256; ++v) {
    unsigned out = 0;
    int pos = 8;
    while (pos >= nbits) {
      unsigned seg = ((unsigned)v >> (pos - nbits)) & (unsigned)mask, rev = 0;
      for (int k = 0; k < nbits; ++k)
        if (seg & (1u << k)) rev |= 1u << (nbits - 1 - k);
      out |= rev;
      if (pos > nbits) out <<= nbits;
      pos -= nbits;
    }
    out &= 0xFF;
    int j = 0;
    for (int k = per - 1; k >= 0; --k) lut[(size_t)v * per + j++] = weights[(out >> (k * nbits)) & mask];
  }
}

// largest row norm of an fp16 matrix (never below 1): the rounding noise of a score's fp32 chain scales with |c| |q|
static float max_row_norm_f16(const uint16_t* m, int64_t rows, int dim) {
  double best = 1.0;
  for (int64_t r = 0; r < rows; ++r) {
    double ss = 0.0;
    const uint16_t* row = m + r * dim;
    for (int k = 0; k < dim; ++k) {
      const double x = (double)(float)__builtin_bit_cast(_Float16, row[k]);
      ss += x * x;
    }
    if (ss > best * best) best = std::sqrt(ss);
  }
  return (float)best;
}

// limit > 0: every entry must lie in [0, limit) -- `what` names the array in the error (the reference fails on such an index
// inside index_select, per query; a code that is no centroid or a list entry that is no document would be an out-of-bounds
// read on the device here, so the index is refused when it is built)
static int upload_narrow(const int64_t* host, int32_t* dev, int64_t n, hipStream_t st, int64_t limit = 0, const char* what = "") {
  // chunked i64 -> i32 through a device staging buffer
  if (n <= 0) return FP_OK;
  const int64_t chunk = 32ll << 20;  // 32M entries = 256 MiB
  DevTmp stage;
  const size_t stage_bytes = (size_t)std::min(chunk, n) * 8;
  HIPCHK(stage.alloc(stage_bytes + 8));
  uint32_t* bad = limit > 0 ? reinterpret_cast<uint32_t*>(stage.as<char>() + stage_bytes) : nullptr;
  uint32_t h_bad = 0;
  hipError_t e = bad ? hipMemsetAsync(bad, 0, 4, st) : hipSuccess;
  for (int64_t s = 0; s < n && e == hipSuccess; s += chunk) {
    int64_t m = std::min(chunk, n - s);
    e = hipMemcpyAsync(stage.p, host + s, (size_t)m * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) break;
    fpk_narrow_i64_i32(stage.as<int64_t>(), dev + s, m, 0, st, limit, bad);
    e = hipStreamSynchronize(st);
  }
  if (e == hipSuccess && bad) e = copy_sync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return fp_fail(FP_EHIP, hipGetErrorString(e));
  if (h_bad) return fp_fail(FP_EINVAL, std::string(what) + ": " + std::to_string(h_bad) + " entries outside [0, " + std::to_string(limit) + ")");
  return FP_OK;
}

// residual_codec.rs:83-140 / search.rs:53-107 are generic in nbits (a divisor of 8) and dim; the centroid GEMM stages K in
// 8-dim (16-byte) pieces, hence dim % 8.  Every accepted shape has an MFMA MaxSim kernel: fixed-dim ones for thirteen shapes
// (k_maxsim6 / k_maxsim5), the K-sliced k_maxsim_sl at a runtime dim for the rest.
static int check_shape(int nbits, int dim) {
  if (!(nbits == 1 || nbits == 2 || nbits == 4 || nbits == 8)) return fp_fail(FP_EINVAL, "nbits must divide 8 (1, 2, 4 or 8)");
  if (dim < 8 || dim % 8 != 0 || dim > 1024) return fp_fail(FP_EUNSUPPORTED, "dim must be a multiple of 8 in [8, 1024]");
  return FP_OK;
}

// What both creators start with, once d.{nbits, dim, pr, C, N, T} and h_doc_off are set: the construction stream, the centroids
// (and their largest norm), the LUT and the document offsets on the device, codes and residuals allocated.
int IndexBuild::open(const uint16_t* centroids, const uint16_t* bucket_weights, int32_t** codes, uint8_t** residuals) {
  FpIndexDev& D = ix->d;
  uint16_t* cent = nullptr; uint16_t* lut = nullptr; int64_t* doc_off = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  HIPCHK(dev_alloc(ix.get(), &cent, (size_t)D.C * D.dim));
  HIPCHK(copy_sync(cent, centroids, (size_t)D.C * D.dim * 2, hipMemcpyHostToDevice, st));
  ix->cent_norm_max = max_row_norm_f16(centroids, D.C, D.dim);
  std::vector<uint16_t> hlut;
  build_lut_host(D.nbits, bucket_weights, hlut);
  HIPCHK(dev_alloc(ix.get(), &lut, hlut.size()));
  HIPCHK(copy_sync(lut, hlut.data(), hlut.size() * 2, hipMemcpyHostToDevice, st));
  HIPCHK(dev_alloc(ix.get(), &doc_off, (size_t)D.N + 1));
  HIPCHK(copy_sync(doc_off, ix->h_doc_off.data(), ((size_t)D.N + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(dev_alloc(ix.get(), codes, (size_t)D.T));
  HIPCHK(dev_alloc(ix.get(), residuals, (size_t)D.T * D.pr));
  D.centroids = cent; D.lut = lut; D.doc_off = doc_off; D.codes = *codes; D.residuals = *residuals;
  return FP_OK;
}

// the self-test of the "last workgroup finishes the job" chains, once per device and process (fpk_ticket_selftest)
static bool device_tickets_ok(int device, hipStream_t st) {
  static std::mutex mu;
  static int state[64];   // 0 unknown, 1 ok, 2 failed
  std::lock_guard<std::mutex> g(mu);
  int& s = state[device & 63];
  if (s == 0) s = fpk_ticket_selftest(st) == 0 ? 1 : 2;
  return s == 1;
}

// common tail of index construction: tokens sorted by code inside each document, per-token norms, per-document unique codes.
// ix->d.{centroids, lut, codes, residuals, doc_off} are set and filled.
static int finish_layout(fp_index* ix, int maxlen, hipStream_t st) {
  FpIndexDev& D = ix->d;
  ix->tickets_ok = device_tickets_ok(ix->device, st);
  {
    uint16_t* perm = nullptr;
    const int src = fps_sort_docs(const_cast<int32_t*>(D.codes), const_cast<uint8_t*>(D.residuals), D.doc_off, D.N, D.T, maxlen, D.pr, &perm, st);
    D.perm = ix->adopt(perm, D.T * 2);
    if (src != 0) return fp_fail(FP_EHIP, "in-document token sort failed (hip error " + std::to_string(src) + ")");
  }
  {
    uint16_t* norms = nullptr;
    LCHK("token norms", ix->alloc(&norms, (size_t)std::max<int64_t>(D.T, 1) * 2 + 64, D.T * 2));
    fpk_token_norms(D, norms, st);
    LCHK("token norms", hipStreamSynchronize(st));
    D.norms = norms;
  }
  // S1's zero-padded view of the centroid table (FpIndexDev::cent_s1)
  D.cent_s1 = nullptr;
  D.dim_s1 = D.dim;
  if (D.dim < 256 && D.dim != 64 && D.dim != 128) {
    const int dp = D.dim < 64 ? 64 : (D.dim < 128 ? 128 : 256);
    uint16_t* cp = nullptr;
    LCHK("padded centroid table", ix->alloc(&cp, (size_t)D.C * dp * 2 + 64, D.C * dp * 2));
    LCHK("padded centroid table", hipMemsetAsync(cp, 0, (size_t)D.C * dp * 2, st));
    LCHK("padded centroid table", hipMemcpy2DAsync(cp, (size_t)dp * 2, D.centroids, (size_t)D.dim * 2, (size_t)D.dim * 2, (size_t)D.C, hipMemcpyDeviceToDevice, st));
    LCHK("padded centroid table", hipStreamSynchronize(st));
    D.cent_s1 = cp;
    D.dim_s1 = dp;
  }
  D.resid_native = 0;
  D.rinv = nullptr;
  if (fpk_maxsim6_shape(D.dim, D.nbits)) {
    // per-token reciprocals (from the rows still in the reference's byte order), then every row rewritten in the MaxSim kernel's
    // unit order IN PLACE, a slab of rows at a time through a bounded temporary
    static const bool use_rinv = fp_test_opt("ms_rinv", 1) != 0;
    if (use_rinv) {
      uint32_t* rv = nullptr;
      DevTmp nh;   // the count of hard tokens (not counted in the index's bytes)
      LCHK("token reciprocals", ix->alloc(&rv, (size_t)std::max<int64_t>(D.T, 1) * 4 + 64, D.T * 4));
      LCHK("token reciprocals", nh.alloc(8));
      (void)hipMemsetAsync(nh.p, 0, 8, st);
      fpk_token_rinv(D, rv, nh.as<unsigned long long>(), st);
      unsigned long long hard = 0;
      LCHK("token reciprocals", hipMemcpyAsync(&hard, nh.p, 8, hipMemcpyDeviceToHost, st));
      LCHK("token reciprocals", hipStreamSynchronize(st));
      D.rinv = rv;
      ix->n_hard_tokens = (int64_t)hard;
    }
    if (D.T > 0) {
      const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(D.T, (512ll << 20) / D.pr));
      DevTmp tmp;
      LCHK("native residual order", tmp.alloc((size_t)slab * D.pr));
      for (int64_t t0 = 0; t0 < D.T; t0 += slab) fpk_resid_native(D, t0, std::min<int64_t>(slab, D.T - t0), tmp.as<uint8_t>(), st);
      LCHK("native residual order", hipStreamSynchronize(st));
    }
    D.resid_native = 1;
  }
  {
    int64_t* uoff = nullptr; int32_t* ucodes = nullptr; int64_t U = 0;
    LCHK("unique-code offsets", ix->alloc(&uoff, ((size_t)D.N + 1) * 8 + 64, (D.N + 1) * 8));
    const int urc = fps_build_ucodes(D.codes, D.doc_off, D.N, maxlen, &ucodes, &U, uoff, st);
    D.ucodes = ix->adopt(ucodes, U * 4);
    if (urc != 0) return fp_fail(FP_EHIP, "unique-code build failed (hip error " + std::to_string(urc) + ")");
    D.uoff = uoff; D.U = U;
  }
  // packed code lines for S4's level 0: one set per range of 2^17 centroids (codes relative to the range), up to 2^20
  D.n_ranges = 0;
  D.n_lines = 0;
  D.l0_ppl = 8;
  // the static part of run_front's level-0 predicate (table of >= 32768 centroids, documents of <= 64 distinct codes on average;
  // FP_APPROX_IMPL=l0 forces level 0 in tests): an index that can never take level 0 does not carry the packed lines
  static const bool l0_forced = [] { const char* e2 = getenv("FP_APPROX_IMPL"); return e2 && e2[0] == 'l'; }();
  if (D.C <= 8 * (1ll << 17) && (l0_forced || (D.C * 64 >= (2ll << 20) && D.U <= 64 * D.N))) {
    const int nr = (int)((D.C + (1ll << 17) - 1) >> 17);
    // lines of 4 pieces (24 codes) when a document has few codes per range: half the lanes, half the bytes per candidate and range
    static const int ppl_env = (int)fp_test_opt("l0_ppl", 0);
    if (ppl_env == 4 || ppl_env == 8) D.l0_ppl = ppl_env;
    else if (nr > 1 && D.N > 0 && (double)D.U / ((double)D.N * nr) <= 14.0) D.l0_ppl = 4;
    // several ranges: ONE array of first lines, a document's ranges side by side (the scan then runs all ranges in one launch
    // and the lines of a document's ranges share fabric requests); the per-range arrays hold the extra lines only
    void* shared = nullptr;
    if (nr > 1) {
      const size_t sb = (size_t)D.N * nr * 16 * D.l0_ppl + 256;
      if (ix->alloc(&shared, sb, (int64_t)sb) != hipSuccess) return fp_fail(FP_EHIP, "packed-code build failed (out of memory)");
      D.n_lines += D.N * nr;
    }
    for (int r = 0; r < nr; ++r) {
      void* lines = nullptr; int32_t* poff = nullptr; int64_t nl = 0;
      const int64_t lo = (int64_t)r << 17, hi = std::min<int64_t>(D.C, lo + (1ll << 17));
      const int prc = fps_build_pcodes(D.ucodes, D.uoff, D.N, lo, hi, &lines, &poff, &nl, st, D.l0_ppl, D.C, shared, nr, r);
      if (ix->adopt(lines, nl * 16 * D.l0_ppl)) D.n_lines += nl;
      ix->adopt(poff, (D.N + 1) * 8);
      if (prc != 0) return fp_fail(FP_EHIP, "packed-code build failed (hip error " + std::to_string(prc) + ")");
      D.pcodes_r[r] = static_cast<const uint4*>(lines); D.poff_r[r] = poff;
    }
    D.n_ranges = nr;
    D.pcodes = nr > 1 ? static_cast<const uint4*>(shared) : D.pcodes_r[0]; D.poff = D.poff_r[0];
  }
  return FP_OK;
}

extern "C" int fp_index_create(const fp_index_desc* d, int device_id, fp_index** out) {
  if (!d || !out) return fp_fail(FP_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = check_shape(d->nbits, d->dim)) return rc;
  if (d->n_centroids <= 0 || !d->centroids || !d->bucket_weights) return fp_fail(FP_EINVAL, "centroids / bucket_weights missing");
  if (d->n_docs < 0 || (d->n_docs > 0 && (!d->doc_lengths || !d->doc_codes || !d->doc_residuals)))
    return fp_fail(FP_EINVAL, "document arrays missing");
  if (d->n_docs >= 0x7FFFFFFFll) return fp_fail(FP_EUNSUPPORTED, "more than 2^31-1 documents per index shard");
  HIPCHK(fp_set_device(device_id));
  IndexBuild b(device_id);
  fp_index* ix = b.ix.get();
  FpIndexDev& D = ix->d;
  D.nbits = d->nbits; D.dim = d->dim; D.pr = d->dim * d->nbits / 8;
  D.C = d->n_centroids; D.N = d->n_docs; D.pid_offset = d->pid_offset;
  // doc offsets (tensor.rs:221-224)
  ix->h_doc_off.assign((size_t)D.N + 1, 0);
  int maxlen = 0;
  for (int64_t i = 0; i < D.N; ++i) {
    int64_t l = d->doc_lengths[i];
    if (l < 0) return fp_fail(FP_EINVAL, "negative document length");
    ix->h_doc_off[i + 1] = ix->h_doc_off[i] + l;
    if (l > maxlen) maxlen = (int)l;
  }
  D.T = ix->h_doc_off[D.N];
  D.max_doc_len = maxlen;
  int32_t* codes = nullptr; uint8_t* res = nullptr; int64_t* ivf_off = nullptr; int32_t* ivf_pids = nullptr;
  if (int rc = b.open(d->centroids, d->bucket_weights, &codes, &res)) return rc;
  hipStream_t st = b.st;
  if (int rc = upload_narrow(d->doc_codes, codes, D.T, st, D.C, "doc_codes (centroid ids)")) return rc;
  if (D.T > 0) HIPCHK(copy_sync(res, d->doc_residuals, (size_t)D.T * D.pr, hipMemcpyHostToDevice, st));
  if (int rc = finish_layout(ix, maxlen, st)) return rc;
  ix->has_ivf = d->ivf != nullptr && d->ivf_lengths != nullptr;
  D.P = ix->has_ivf ? d->n_ivf_lists : 0;
  std::vector<int64_t> hoff((size_t)D.P + 1, 0);
  for (int64_t i = 0; i < D.P; ++i) {
    if (d->ivf_lengths[i] < 0) return fp_fail(FP_EINVAL, "negative ivf length");
    hoff[i + 1] = hoff[i] + d->ivf_lengths[i];
  }
  HIPCHK(dev_alloc(ix, &ivf_off, hoff.size()));
  HIPCHK(copy_sync(ivf_off, hoff.data(), hoff.size() * 8, hipMemcpyHostToDevice, st));
  const int64_t tot = hoff[D.P];
  HIPCHK(dev_alloc(ix, &ivf_pids, (size_t)tot));
  if (tot > 0) {
    if (int rc = upload_narrow(d->ivf, ivf_pids, tot, st, std::max<int64_t>(D.N, 1), "ivf (document ids)")) return rc;
    // The reference gathers the probed lists and sorts + de-duplicates the ids per query (search.rs:538-541): any order inside a
    // list, repeated ids included, gives the same candidates there.  S3's per-tile range cut needs strictly ascending lists --
    // what create.rs / update.rs / delete.rs write (optimize_ivf).  Anything else is put in that order here, once.
    uint32_t h_flag = 0;
    {
      DevTmp flag;
      HIPCHK(flag.alloc(4));
      HIPCHK(hipMemsetAsync(flag.p, 0, 4, st));
      fpk_ivf_check_sorted(ivf_off, ivf_pids, D.P, flag.as<uint32_t>(), st);
      HIPCHK(hipMemcpyAsync(&h_flag, flag.p, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (h_flag) {
      std::vector<int64_t> fixed;
      fixed.reserve((size_t)tot);
      std::vector<int64_t> noff((size_t)D.P + 1, 0);
      for (int64_t i = 0; i < D.P; ++i) {
        const size_t b0 = fixed.size();
        fixed.insert(fixed.end(), d->ivf + hoff[i], d->ivf + hoff[i + 1]);
        std::sort(fixed.begin() + b0, fixed.end());
        fixed.erase(std::unique(fixed.begin() + b0, fixed.end()), fixed.end());
        noff[i + 1] = (int64_t)fixed.size();
      }
      HIPCHK(copy_sync(ivf_off, noff.data(), noff.size() * 8, hipMemcpyHostToDevice, st));
      if (int rc = upload_narrow(fixed.data(), ivf_pids, (int64_t)fixed.size(), st)) return rc;
    }
  }
  D.ivf_off = ivf_off; D.ivf_pids = ivf_pids;
  return b.hand_over(out);
}

extern "C" int64_t fp_index_num_docs(const fp_index* ix) { return ix ? ix->d.N : 0; }
extern "C" int64_t fp_index_num_tokens(const fp_index* ix) { return ix ? ix->d.T : 0; }
extern "C" int64_t fp_index_num_centroids(const fp_index* ix) { return ix ? ix->d.C : 0; }
extern "C" int32_t fp_index_dim(const fp_index* ix) { return ix ? ix->d.dim : 0; }
extern "C" int32_t fp_index_nbits(const fp_index* ix) { return ix ? ix->d.nbits : 0; }
extern "C" int64_t fp_index_device_bytes(const fp_index* ix) { return ix ? ix->device_bytes() : 0; }
extern "C" int64_t fp_index_num_unique_codes(const fp_index* ix) { return ix ? ix->d.U : 0; }
extern "C" int64_t fp_index_num_code_lines(const fp_index* ix) { return ix ? ix->d.n_lines * ix->d.l0_ppl / 8 : 0; }   // in 128-byte units
extern "C" int64_t fp_index_num_hard_tokens(const fp_index* ix) { return ix ? ix->n_hard_tokens : 0; }
extern "C" int32_t fp_index_tickets_ok(const fp_index* ix) { return ix && ix->tickets_ok ? 1 : 0; }

// ------------------------------------------------------------------------------------------
// synthetic device-resident corpora
// ------------------------------------------------------------------------------------------
extern "C" int fp_index_create_synthetic(const fp_synth_desc* d, int device_id, fp_index** out) {
  if (!d || !out) return fp_fail(FP_EINVAL, "null argument");
  *out = nullptr;
  if (int rc = check_shape(d->nbits, d->dim)) return rc;
  if (d->n_centroids <= 1 || (d->n_centroids & (d->n_centroids - 1))) return fp_fail(FP_EINVAL, "n_centroids must be a power of two");
  if (d->doc_begin < 0 || d->doc_end < d->doc_begin || d->doc_end > d->n_docs_total) return fp_fail(FP_EINVAL, "bad document range");
  if (d->doc_len < 1) return fp_fail(FP_EINVAL, "doc_len < 1");
  HIPCHK(fp_set_device(device_id));
  IndexBuild b(device_id);
  fp_index* ix = b.ix.get();
  ix->synthetic = true;
  FpSynthParams p{};
  p.nbits = d->nbits; p.dim = d->dim; p.pr = d->dim * d->nbits / 8; p.C = d->n_centroids;
  p.lgC = 0;
  while ((1ll << p.lgC) < p.C) ++p.lgC;
  p.n_docs_total = d->n_docs_total; p.doc_begin = d->doc_begin; p.doc_end = d->doc_end;
  p.doc_len = d->doc_len; p.variable_len = d->variable_len; p.seed = d->seed;
  FpIndexDev& D = ix->d;
  D.nbits = p.nbits; D.dim = p.dim; D.pr = p.pr; D.C = p.C; D.P = p.C; D.N = p.doc_end - p.doc_begin; D.pid_offset = p.doc_begin;
  std::vector<int64_t> hoff((size_t)D.N + 2, 0);
  int maxlen = 0;
  D.T = fps_doc_offsets_host(p, hoff.data(), &maxlen);
  const int64_t tok_base = hoff[(size_t)D.N + 1];
  D.max_doc_len = maxlen;
  ix->h_doc_off.assign(hoff.begin(), hoff.begin() + D.N + 1);
  int32_t* codes = nullptr; uint8_t* res = nullptr; int64_t* ivf_off = nullptr; int32_t* ivf_pids = nullptr;
  if (int rc = b.open(d->centroids, d->bucket_weights, &codes, &res)) return rc;
  hipStream_t st = b.st;
  fps_generate(p, D.doc_off, D.N, D.T, tok_base, codes, res, st);
  HIPCHK(hipStreamSynchronize(st));
  if (int rc = finish_layout(ix, maxlen, st)) return rc;
  HIPCHK(dev_alloc(ix, &ivf_off, (size_t)D.P + 1));
  int64_t tot = 0;
  const int rc = fps_build_ivf(D.ucodes, D.uoff, D.N, D.U, D.P, &ivf_pids, &tot, ivf_off, st);
  ix->adopt(ivf_pids, tot * 4);
  if (rc != 0) return fp_fail(FP_EHIP, "IVF build failed (hip/hipcub error " + std::to_string(rc) + ")");
  ix->has_ivf = true;
  D.ivf_off = ivf_off; D.ivf_pids = ivf_pids;
  return b.hand_over(out);
}

// ------------------------------------------------------------------------------------------
// read-back: one document, one IVF list, or every array in the reference's construct_index layout
// ------------------------------------------------------------------------------------------
// one stored residual row -> the reference's byte order (identity unless the index keeps k_maxsim6's unit order)
static inline void row_to_reference_order(const fp_index* ix, const uint8_t* stored, uint8_t* out) {
  const int pr = ix->d.pr;
  if (!ix->d.resid_native) { memcpy(out, stored, (size_t)pr); return; }
  const int nbits = ix->d.nbits, nu = ix->d.dim / 8;
  for (int b = 0; b < pr; ++b) out[b] = stored[fp_resid_pos(b, nbits, nu, 1)];
}

extern "C" int64_t fp_index_read_doc(const fp_index* ix, int64_t doc, int64_t* codes, uint8_t* residuals, int64_t cap) {
  if (!ix || doc < 0 || doc >= ix->d.N) return fp_fail(FP_EINVAL, "bad document id");
  (void)fp_set_device(ix->device);
  const int64_t off = ix->h_doc_off[doc], len = ix->h_doc_off[doc + 1] - off;
  if (len > cap) return fp_fail(FP_EINVAL, "capacity too small");
  const int pr = ix->d.pr;
  std::vector<int32_t> tmp((size_t)len);
  std::vector<uint8_t> rtmp((size_t)len * pr);
  std::vector<uint16_t> perm((size_t)len);
  if (len > 0) {
    HIPCHK(copy_sync(tmp.data(), ix->d.codes + off, (size_t)len * 4, hipMemcpyDeviceToHost, util_stream(ix->device)));
    HIPCHK(copy_sync(rtmp.data(), ix->d.residuals + off * pr, (size_t)len * pr, hipMemcpyDeviceToHost, util_stream(ix->device)));
    if (ix->d.perm) HIPCHK(copy_sync(perm.data(), ix->d.perm + off, (size_t)len * 2, hipMemcpyDeviceToHost, util_stream(ix->device)));
  }
  for (int64_t i = 0; i < len; ++i) {  // stored position i holds original token perm[i]
    const int64_t p = ix->d.perm ? perm[i] : i;
    codes[p] = tmp[i];
    row_to_reference_order(ix, rtmp.data() + i * pr, residuals + p * pr);
  }
  return len;
}

extern "C" int64_t fp_index_read_ivf(const fp_index* ix, int64_t cell, int64_t* pids, int64_t cap) {
  if (!ix || !ix->has_ivf || cell < 0 || cell >= ix->d.P) return fp_fail(FP_EINVAL, "bad cell");
  (void)fp_set_device(ix->device);
  int64_t be[2];
  HIPCHK(copy_sync(be, ix->d.ivf_off + cell, 16, hipMemcpyDeviceToHost, util_stream(ix->device)));
  const int64_t len = be[1] - be[0];
  if (len > cap) return fp_fail(FP_EINVAL, "capacity too small");
  std::vector<int32_t> tmp((size_t)len);
  if (len > 0) HIPCHK(copy_sync(tmp.data(), ix->d.ivf_pids + be[0], (size_t)len * 4, hipMemcpyDeviceToHost, util_stream(ix->device)));
  for (int64_t i = 0; i < len; ++i) pids[i] = tmp[i];
  return len;
}

extern "C" int64_t fp_index_ivf_total(const fp_index* ix) {
  if (!ix || !ix->has_ivf) return 0;
  (void)fp_set_device(ix->device);
  int64_t tot = 0;
  if (copy_sync(&tot, ix->d.ivf_off + ix->d.P, 8, hipMemcpyDeviceToHost, util_stream(ix->device)) != hipSuccess) return fp_fail(FP_EHIP, "memcpy");
  return tot;
}

extern "C" int fp_index_export(const fp_index* ix, int64_t* doc_codes, uint8_t* doc_residuals, int64_t* doc_lengths, int64_t* ivf,
                               int32_t* ivf_lengths) {
  if (!ix) return fp_fail(FP_EINVAL, "null argument");
  HIPCHK(fp_set_device(ix->device));
  const FpIndexDev& D = ix->d;
  if (doc_lengths)
    for (int64_t i = 0; i < D.N; ++i) doc_lengths[i] = ix->h_doc_off[i + 1] - ix->h_doc_off[i];
  const int64_t chunk = 64ll << 20;
  std::vector<int32_t> tmp;
  std::vector<uint16_t> hperm;
  if (D.perm && D.T > 0 && (doc_codes || doc_residuals)) {
    hperm.resize((size_t)D.T);
    HIPCHK(copy_sync(hperm.data(), D.perm, (size_t)D.T * 2, hipMemcpyDeviceToHost, util_stream(ix->device)));
  }
  // stored token i of document d is original token perm[i]: write it back to its original slot
  auto orig_row = [&](int64_t doc, int64_t i) { return hperm.empty() ? i : ix->h_doc_off[doc] + hperm[i]; };
  if (doc_codes) {
    tmp.resize((size_t)std::max<int64_t>(D.T, 1));
    if (D.T > 0) HIPCHK(copy_sync(tmp.data(), D.codes, (size_t)D.T * 4, hipMemcpyDeviceToHost, util_stream(ix->device)));
    for (int64_t d0 = 0; d0 < D.N; ++d0)
      for (int64_t i = ix->h_doc_off[d0]; i < ix->h_doc_off[d0 + 1]; ++i) doc_codes[orig_row(d0, i)] = tmp[i];
  }
  if (doc_residuals && D.T > 0) {
    if (hperm.empty() && !D.resid_native) {
      HIPCHK(copy_sync(doc_residuals, D.residuals, (size_t)D.T * D.pr, hipMemcpyDeviceToHost, util_stream(ix->device)));
    } else {
      std::vector<uint8_t> rt((size_t)std::min<int64_t>(chunk, D.T) * D.pr);
      int64_t d0 = 0;
      for (int64_t s0 = 0; s0 < D.T; s0 += chunk) {
        const int64_t m = std::min(chunk, D.T - s0);
        HIPCHK(copy_sync(rt.data(), D.residuals + s0 * D.pr, (size_t)m * D.pr, hipMemcpyDeviceToHost, util_stream(ix->device)));
        for (int64_t i = s0; i < s0 + m; ++i) {
          while (ix->h_doc_off[d0 + 1] <= i) ++d0;
          row_to_reference_order(ix, rt.data() + (i - s0) * D.pr, doc_residuals + orig_row(d0, i) * D.pr);
        }
      }
    }
  }
  if (ix->has_ivf && (ivf || ivf_lengths)) {
    std::vector<int64_t> off((size_t)D.P + 1);
    HIPCHK(copy_sync(off.data(), D.ivf_off, off.size() * 8, hipMemcpyDeviceToHost, util_stream(ix->device)));
    if (ivf_lengths)
      for (int64_t i = 0; i < D.P; ++i) ivf_lengths[i] = (int32_t)(off[i + 1] - off[i]);
    if (ivf) {
      const int64_t tot = off[D.P];
      tmp.resize((size_t)std::min<int64_t>(chunk, std::max<int64_t>(tot, 1)));
      for (int64_t s = 0; s < tot; s += chunk) {
        const int64_t m = std::min(chunk, tot - s);
        HIPCHK(copy_sync(tmp.data(), D.ivf_pids + s, (size_t)m * 4, hipMemcpyDeviceToHost, util_stream(ix->device)));
        for (int64_t i = 0; i < m; ++i) ivf[s + i] = tmp[i];
      }
    }
  }
  return FP_OK;
}
