// What the three host files share (fp_engine.cpp: search engine and the rest of the C ABI; fp_index.cpp: the life of an fp_index --
// construction, destruction, getters, read-back; fp_build.cpp: the stand-alone index-build operators).
// Each function is defined once, in fp_engine.cpp.  Not part of the C ABI: none of it leaves the library.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "fp_internal.h"

#define FP_HIDDEN __attribute__((visibility("hidden")))

// the error sink: `msg` becomes the calling thread's fp_last_error(), `code` is returned
FP_HIDDEN int fp_fail(int code, const std::string& msg);
// hipSetDevice; the first call on a thread also relaxes that thread's stream-capture mode (see the definition)
FP_HIDDEN hipError_t fp_set_device(int device);
// blocking copies go through an explicit stream, never the legacy one: the caller's own or the device's utility stream
FP_HIDDEN hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st);
FP_HIDDEN hipStream_t util_stream(int device);
// the one deliberate legacy-stream call of the library, at the end of an index construction (see the definition)
FP_HIDDEN void prepay_legacy_stream();

#define HIPCHK(x)                                                                                      \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess)                                                                              \
      return fp_fail(FP_EHIP, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x);         \
  } while (0)

// a search's working set (stream, events, grow-only buffers, captured graphs): private to fp_engine.cpp.  An index pools the
// scratches its searches have used and deletes them, with its device selected, when it goes.
struct Scratch;
FP_HIDDEN void fp_delete_scratch(Scratch* s);

struct FP_HIDDEN fp_index {
  FpIndexDev d{};
  int device = 0;
  bool has_ivf = false;
  std::vector<int64_t> h_doc_off;
  std::mutex mu;
  std::vector<Scratch*> pool;
  bool synthetic = false;
  int64_t n_hard_tokens = 0;   // tokens without a one-multiply reciprocal (k_token_rinv)
  float cent_norm_max = 1.f;   // largest centroid norm (>= 1): scales S1's certification window (FpS1Exact)
  bool tickets_ok = true;      // the fence-free ticket chains passed their self-test on this index's device (finish_layout)
  ~fp_index();   // selects the device, deletes the pooled scratches, frees the device buffers

  // The one way a device buffer becomes the index's (fp_index.cpp): freed by the destructor, `counted` bytes of it reported by
  // fp_index_device_bytes.  adopt() takes what a builder handed back (null: nothing) and is called BEFORE the builder's return
  // code is looked at, so that a failing build frees it with the index.
  template <typename T> hipError_t alloc(T** p, size_t alloc_bytes, int64_t counted);
  template <typename T> T* adopt(T* p, int64_t counted);
  int64_t device_bytes() const { return bytes; }

 private:
  std::vector<void*> owned;
  int64_t bytes = 0;
};
