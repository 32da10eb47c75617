// What the two host files (fp_engine.cpp: search engine and C ABI; fp_build.cpp: the stand-alone index-build operators) share.
// Each item is defined once, in fp_engine.cpp.  Not part of the C ABI: none of it leaves the library.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

// the error sink: `msg` becomes the calling thread's fp_last_error(), `code` is returned
__attribute__((visibility("hidden"))) int fp_fail(int code, const std::string& msg);
// hipSetDevice; the first call on a thread also relaxes that thread's stream-capture mode (see the definition)
__attribute__((visibility("hidden"))) hipError_t fp_set_device(int device);

#define HIPCHK(x)                                                                                      \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess)                                                                              \
      return fp_fail(FP_EHIP, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x);         \
  } while (0)
