// k_sink.h -- where a sampled value goes, once for every output kernel: the
// sink a kernel is instantiated with, and the host's window of the running
// mean  X_avg = X_avg*(1-coef) + X*coef, coef = 1/navg  (calc_avg_ocean_vars,
// basic_output.F:421-448; calc_diag_avg, diagnostics.F:709-732).  The host
// part compiles without HIP (tests/mean_window.cpp).
#pragma once

namespace roms {

enum Sink : int { kStore = 0, kMean = 1, kMeanFirst = 2 };   // x | avg*cm1 + x*coef | x*coef, no load

// The window of one producer.  open() starts a sample; without avg every
// sample is a window of its own (navg = 1, coef = 1, cm1 = 0).
struct MeanWindow {
  bool avg = false;
  int navg = 0;                   // samples in the open window
  double coef = 1.0, cm1 = 0.0;   // of the sample under way
  bool have = false;              // there is a sample to write
  void open() {
    navg = avg ? navg + 1 : 1;
    coef = 1.0 / (double)navg;
    cm1 = 1.0 - coef;
    have = true;
  }
  int sink() const { return !avg ? kStore : (coef == 1.0 ? kMeanFirst : kMean); }
  void written() {   // a record took the window: the next sample has coef == 1 (basic_output.F:501, diagnostics.F:778)
    if (!avg) return;
    navg = 0;
    have = false;
  }
  int reported() const { return avg ? navg : 0; }   // navg of the *_state entries
};

}  // namespace roms

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace roms {

template <int SINK>
__device__ __forceinline__ void sink_put(double* __restrict__ p, double x, double coef, double cm1) {
  if (SINK == kStore) *p = x;
  else if (SINK == kMeanFirst) *p = x * coef;
  else *p = *p * cm1 + x * coef;
}

}  // namespace roms

// CALL(SINK) with the compile-time sink that equals the run-time `sink`
#define ROMS_SINKS(sink, CALL)                           \
  do {                                                   \
    if ((sink) == kStore) { CALL(kStore); }              \
    else if ((sink) == kMeanFirst) { CALL(kMeanFirst); } \
    else { CALL(kMean); }                                \
  } while (0)
#endif
