// MeanWindow (ucla-roms_amd/csrc/k_sink.h) alone, on the host: five open() calls with and without avg and one
// written() after the third.  Exit status 0, or 1 after naming each check that failed.
#include <cstdio>

#include "k_sink.h"

using namespace roms;

static int bad = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); bad = 1; } \
  } while (0)

int main() {
  for (int avg = 0; avg < 2; avg++) {
    MeanWindow w;
    w.avg = avg != 0;
    CHECK(w.navg == 0 && !w.have && w.reported() == 0);
    int n = 0;   // samples in the window as the reference counts them
    for (int q = 1; q <= 5; q++) {
      w.open();
      n = avg ? n + 1 : 1;
      const double coef = 1.0 / (double)n;
      CHECK(w.navg == n);
      CHECK(w.coef == coef);         // exactly 1/n
      CHECK(w.cm1 == 1.0 - coef);    // exactly 1 - 1/n
      CHECK(w.have);
      CHECK(w.reported() == (avg ? n : 0));
      CHECK((w.sink() == kMeanFirst) == (avg && w.coef == 1.0));
      CHECK((w.sink() == kStore) == !avg);
      CHECK(avg ? (w.sink() == kMeanFirst) == (n == 1) : w.sink() == kStore);
      if (q == 3) {
        const MeanWindow before = w;
        w.written();
        if (avg) {
          n = 0;
          CHECK(w.navg == 0 && !w.have && w.reported() == 0 && w.avg);
        } else {   // nothing changes
          CHECK(w.avg == before.avg && w.navg == before.navg && w.coef == before.coef && w.cm1 == before.cm1 &&
                w.have == before.have);
        }
      }
    }
    CHECK(w.navg == (avg ? 2 : 1));   // the window after the record holds samples 4 and 5
  }
  CHECK(kStore == 0 && kMean == 1 && kMeanFirst == 2);
  if (!bad) std::printf("ok\n");
  return bad;
}
