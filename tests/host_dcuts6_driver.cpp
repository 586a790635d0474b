// Stand-alone driver (own main) for hz_host.hpp's env_p2_dcuts, the reader of
// pipeline 2's draw cuts (HZ_P2_DCUTS) with six draw stages: five values (the
// first draws of D2-D6, the last may be 24: D6 empty), four values (D2-D5; D6
// keeps its default, raised to D5's), junk, and sets the gap rule rejects
// (a stage of more than seven draws); and with five stages, where only four
// values are read.  Built with -fsanitize=address,undefined by
// tests/test_host_dcuts6_cpu.py.  Every expected value is written out here.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../harmonies-alphazero_amd/csrc/hz_host.hpp"

using namespace hz_host;

static int g_fail = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      g_fail++;                                                 \
    }                                                           \
  } while (0)

static const char *kName = "HZ_P2_DCUTS";

struct Case {
  const char *text;  // nullptr: unset
  bool ok;
  int want[7];       // dcut[0..6] when ok
};

// the cuts on the heap, exactly ndraw + 1 ints: a reader that writes one past
// them, or before them, is ASan's to catch; a guarded stack copy beside it
static void run(int ndraw, const int *dflt, const Case *cases, int n_cases) {
  for (int i = 0; i < n_cases; i++) {
    const Case &c = cases[i];
    if (c.text) setenv(kName, c.text, 1);
    else unsetenv(kName);
    int *heap = (int *)malloc((size_t)(ndraw + 1) * sizeof(int));
    memcpy(heap, dflt, (size_t)(ndraw + 1) * sizeof(int));
    const bool ok = env_p2_dcuts(kName, heap, ndraw, 24, 7);
    CHECK(ok == c.ok);
    for (int k = 0; k <= ndraw; k++) CHECK(heap[k] == (c.ok ? c.want[k] : dflt[k]));
    free(heap);
    int got[9] = {-7, 0, 0, 0, 0, 0, 0, 0, -7};
    memcpy(got + 1, dflt, (size_t)(ndraw + 1) * sizeof(int));
    got[ndraw + 2] = -7;
    CHECK(env_p2_dcuts(kName, got + 1, ndraw, 24, 7) == c.ok);
    CHECK(got[0] == -7 && got[ndraw + 2] == -7);
    for (int k = 0; k <= ndraw; k++) CHECK(got[1 + k] == (c.ok ? c.want[k] : dflt[k]));
    if (ok != c.ok) printf("  ndraw %d case %d (%s)\n", ndraw, i, c.text ? c.text : "unset");
  }
  unsetenv(kName);
}

int main() {
  const int dflt6[7] = {0, 5, 9, 13, 17, 20, 24};
  const Case six[] = {
      {nullptr, false, {}},
      // five values
      {"5,9,13,17,20", true, {0, 5, 9, 13, 17, 20, 24}},
      {"1,3,10,17,24", true, {0, 1, 3, 10, 17, 24, 24}},   // D6 draws nothing
      {"3,6,10,14,17", true, {0, 3, 6, 10, 14, 17, 24}},   // D6 makes seven draws
      {"1,2,3,4,17", false, {}},                           // D6 seven, but D5 thirteen
      {"7,14,21,22,23", true, {0, 7, 14, 21, 22, 23, 24}},
      {"1,2,3,4,16", false, {}},                           // D6 would make eight
      {"1,2,3,4,5", false, {}},                            // ... nineteen
      {"8,9,13,17,20", false, {}},                         // D1 eight
      {"5,9,17,20,22", false, {}},                         // D3 eight
      {"5,9,13,17,25", false, {}},                         // past the last draw
      {"5,9,13,24,24", false, {}},                         // not increasing (only D6 may be empty by 24)
      {"5,9,13,17,17", false, {}},
      {"0,9,13,17,20", false, {}},                         // stage 1's start is not listed
      {"5,9,13,17,20,22", false, {}},                      // six values
      {"5,9,13,17,20,", false, {}},
      {"5,9,13,17,20x", false, {}},
      {"5,9,13,17, 20", false, {}},
      {"5,9,13,17,-20", false, {}},
      {"5,9,13,17,99999999999999999999", false, {}},
      // four values: D6 from the default (20), raised to D5's
      {"1,3,10,17", true, {0, 1, 3, 10, 17, 20, 24}},
      {"7,14,21,23", true, {0, 7, 14, 21, 23, 23, 24}},    // D5 empty, D6 draws the last
      {"6,11,15,19", true, {0, 6, 11, 15, 19, 20, 24}},
      {"6,12,18,20", true, {0, 6, 12, 18, 20, 20, 24}},
      {"1,2,3,4", false, {}},                              // D5 would make sixteen up to the default
      {"6,11,12,13", true, {0, 6, 11, 12, 13, 20, 24}},    // D5 seven
      {"6,10,11,12", false, {}},                           // D5 eight
      {"7,13,18,24", false, {}},                           // four values end at 23
      {"8,14,21,23", false, {}},
      {"7,13,18", false, {}},
      {"7,7,18,21", false, {}},
      {"13,7,18,21", false, {}},
      {"garbage", false, {}},
      {"", false, {}},
      {",,,,", false, {}},
      {"1,2,3,4,", false, {}},
  };
  run(6, dflt6, six, (int)(sizeof(six) / sizeof(six[0])));

  // five stages: four values only, as before
  const int dflt5[6] = {0, 6, 11, 15, 19, 24};
  const Case five[] = {
      {nullptr, false, {}},
      {"1,3,10,17", true, {0, 1, 3, 10, 17, 24}},
      {"7,14,21,23", true, {0, 7, 14, 21, 23, 24}},
      {"1,2,3,4", false, {}},              // the last stage would make twenty
      {"8,14,21,23", false, {}},
      {"1,3,10,17,24", false, {}},         // five values are a six-stage setting
      {"1,3,10,17,20", false, {}},
      {"7,13,18,24", false, {}},
      {"garbage", false, {}},
  };
  run(5, dflt5, five, (int)(sizeof(five) / sizeof(five[0])));

  // stage counts the reader does not know leave the cuts alone
  setenv(kName, "1,3,10,17", 1);
  int keep[10] = {0, 6, 11, 15, 19, 24, 24, 24, 24, 24};
  CHECK(!env_p2_dcuts(kName, keep, 1, 24, 7) && !env_p2_dcuts(kName, keep, 9, 24, 7));
  CHECK(keep[1] == 6 && keep[4] == 19 && keep[9] == 24);
  unsetenv(kName);

  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("host dcuts6 driver ok\n");
  return 0;
}
