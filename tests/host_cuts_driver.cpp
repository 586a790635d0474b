// Stand-alone driver (own main) for hz_host.hpp's env_cuts_n, the reader of
// pipeline 2's play cuts (HZ_P2_CUTS5: four increasing positive multiples of
// 4) and draw cuts (HZ_P2_DCUTS: four increasing draws in 1..23), built with
// -fsanitize=address,undefined by tests/test_host_cuts_cpu.py.  Every
// expected value is written out here.
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

static void put(const char *name, const char *v) {
  if (v) setenv(name, v, 1);
  else unsetenv(name);
}

struct Case {
  const char *text;  // nullptr: unset
  bool ok;
  int want[4];
};

static void run(const char *name, int step, int hi, const int dflt[4], const Case *cases, int n_cases) {
  for (int i = 0; i < n_cases; i++) {
    const Case &c = cases[i];
    put(name, c.text);
    // the four cuts inside a guarded array: a reader that writes a fifth
    // value, or one before the first, is caught here (and by ASan on the
    // heap copy below)
    int got[6] = {-7, dflt[0], dflt[1], dflt[2], dflt[3], -7};
    const bool ok = env_cuts_n(name, got + 1, 4, step, hi);
    CHECK(ok == c.ok);
    CHECK(got[0] == -7 && got[5] == -7);
    for (int k = 0; k < 4; k++) CHECK(got[1 + k] == (c.ok ? c.want[k] : dflt[k]));
    int *heap = (int *)malloc(4 * sizeof(int));
    memcpy(heap, dflt, 4 * sizeof(int));
    CHECK(env_cuts_n(name, heap, 4, step, hi) == c.ok);
    for (int k = 0; k < 4; k++) CHECK(heap[k] == (c.ok ? c.want[k] : dflt[k]));
    free(heap);
    if (!ok && c.ok) printf("  case %d (%s)\n", i, c.text ? c.text : "unset");
  }
  unsetenv(name);
}

int main() {
  const int play_dflt[4] = {16, 32, 48, 64};
  const Case play[] = {
      {nullptr, false, {}},                       // unset
      {"4,8,12,16", true, {4, 8, 12, 16}},        // the smallest
      {"60,64,68,72", true, {60, 64, 68, 72}},    // late
      {"24,40,56,1048576", true, {24, 40, 56, 1048576}},  // the upper bound itself
      {"24,40,56,1048580", false, {}},            // past it
      {"24,40,56", false, {}},                    // wrong count: three
      {"24,40,56,64,72", false, {}},              // wrong count: five
      {"24,40,56,", false, {}},                   // a trailing comma
      {"24,40,40,56", false, {}},                 // not increasing
      {"40,24,56,64", false, {}},                 // decreasing
      {"0,8,12,16", false, {}},                   // not positive
      {"-4,8,12,16", false, {}},                  // a sign
      {"4,8,12,18", false, {}},                   // not a multiple of 4
      {"5,8,12,16", false, {}},
      {"", false, {}},                            // empty
      {"garbage", false, {}},
      {"4,8,12,16x", false, {}},                  // something after the last
      {"4, 8,12,16", false, {}},                  // a blank
      {"4;8;12;16", false, {}},
      {"4,8,,16", false, {}},
      {"99999999999999999999,8,12,16", false, {}},  // overflows a long
      {"4,8,12,99999999999999999999", false, {}},
  };
  run("HZ_P2_CUTS5", 4, 1 << 20, play_dflt, play, (int)(sizeof(play) / sizeof(play[0])));

  const int draw_dflt[4] = {5, 10, 14, 18};
  const Case draw[] = {
      {nullptr, false, {}},
      {"1,2,3,4", true, {1, 2, 3, 4}},
      {"20,21,22,23", true, {20, 21, 22, 23}},
      {"7,13,18,21", true, {7, 13, 18, 21}},
      {"7,13,18,24", false, {}},   // draw 24 does not exist
      {"0,7,13,18", false, {}},    // stage 1's start is not listed
      {"7,13,18", false, {}},
      {"7,13,18,21,23", false, {}},
      {"7,7,18,21", false, {}},
      {"13,7,18,21", false, {}},
      {"garbage", false, {}},
      {"", false, {}},
  };
  run("HZ_P2_DCUTS", 1, 23, draw_dflt, draw, (int)(sizeof(draw) / sizeof(draw[0])));

  // the draw stages' lengths (first draw 0, the cuts, one past the last draw)
  {
    const int fits[6] = {0, 7, 14, 21, 23, 24}, early[6] = {0, 1, 3, 10, 17, 24};
    const int long_first[6] = {0, 8, 14, 21, 23, 24}, long_last[6] = {0, 1, 2, 3, 4, 24};
    CHECK(cuts_gaps_within(fits, 6, 7) && cuts_gaps_within(early, 6, 7));
    CHECK(!cuts_gaps_within(long_first, 6, 7) && !cuts_gaps_within(long_last, 6, 7));
    CHECK(cuts_gaps_within(long_last, 5, 7));   // (only the values given)
    CHECK(cuts_gaps_within(fits, 1, 0) && cuts_gaps_within(fits, 0, 0));
  }

  // the argument checks: a count outside 1..8 or a step below 1 reads nothing
  put("HZ_P2_CUTS5", "4,8,12,16");
  int keep[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  CHECK(!env_cuts_n("HZ_P2_CUTS5", keep, 0, 4, 100) && !env_cuts_n("HZ_P2_CUTS5", keep, 9, 4, 100) &&
        !env_cuts_n("HZ_P2_CUTS5", keep, 4, 0, 100));
  for (int k = 0; k < 9; k++) CHECK(keep[k] == k + 1);
  unsetenv("HZ_P2_CUTS5");

  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("host cuts driver ok\n");
  return 0;
}
