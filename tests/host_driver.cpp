// Stand-alone check of libhz's host layer (csrc/hz_host.hpp, its HIP-free
// part, and the request lists of the search handle's buffers and its launch-form picker, csrc/hz_mcts.hpp): built with ASan + UBSan by tests/test_host_cpu.py and run without a
// GPU.  The expected values are written out from the rules the knobs had
// before they shared a reader; nothing here is computed by the code under test.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <set>

#include "../harmonies-alphazero_amd/csrc/hz_host.hpp"
#include "../harmonies-alphazero_amd/csrc/hz_mcts.hpp"

using namespace hz_host;

static int g_fail = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      g_fail++;                                                 \
    }                                                           \
  } while (0)

static void put(const char *name, const char *v) {
  if (v) setenv(name, v, 1);
  else unsetenv(name);
}

// ------------------------------------------------------------------ knobs
// the seven cases of every rule: unset, "", "0", "1", "abc", the special
// value, a value outside the knob's range
struct PickCase {
  const char *name;
  int special, otherwise;
  const char *special_s, *outside_s;
  int want[7];
};
static const PickCase kPick[] = {
    // on unless the value parses to 0
    {"HZ_AR_AHEAD", 0, 1, "0", "-5", {1, 0, 0, 1, 0, 0, 1}},
    {"HZ_X6_W4", 0, 1, "0", "2", {1, 0, 0, 1, 0, 0, 1}},
    {"HZ_STEM_CS4", 0, 1, "0", "2", {1, 0, 0, 1, 0, 0, 1}},
    // off unless it parses to 1
    {"HZ_X6_CS4", 1, 0, "1", "2", {0, 0, 0, 1, 0, 1, 0}},
    // this one value or the default
    {"HZ_PIPELINE", 1, 2, "1", "3", {2, 2, 2, 1, 2, 1, 2}},
    {"HZ_TS_AHEAD", 12, 4, "12", "18", {4, 4, 4, 4, 4, 12, 4}},
};

static void test_knobs() {
  for (const PickCase &c : kPick) {
    const char *in[7] = {nullptr, "", "0", "1", "abc", c.special_s, c.outside_s};
    for (int i = 0; i < 7; i++) {
      put(c.name, in[i]);
      const int got = env_pick(c.name, c.special, c.otherwise);
      if (got != c.want[i]) printf("%s=%s: %d, want %d\n", c.name, in[i] ? in[i] : "(unset)", got, c.want[i]);
      CHECK(got == c.want[i]);
    }
    put(c.name, nullptr);
  }
  // plain integers (HZ_X6_SMALL_MAX, HZ_X6_TINY_MAX, HZ_HEADS1_MAX, HZ_TOWER_STAGGER)
  {
    const char *in[7] = {nullptr, "", "0", "1", "abc", "4096", "-3"};
    const int want[7] = {768, 0, 0, 1, 0, 4096, -3};
    for (int i = 0; i < 7; i++) {
      put("HZ_X6_SMALL_MAX", in[i]);
      CHECK(env_int("HZ_X6_SMALL_MAX", 768) == want[i]);
    }
    put("HZ_X6_SMALL_MAX", nullptr);
  }
  // HZ_TS_RB1_MAX: default 10, clamped to [0, 256 / (3 * 8)] = [0, 10]
  {
    const char *in[8] = {nullptr, "", "0", "1", "abc", "7", "1000", "-4"};
    const int want[8] = {10, 0, 0, 1, 0, 7, 10, 0};
    for (int i = 0; i < 8; i++) {
      put("HZ_TS_RB1_MAX", in[i]);
      CHECK(env_clamped("HZ_TS_RB1_MAX", 10, 0, 10) == want[i]);
    }
    put("HZ_TS_RB1_MAX", nullptr);
    CHECK(env_clamped("HZ_TS_RB1_MAX", 99, 0, 10) == 10);  // the default is clamped too
  }
  // HZ_P2_CUTS: three increasing positive multiples of 4, else 24, 40, 56
  {
    struct {
      const char *in;
      int want[3];
    } cuts[] = {
        {nullptr, {24, 40, 56}},       {"", {24, 40, 56}},           {"0", {24, 40, 56}},
        {"1", {24, 40, 56}},           {"abc", {24, 40, 56}},        {"16,32,48", {16, 32, 48}},
        {"8,20,60", {8, 20, 60}},      {"16, 32, 48", {16, 32, 48}}, {"16,32,48,64", {16, 32, 48}},
        {"16,32", {24, 40, 56}},       {"32,16,48", {24, 40, 56}},   {"16,16,32", {24, 40, 56}},
        {"0,4,8", {24, 40, 56}},       {"-4,4,8", {24, 40, 56}},     {"10,20,30", {24, 40, 56}},
        {"16,32,50", {24, 40, 56}},    {"16,x,48", {24, 40, 56}},    {"4,8,12", {4, 8, 12}},
    };
    for (auto &c : cuts) {
      put("HZ_P2_CUTS", c.in);
      int got[3] = {24, 40, 56};
      env_cuts("HZ_P2_CUTS", got);
      if (got[0] != c.want[0] || got[1] != c.want[1] || got[2] != c.want[2])
        printf("HZ_P2_CUTS=%s: %d,%d,%d\n", c.in ? c.in : "(unset)", got[0], got[1], got[2]);
      CHECK(got[0] == c.want[0] && got[1] == c.want[1] && got[2] == c.want[2]);
    }
    put("HZ_P2_CUTS", nullptr);
  }
}

// HZ_X6_BLOCK / HZ_BLK_TABLE (on unless 0) and HZ_TOWER_STAGGER (integer,
// default 4): the first use reads the environment unless the setter came
// first; the setter wins from then on; the environment is read once
static void test_settings() {
  const char *in[7] = {nullptr, "", "0", "1", "abc", "0", "5"};
  const bool want_on[7] = {true, false, false, true, false, false, true};
  const int want_stagger[7] = {4, 0, 0, 1, 0, 0, 5};
  for (int i = 0; i < 7; i++) {
    put("HZ_X6_BLOCK", in[i]);
    put("HZ_TOWER_STAGGER", in[i]);
    Setting blk{"HZ_X6_BLOCK", 1}, stg{"HZ_TOWER_STAGGER", 4};
    CHECK((blk.get() != 0) == want_on[i]);
    CHECK(stg.get() == want_stagger[i]);
    put("HZ_X6_BLOCK", want_on[i] ? "0" : "1");  // too late: read once
    put("HZ_TOWER_STAGGER", "77");
    CHECK((blk.get() != 0) == want_on[i]);
    CHECK(stg.get() == want_stagger[i]);
    blk.set(want_on[i] ? 0 : 1);  // the setter after the first use
    stg.set(9);
    CHECK((blk.get() != 0) == !want_on[i]);
    CHECK(stg.get() == 9);
  }
  put("HZ_X6_BLOCK", "0");
  put("HZ_TOWER_STAGGER", "6");
  Setting blk{"HZ_X6_BLOCK", 1}, stg{"HZ_TOWER_STAGGER", 4};
  blk.set(1);  // the setter before the first use
  stg.set(0);
  CHECK(blk.get() == 1);
  CHECK(stg.get() == 0);
  stg.set(-1);  // (no value of the setter's reads as "not read yet")
  CHECK(stg.get() == -1);
  put("HZ_X6_BLOCK", nullptr);
  put("HZ_TOWER_STAGGER", nullptr);
}

// ---------------------------------------------------------------- buffers
// a counting allocator over malloc (so the leak check sees what the owner
// drops): the k-th alloc or the k-th fill can be made to fail
struct FakeDev {
  static std::set<void *> live;
  static int allocs, frees, fills, bad_frees, fail_alloc_at, fail_fill_at;
  static void reset(int fail_alloc, int fail_fill) {
    allocs = frees = fills = bad_frees = 0;
    fail_alloc_at = fail_alloc;
    fail_fill_at = fail_fill;
  }
  static bool alloc(void **p, size_t bytes) {
    if (++allocs == fail_alloc_at) return false;
    *p = malloc(bytes);
    live.insert(*p);
    return true;
  }
  static bool fill(void *p, int byte, size_t bytes) {
    if (++fills == fail_fill_at) return false;
    if (!live.count(p)) bad_frees++;
    for (size_t i = 0; i < bytes; i++) ((unsigned char *)p)[i] = (unsigned char)byte;
    return true;
  }
  static bool fill_async(void *p, int byte, size_t bytes, void *) { return fill(p, byte, bytes); }
  static void free(void *p) {
    frees++;
    if (!live.erase(p)) {
      bad_frees++;  // never obtained, or freed twice
      return;
    }
    ::free(p);
  }
};
std::set<void *> FakeDev::live;
int FakeDev::allocs, FakeDev::frees, FakeDev::fills, FakeDev::bad_frees, FakeDev::fail_alloc_at, FakeDev::fail_fill_at;

struct Handle {  // pointers of several types, some in arrays and nested structs, as hz_env has
  DevBufsT<FakeDev> bufs;
  uint64_t *state;
  uint32_t *mt[2];
  int32_t *tag;
  struct {
    int32_t *k;
    uint64_t *q;
  } draw;
  unsigned char *bytes;
};
constexpr int kRequests = 7, kFills = 3;

static bool request_all(Handle *h) {
  auto &o = h->bufs;
  o.get(h->state, 6 * 8, 0);
  o.get(h->mt[0], 624 * 4);
  o.get(h->mt[1], 624 * 4);
  o.get(h->tag, 64 * 4, 0xff);
  o.get(h->draw.k, 4);
  o.get(h->draw.q, 8 * 3);
  o.get(h->bytes, 5, 0xff, nullptr);
  return o.ok;
}
static bool all_null(const Handle *h) {
  return !h->state && !h->mt[0] && !h->mt[1] && !h->tag && !h->draw.k && !h->draw.q && !h->bytes;
}

static void test_bufs() {
  Handle *h = new Handle();
  CHECK(all_null(h));
  // normal use, then release() twice
  FakeDev::reset(0, 0);
  CHECK(request_all(h));
  CHECK(FakeDev::allocs == kRequests && FakeDev::fills == kFills && (int)FakeDev::live.size() == kRequests);
  CHECK(h->state && h->mt[0] && h->mt[1] && h->tag && h->draw.k && h->draw.q && h->bytes);
  CHECK(h->state[5] == 0 && h->tag[63] == -1 && h->bytes[4] == 0xff);
  h->bufs.release();
  CHECK(FakeDev::frees == kRequests && FakeDev::bad_frees == 0 && FakeDev::live.empty() && all_null(h));
  h->bufs.release();
  CHECK(FakeDev::frees == kRequests && FakeDev::bad_frees == 0 && h->bufs.ok);
  // the k-th allocation fails, then the k-th fill
  for (int pass = 0; pass < 2; pass++)
    for (int k = 1; k <= (pass ? kFills : kRequests); k++) {
      FakeDev::reset(pass ? 0 : k, pass ? k : 0);
      CHECK(!request_all(h));
      CHECK(!h->bufs.ok);
      const int got = (int)FakeDev::live.size();
      if (!pass) CHECK(got == k - 1 && FakeDev::allocs == k);  // nothing requested past the failure
      int32_t *late = nullptr;
      CHECK(!h->bufs.get(late, 16) && !late && (int)FakeDev::live.size() == got);
      h->bufs.release();
      CHECK(FakeDev::frees == got && FakeDev::bad_frees == 0 && FakeDev::live.empty() && all_null(h));
      // the handle stays usable: the same requests succeed afterwards
      FakeDev::reset(0, 0);
      CHECK(request_all(h) && (int)FakeDev::live.size() == kRequests);
      h->bufs.release();
      CHECK(FakeDev::frees == kRequests && FakeDev::bad_frees == 0 && FakeDev::live.empty() && all_null(h));
    }
  delete h;
}

// ------------------------------------------- the search handle's three groups
// hz_mcts's buffers as hz_mcts.hpp's request lists ask for them: the base
// group has 23 requests of which 9 are filled (ht, counts, depth, err,
// sims_done, budget_buf, mask_buf with 0; leaf, leaf_gidx with 0xff), the
// carry group 3 and 1 (carry), the Gumbel group 4 and 2 (g_score, root_value)
struct TreeHandle : hz_mcts_args {
  DevBufsT<FakeDev> base_bufs, carry_bufs, gumbel_bufs;
};
struct TreeGroup {
  const char *name;
  int requests, fills;
  DevBufsT<FakeDev> TreeHandle::*bufs;
  bool (*request)(DevBufsT<FakeDev> &, hz_mcts_args &);
  int (*held)(const hz_mcts_args &);  // how many of the group's pointers are not null
};
static int count_set(std::initializer_list<const void *> ps) {
  int c = 0;
  for (const void *p : ps) c += p != nullptr;
  return c;
}
static int held_base(const hz_mcts_args &a) {
  return count_set({a.node_state, a.node_key, a.node_e0, a.node_ne, a.edge_action, a.edge_child, a.edge_n, a.edge_w,
                    a.edge_p, a.edge_player, a.edge_hint, a.ht, a.counts, a.path, a.depth, a.leaf, a.leaf_gidx, a.slot,
                    a.gidx_c, a.err, a.sims_done, a.budget_buf, a.mask_buf});
}
static int held_carry(const hz_mcts_args &a) { return count_set({a.carry, a.adv_remap, a.adv_queue}); }
static int held_gumbel(const hz_mcts_args &a) { return count_set({a.gumbel_buf, a.g_score, a.root_value, a.g_table}); }
static const TreeGroup kTreeGroups[3] = {
    {"base", 23, 9, &TreeHandle::base_bufs, hz_tree::request_base<DevBufsT<FakeDev>>, held_base},
    {"carry", 3, 1, &TreeHandle::carry_bufs, hz_tree::request_carry<DevBufsT<FakeDev>>, held_carry},
    {"gumbel", 4, 2, &TreeHandle::gumbel_bufs, hz_tree::request_gumbel<DevBufsT<FakeDev>>, held_gumbel},
};

static void test_tree_groups() {
  TreeHandle *h = new TreeHandle();
  h->n = 3;
  h->max_nodes = h->max_edges = 5;
  h->hcap = 16;
  h->max_depth = 4;
  CHECK(held_base(*h) + held_carry(*h) + held_gumbel(*h) == 0);
  // no failure: every pointer of a group is set by its list, the filled ones hold their byte
  FakeDev::reset(0, 0);
  int want_live = 0, want_fills = 0;
  for (const TreeGroup &g : kTreeGroups) {
    CHECK(g.request(h->*g.bufs, *h) && (h->*g.bufs).ok);
    want_live += g.requests;
    want_fills += g.fills;
    CHECK(g.held(*h) == g.requests);
    CHECK((int)FakeDev::live.size() == want_live && FakeDev::allocs == want_live && FakeDev::fills == want_fills);
  }
  CHECK(want_live == 30 && want_fills == 12);
  CHECK(h->ht[3 * 16 - 1] == 0 && h->counts[3 * 4 - 1] == 0 && h->depth[2] == 0 && h->err[0] == 0);
  CHECK(h->sims_done[2] == 0 && h->budget_buf[2] == 0 && h->mask_buf[2] == 0);
  CHECK(h->leaf[2] == -1 && h->leaf_gidx[2] == -1);
  CHECK(h->carry[2] == 0 && h->g_score[3 * 69 - 1] == 0.0 && h->root_value[2] == 0.f);
  CHECK(!h->budget && !h->noise_mask && !h->gumbel && !h->eval_ctr);  // (aliases and borrowed: no list sets them)
  for (const TreeGroup &g : kTreeGroups) (h->*g.bufs).release();
  CHECK(FakeDev::live.empty() && FakeDev::bad_frees == 0 && FakeDev::frees == 30);
  CHECK(held_base(*h) + held_carry(*h) + held_gumbel(*h) == 0);
  // group g's k-th allocation fails, then its k-th fill, while the two other groups are held
  for (const TreeGroup &g : kTreeGroups)
    for (int pass = 0; pass < 2; pass++)
      for (int k = 1; k <= (pass ? g.fills : g.requests); k++) {
        FakeDev::reset(0, 0);
        int others = 0;
        for (const TreeGroup &o : kTreeGroups)
          if (&o != &g) {
            CHECK(o.request(h->*o.bufs, *h));
            others += o.requests;
          }
        const hz_mcts_args before = *h;
        const int start = (int)FakeDev::live.size();
        CHECK(start == others && others == 30 - g.requests);
        FakeDev::reset(pass ? 0 : k, pass ? k : 0);
        CHECK(!g.request(h->*g.bufs, *h));
        CHECK(!(h->*g.bufs).ok);
        if (!pass) CHECK((int)FakeDev::live.size() == start + k - 1 && g.held(*h) == k - 1);
        (h->*g.bufs).release();
        CHECK((h->*g.bufs).ok && g.held(*h) == 0);
        CHECK((int)FakeDev::live.size() == start && FakeDev::bad_frees == 0);
        for (const TreeGroup &o : kTreeGroups)
          if (&o != &g) CHECK(o.held(*h) == o.requests);
        // the other groups' pointers are the ones they were (g's are null on both sides)
        const hz_mcts_args &a = *h;
        CHECK(a.node_state == before.node_state && a.node_key == before.node_key && a.node_e0 == before.node_e0 &&
              a.node_ne == before.node_ne && a.edge_action == before.edge_action && a.edge_child == before.edge_child &&
              a.edge_n == before.edge_n && a.edge_w == before.edge_w && a.edge_p == before.edge_p &&
              a.edge_player == before.edge_player && a.edge_hint == before.edge_hint && a.ht == before.ht &&
              a.counts == before.counts && a.path == before.path && a.depth == before.depth && a.leaf == before.leaf &&
              a.leaf_gidx == before.leaf_gidx && a.slot == before.slot && a.gidx_c == before.gidx_c &&
              a.err == before.err && a.sims_done == before.sims_done && a.budget_buf == before.budget_buf &&
              a.mask_buf == before.mask_buf);
        CHECK(a.carry == before.carry && a.adv_remap == before.adv_remap && a.adv_queue == before.adv_queue);
        CHECK(a.gumbel_buf == before.gumbel_buf && a.g_score == before.g_score && a.root_value == before.root_value &&
              a.g_table == before.g_table);
        // a later call tries again, and succeeds
        FakeDev::reset(0, 0);
        CHECK(g.request(h->*g.bufs, *h) && g.held(*h) == g.requests && (int)FakeDev::live.size() == 30);
        for (const TreeGroup &o : kTreeGroups) (h->*o.bufs).release();
        CHECK(FakeDev::live.empty() && FakeDev::bad_frees == 0);
        CHECK(held_base(*h) + held_carry(*h) + held_gumbel(*h) == 0);
      }
  delete h;
}

// ------------------------------------------------------------ the launch form
// pick_form over every combination of the gates and of a launch with or
// without a select, against the instantiation the three launch ladders of
// hz_mcts.hip chose before they shared it (root form 0 PUCT, 1 Gumbel, 2
// forced; -1: the entry point returned -1), and with_form reaching exactly
// that instantiation
struct FormCase {
  bool gumbel, forced, leaf_key, walk;
  int root;
  bool sym;
};
static const FormCase kForms[16] = {
    {false, false, false, false, 0, false}, {false, false, false, true, 0, false},
    {false, false, true, false, 0, true},   {false, false, true, true, 0, true},
    {false, true, false, false, 0, false},  {false, true, false, true, 2, false},
    {false, true, true, false, 0, true},    {false, true, true, true, 2, true},
    {true, false, false, false, 1, false},  {true, false, false, true, 1, false},
    {true, false, true, false, -1, false},  {true, false, true, true, -1, false},
    {true, true, false, false, -1, false},  {true, true, false, true, -1, false},
    {true, true, true, false, -1, false},   {true, true, true, true, -1, false},
};

static void test_launch_forms() {
  for (const FormCase &c : kForms) {
    const hz_tree::LaunchForm f = hz_tree::pick_form(c.gumbel, c.forced, c.leaf_key, c.walk);
    if (f.root != c.root || (c.root >= 0 && f.sym != c.sym))
      printf("gumbel %d forced %d leaf_key %d walk %d: root %d sym %d\n", c.gumbel, c.forced, c.leaf_key, c.walk, f.root,
             f.sym);
    CHECK(f.root == c.root);
    if (c.root >= 0) CHECK(f.sym == c.sym);
    // the handle's fields read as the gates
    hz_mcts_args a{};
    double g = 0.0;
    uint64_t key = 0;
    a.gumbel = c.gumbel ? &g : nullptr;
    a.forced_k = c.forced ? 2.0 : 0.0;
    a.leaf_key = c.leaf_key ? &key : nullptr;
    CHECK(hz_tree::pick_form(a, c.walk).root == c.root && (c.root < 0 || hz_tree::pick_form(a, c.walk).sym == c.sym));
    // the dispatch: one call, with the picked form's constants; none for a refused combination
    int calls = 0, root = -2;
    bool sym = false;
    const auto note = [&](auto form) {
      calls++;
      root = decltype(form)::root;
      sym = decltype(form)::sym;
    };
    if (c.walk) hz_tree::with_form<true>(f, note);
    else hz_tree::with_form<false>(f, note);
    CHECK(calls == (c.root >= 0 ? 1 : 0));
    if (c.root >= 0) CHECK(root == c.root && sym == c.sym);
  }
}

// --------------------------------------------------------- stream windows
struct FakeEnv {
  int32_t *pw_tag;
  size_t nrow;
  void *stream;
};
static void test_windows_voided() {
  FakeDev::reset(0, 0);
  FakeEnv e{nullptr, 128, nullptr};
  int32_t *guard = nullptr;
  void *raw = nullptr;
  CHECK(FakeDev::alloc(&raw, (e.nrow + 1) * sizeof(int32_t)));
  e.pw_tag = static_cast<int32_t *>(raw);
  guard = e.pw_tag + e.nrow;
  for (size_t b = 0; b <= e.nrow; b++) e.pw_tag[b] = (int32_t)b;
  CHECK(streams_touched<FakeDev>(&e));
  for (size_t b = 0; b < e.nrow; b++) CHECK(e.pw_tag[b] == -1);  // every row's tag: none
  CHECK(*guard == (int32_t)e.nrow);                              // and nothing past them
  FakeDev::reset(0, 1);
  CHECK(!streams_touched<FakeDev>(&e));  // a fill that cannot be enqueued is reported
  FakeDev::free(raw);
  CHECK(FakeDev::bad_frees == 0 && FakeDev::live.empty());
}

int main() {
  test_knobs();
  test_settings();
  test_bufs();
  test_tree_groups();
  test_launch_forms();
  test_windows_voided();
  if (g_fail) {
    printf("host driver: %d checks failed\n", g_fail);
    return 1;
  }
  printf("host driver ok\n");
  return 0;
}
