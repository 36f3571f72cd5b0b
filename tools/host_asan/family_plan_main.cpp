// The route plan of a batch at its edges: family_plan (static in ramx_device.hip), which needs no device, under ASan + UBSan.
// Host code only: nothing here touches a GPU (the CU count is given by hand; the class and device-wide plans it asks for are
// ramx_cp.hip's host functions, taken from the built library).  Built and run by tools/host_asan/run.sh.
#include "../../repeatafterme_amd/csrc/ramx_device.hip"

#include <random>

static int g_failed;      // (every case is looked at: one wrong group does not hide the next)
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); g_failed++; } } while (0)

static int g_tab[RAMX_NCLASS][4];
static const int NC = RAMX_CP_NCLASS;

struct Batch
{
  std::vector<ramx_flank> fl; std::vector<int32_t> first, count;
  int n() const { return (int)count.size(); }
};

// families of these sizes, every flank starting at the core edge, each family padded to whole tiles with empty flanks
static Batch batch_of(const std::vector<int> &sizes)
{
  Batch b;
  for (int nx : sizes)
  {
    b.first.push_back((int32_t)b.fl.size()); b.count.push_back(nx);
    for (int i = 0; i < ((nx + 63) / 64) * 64; i++)
    {
      ramx_flank x = empty_flank();
      if (i < nx) { x.start = 1000 * (int64_t)b.fl.size(); x.t_lo = i % 3 ? 0 : -(i % 7); x.t_hi = 300; }
      b.fl.push_back(x);
    }
  }
  if (b.fl.empty()) b.fl.push_back(empty_flank());
  return b;
}

struct Case { int W = 40, go = -30, ge = -5, L = 200, cus = 256; bool force_chain = false, allow_dev = true; };

static FamilyPlan plan(const Batch &b, const Case &c = Case())
{
  return family_plan(route_env(), c.W, c.go, c.ge, g_tab, c.L, c.cus, c.force_chain, c.allow_dev, b.fl.data(), b.first.data(), b.count.data(), b.n());
}

// what holds for every plan: each family in exactly one group, the descriptor array grouped as cls_first / cls_count say, the
// rounds a partition of the workgroup descriptors with at most `cus` workgroups each, the streams of the join
static void check_shape(const Batch &b, const FamilyPlan &pl, int cus)
{
  const int n = b.n();
  int cnt[RAMX_NGROUP] = { 0 }, n_dev = 0, n_cp = 0;
  CHECK((int)pl.grp.size() == n);
  for (int f = 0; f < n; f++)
  {
    CHECK(pl.grp[f] >= -1 && pl.grp[f] < RAMX_NGROUP);
    if (pl.grp[f] < 0) n_dev++; else cnt[pl.grp[f]]++;
    if (pl.grp[f] >= 0 && pl.grp[f] < NC) n_cp++;
  }
  CHECK(n_dev == pl.n_dev && n_cp == pl.n_cp && pl.cls_first[0] == 0 && pl.cls_first[RAMX_NGROUP] == n - n_dev && (int)pl.fam.size() == n - n_dev);
  std::vector<int> seen((size_t)n, 0);
  for (int c = 0; c < RAMX_NGROUP; c++)
  {
    CHECK(pl.cls_count[c] == cnt[c] && pl.cls_first[c + 1] == pl.cls_first[c] + cnt[c]);
    for (int i = pl.cls_first[c]; i < pl.cls_first[c + 1] && i < (int)pl.fam.size(); i++)
    {
      const FamDesc &x = pl.fam[(size_t)i];
      CHECK(x.id >= 0 && x.id < n);
      if (x.id < 0 || x.id >= n) continue;
      CHECK(pl.grp[x.id] == c && x.tile0 == b.first[x.id] / 64 && x.nx == b.count[x.id] && x.ntiles == (x.nx + 63) / 64);
      CHECK(i == pl.cls_first[c] || pl.fam[(size_t)i - 1].id < x.id);
      seen[(size_t)x.id]++;
    }
    if (c < NC && cnt[c]) CHECK(pl.cp_k[c] > 1 && pl.cp_threads[c] >= 64 && pl.cp_k[c] * b.count[pl.fam[(size_t)pl.cls_first[c]].id] <= pl.cp_threads[c]);
  }
  for (int f = 0; f < n; f++) CHECK(seen[(size_t)f] == (pl.grp[f] >= 0 ? 1 : 0));
  // the device-wide part
  int at = 0;
  for (const int2 &ro : pl.rounds) { CHECK(ro.x == at && ro.y > 0 && ro.y <= cus); at += ro.y; }
  CHECK(at == (int)pl.dev.size() && (pl.n_dev > 0) == !pl.rounds.empty());
  int vs = -1, last = -1;
  for (size_t i = 0; i < pl.dev.size(); i++)
  {
    const CpDevDesc &x = pl.dev[i];
    if (x.b == 0) { vs++; CHECK(x.id > last); last = x.id; }
    CHECK(x.b >= 0 && x.b < x.nb && x.vs == vs && x.id == last && x.id >= 0 && x.id < n);
    if (x.id < 0 || x.id >= n) continue;
    CHECK(pl.grp[x.id] == -1 && x.first == b.first[x.id] && x.nx == b.count[x.id]);
    CHECK(i + (size_t)(x.nb - x.b) <= pl.dev.size() && (x.b == 0 || pl.dev[i - 1].b == x.b - 1));
  }
  CHECK(vs + 1 == pl.n_dev && (pl.n_dev == 0 || (pl.dev_k > 1 && pl.dev_threads >= 64)));
  // the streams of the join
  for (int c = 0; c < RAMX_NGROUP; c++)
  {
    bool want = cnt[c] > 0;
    if (pl.resident && (c == NC || c == NC + 1)) want = false;
    if (pl.resident && c == NC + 2) want = cnt[NC] + cnt[NC + 1] + cnt[NC + 2] > 0;
    if (c == RAMX_NGROUP - 1 && pl.n_dev > 0) want = true;
    CHECK(pl.launched[c] == want);
  }
}

int main()
{
  for (int c = 0; c < RAMX_NCLASS; c++)
    for (int k = 0; k < 4; k++) g_tab[c][k] = (c < 8 && (c & 3) == k) ? 10 : -8;
  for (const char *v : { "RAMX_NO_PERSISTENT", "RAMX_NO_PEER", "RAMX_NO_PK_MULTI", "RAMX_NO_CP_DEVICE", "RAMX_CP_K", "RAMX_CP_DEVICE_MAXN", "RAMX_NO_PK",
                         "RAMX_NO_CP", "RAMX_CP_DEV_THREADS", "RAMX_CP_NO_VOTE_WAVE" })
    unsetenv(v);
  const std::vector<int> edges = { 0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512 };
  const Batch eb = batch_of(edges);
  {
    // W = 40, an ordinary system: the classes change at 16/17, 32/33, 64/65, 128/129; above 256 flanks several workgroups
    const int want[13] = { NC, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, -1, -1 };
    const FamilyPlan pl = plan(eb);
    check_shape(eb, pl, 256);
    for (int f = 0; f < 13; f++) CHECK(pl.grp[f] == want[f]);
    const int k[5] = { 16, 16, 8, 4, 2 };
    for (int c = 0; c < 5; c++) CHECK(pl.cp_k[c] == k[c] && pl.cp_threads[c] == (c ? 512 : 256));
    CHECK(pl.resident && !pl.chain && pl.n_cp == 10 && pl.n_dev == 2 && pl.dev_k > 1 && pl.rounds.size() == 1);
    Case c; c.allow_dev = false;
    const FamilyPlan p2 = plan(eb, c);
    check_shape(eb, p2, 256);
    for (int f = 0; f < 13; f++) CHECK(p2.grp[f] == (want[f] < 0 ? NC + 3 : want[f]));
    CHECK(p2.n_dev == 0 && p2.dev.empty() && p2.n_cp == 10);
  }
  {
    // W = 80: no two lanes per flank (blocks of 81 cells), one workgroup takes 128 flanks, 129 go device-wide
    Case c; c.W = 80;
    const int want[13] = { NC, 0, 0, 1, 1, 2, 2, 3, 3, -1, -1, -1, -1 };
    const FamilyPlan pl = plan(eb, c);
    check_shape(eb, pl, 256);
    for (int f = 0; f < 13; f++) CHECK(pl.grp[f] == want[f]);
    CHECK(!pl.resident && pl.cls_count[4] == 0 && pl.n_dev == 4);
  }
  {
    setenv("RAMX_CP_K", "2", 1);
    const FamilyPlan pl = plan(eb);
    check_shape(eb, pl, 256);
    for (int f = 1; f <= 10; f++) CHECK(pl.grp[f] == 4);
    CHECK(pl.grp[0] == NC && pl.cp_k[4] == 2 && pl.n_cp == 10 && (pl.n_dev == 0 || pl.dev_k == 2));
    unsetenv("RAMX_CP_K");
  }
  {
    // one flank that starts behind the core edge: its family alone leaves the cell-parallel kernels
    Batch b = batch_of({ 20, 20, 300, 300 });
    b.fl[(size_t)b.first[1] + 7].t_lo = 1;
    b.fl[(size_t)b.first[3] + 299].t_lo = 5;
    b.fl[(size_t)b.first[0] + 3].t_lo = 9; b.fl[(size_t)b.first[0] + 3].t_hi = 8;      // (empty: fits)
    const FamilyPlan pl = plan(b);
    check_shape(b, pl, 256);
    CHECK(pl.grp[0] == 1 && pl.grp[1] == NC && pl.grp[2] == -1 && pl.grp[3] == NC + 3);
  }
  {
    // what switches the kernels of the whole batch
    struct { const char *what; int W, go, ge; bool force; const char *env; int cus; bool allow; bool resident, chain, cp, dev; } t[] = {
      { "plain", 40, -30, -5, false, NULL, 256, true, true, false, true, true },
      { "W = 9", 9, -30, -5, false, NULL, 256, true, false, false, false, false },
      { "go = 1", 40, 1, -5, false, NULL, 256, true, false, true, false, false },
      { "ge = 1", 40, -30, 1, false, NULL, 256, true, false, true, false, false },
      { "go + ge = -32768", 40, -32000, -768, false, NULL, 256, true, true, false, false, false },       // (scores past the packed keys)
      { "go + ge = -32769", 40, -32000, -769, false, NULL, 256, true, false, false, false, false },
      { "force_chain", 40, -30, -5, true, NULL, 256, true, false, true, false, false },
      { "RAMX_NO_CP", 40, -30, -5, false, "RAMX_NO_CP", 256, true, true, false, false, false },
      { "RAMX_NO_PERSISTENT", 40, -30, -5, false, "RAMX_NO_PERSISTENT", 256, true, false, false, true, false },
      { "RAMX_NO_CP_DEVICE", 40, -30, -5, false, "RAMX_NO_CP_DEVICE", 256, true, true, false, true, false },
      { "cus = 0", 40, -30, -5, false, NULL, 0, true, true, false, true, false },
      { "allow_dev = false", 40, -30, -5, false, NULL, 256, false, true, false, true, false },
    };
    for (const auto &x : t)
    {
      if (x.env) setenv(x.env, "1", 1);
      Case c; c.W = x.W; c.go = x.go; c.ge = x.ge; c.force_chain = x.force; c.cus = x.cus; c.allow_dev = x.allow;
      const FamilyPlan pl = plan(eb, c);
      if (x.env) unsetenv(x.env);
      check_shape(eb, pl, x.cus);
      const bool ok = pl.resident == x.resident && pl.chain == x.chain && pl.n_cp == (x.cp ? 10 : 0) && pl.n_dev == (x.dev ? 2 : 0);
      if (!ok) fprintf(stderr, "%s: resident %d chain %d n_cp %d n_dev %d\n", x.what, pl.resident, pl.chain, pl.n_cp, pl.n_dev);
      CHECK(ok);
    }
  }
  {
    // the shape rule: the first device-wide family fixes (lanes, threads, vote wave); a later family whose own plan differs stays
    // on its lane-per-flank shape -- two such sizes found with the plan function itself, on a device of a few CUs
    int found = 0;
    for (int cus : { 4, 8, 12, 16, 24 })
      for (int a = 257; a <= 512 && found < 3; a += 15)
        for (int b2 = a + 1; b2 <= 512 && found < 3; b2 += 17)
        {
          int k[2][2], th[2][2], nb[2][2], vw[2][2];
          for (int w = 0; w < 2; w++)
          {
            ramx_cp_device_plan(40, a, cus, w, &k[0][w], &th[0][w], &nb[0][w], &vw[0][w]);
            ramx_cp_device_plan(40, b2, cus, w, &k[1][w], &th[1][w], &nb[1][w], &vw[1][w]);
          }
          const int w = 2 * (k[0][0] > 0 ? nb[0][0] : 0) + (k[1][0] > 0 ? nb[1][0] : 0) > cus ? 1 : 0;      // (the batch below: a, b2, a)
          if (k[0][w] <= 0 || k[1][w] <= 0 || nb[0][w] > cus || nb[1][w] > cus) continue;
          if (k[0][w] == k[1][w] && th[0][w] == th[1][w] && vw[0][w] == vw[1][w]) continue;
          found++;
          Case c; c.cus = cus;
          const Batch b = batch_of({ a, b2, a });
          const FamilyPlan pl = plan(b, c);
          check_shape(b, pl, cus);
          CHECK(pl.grp[0] == -1 && pl.grp[1] == NC + 3 && pl.grp[2] == -1 && pl.n_dev == 2);
          CHECK(pl.dev_k == k[0][w] && pl.dev_threads == th[0][w] && pl.dev_vw == vw[0][w] && (int)pl.dev.size() == 2 * nb[0][w]);
        }
    CHECK(found > 0);
    // rounds: twenty families of 512 flanks need more workgroups than there are CUs
    Case c; c.cus = 64;
    const Batch b = batch_of(std::vector<int>(20, 512));
    const FamilyPlan pl = plan(b, c);
    check_shape(b, pl, 64);
    CHECK(pl.n_dev == 20 && pl.rounds.size() >= 2 && (int)pl.dev.size() > 64);
  }
  {
    // random batches
    std::mt19937 rng(12345);
    const int cuses[5] = { 0, 8, 64, 256, 304 }, widths[5] = { 40, 40, 14, 80, 9 };
    for (int it = 0; it < 300; it++)
    {
      std::vector<int> sizes((size_t)(1 + rng() % 40));
      for (int &s : sizes) s = rng() % 4 == 0 ? (int)(rng() % 513) : (int)(rng() % 80);
      Batch b = batch_of(sizes);
      for (int f = 0; f < b.n(); f++)
        if (b.count[f] > 0 && rng() % 8 == 0) b.fl[(size_t)b.first[f] + rng() % (unsigned)b.count[f]].t_lo = 1 + (int)(rng() % 5);
      Case c; c.cus = cuses[rng() % 5]; c.W = widths[rng() % 5]; c.allow_dev = rng() % 4 != 0; c.force_chain = rng() % 16 == 0;
      if (rng() % 8 == 0) c.go = 2;
      const FamilyPlan pl = plan(b, c);
      check_shape(b, pl, c.cus);
      const FamilyPlan none = plan(batch_of({}), c);
      CHECK(none.grp.empty() && none.fam.empty() && none.dev.empty() && none.n_cp == 0 && none.n_dev == 0);
    }
  }
  if (g_failed) return 1;
  printf("family_plan: ok\n");
  return 0;
}
