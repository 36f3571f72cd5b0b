// The route of a whole-set direction at the edges of its gates: route_gates and route_settle (static in ramx_device.hip), the
// part of direction_route that needs no device, under ASan + UBSan.  Host code only: nothing here touches a GPU (the occupancy
// answers route_settle reads are given by hand).  Built and run by tools/host_asan/run.sh.
#include "../../repeatafterme_amd/csrc/ramx_device.hip"

static int g_failed;      // (every edge is looked at: one wrong gate does not hide the next)
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); g_failed++; } } while (0)

struct Case
{
  int W = 14, go = -30, ge = -5, L = 200, Nx = 150, pk_r0 = 0, nranks = 1, cus = 256;
  bool flanks_ok = true, tracing = false, multi = false, peer_ready = false, force_chain = false;
};

static int g_tab[RAMX_NCLASS][4];

static DirRoute gates(const Case &c) { return route_gates(route_env(), c.W, c.go, c.ge, g_tab, c.L, c.Nx, c.pk_r0, c.flanks_ok, c.tracing, c.multi, c.peer_ready, c.nranks, c.force_chain, c.cus); }

// ... and with both lane-per-flank kernels co-resident (or not) where they are admissible
static DirRoute settled(const Case &c, bool resident32 = true, bool resident_pk = true)
{
  DirRoute rt = gates(c);
  if (rt.int32_can && resident32) { rt.block = 256; rt.blocks = 1; }
  if (rt.pk && resident_pk) { rt.pk_block = 320; rt.pk_blocks = 1; }
  route_settle(rt, route_env(), c.Nx);
  return rt;
}

static bool nothing_in_one_launch(const DirRoute &rt) { return !rt.int32_can && !rt.pk && !rt.cp_try && rt.k == 0; }

int main()
{
  for (int c = 0; c < RAMX_NCLASS; c++)
    for (int k = 0; k < 4; k++) g_tab[c][k] = (c < 8 && (c & 3) == k) ? 10 : -8;
  for (const char *v : { "RAMX_NO_PERSISTENT", "RAMX_NO_PEER", "RAMX_NO_PK_MULTI", "RAMX_NO_CP_DEVICE", "RAMX_CP_K", "RAMX_CP_DEVICE_MAXN", "RAMX_NO_PK",
                         "RAMX_NO_CP", "RAMX_CP_DEV_THREADS", "RAMX_CP_NO_VOTE_WAVE" })
    unsetenv(v);
  Case base;
  {
    // an ordinary system, 150 flanks: everything admissible, sixteen lanes per flank, and the cell-parallel kernel packs the rest
    DirRoute rt = settled(base);
    CHECK(rt.mailbox_ok && rt.int32_can && rt.pk && rt.pk_r0 == 0 && rt.cp_try && rt.k == 16 && rt.nb > 0 && rt.nb <= base.cus && rt.th > 0 && rt.pack_now);
    CHECK(rt.spread > 0 && rt.rebase > 0);
  }
  // go + ge = -32768 keeps the int32 rows, -32769 does not (neither takes the packed rows)
  { Case c; c.go = -32000; c.ge = -768; CHECK(gates(c).int32_can && !gates(c).pk); c.ge = -769; CHECK(!gates(c).int32_can && !gates(c).pk); }
  // a positive gap penalty: the full candidate recurrence, per column (multi-rank the cell-parallel agreement is still held)
  for (int which = 0; which < 2; which++)
  {
    Case c; (which ? c.ge : c.go) = 1;
    DirRoute rt = settled(c);
    CHECK(!rt.int32_can && !rt.pk && rt.k == 0 && rt.cp_try && rt.pack_now);
  }
  // band widths with and without an instantiation
  for (int W : { 14, 20, 40, 80, 7 })
  {
    Case c; c.W = W;
    DirRoute rt = settled(c);
    CHECK(rt.int32_can == (W != 7) && rt.pk == (W != 7) && (rt.k > 0) == (W != 7));
  }
  // L = 0: nothing to launch
  { Case c; c.L = 0; CHECK(nothing_in_one_launch(settled(c)) && settled(c).pk_r0 == -1 && settled(c).pack_now); }
  // two ranks: the mailboxes carry fewer than 65,536 rows; one GPU has no such limit
  {
    Case c; c.multi = true; c.peer_ready = true; c.nranks = 2; c.L = 65535;
    DirRoute rt = settled(c);
    CHECK(rt.mailbox_ok && rt.int32_can && rt.pk && rt.cp_try && rt.k == 16 && !rt.pack_now);      // (multi-rank: packed by whoever runs)
    c.L = 65536;
    CHECK(!gates(c).mailbox_ok && nothing_in_one_launch(settled(c)));
    c.multi = false;
    CHECK(gates(c).mailbox_ok && gates(c).int32_can && gates(c).cp_try);
    c.multi = true; c.L = 200; c.peer_ready = false;
    CHECK(nothing_in_one_launch(settled(c)));
    c.peer_ready = true; c.nranks = 1;
    CHECK(nothing_in_one_launch(settled(c)));
    // a rank without a flank of its own plans the agreed launch for one
    c.nranks = 2; c.Nx = 0;
    CHECK(gates(c).cp_try && gates(c).k == 16 && gates(c).nb == 1 && settled(c).pack_now);
    c.multi = false;
    CHECK(!gates(c).cp_try && gates(c).k == 0 && gates(c).int32_can);
  }
  // the first row of the packed kernel: none, 0, behind first rows on the int32 kernel (which must then be resident), past the end
  {
    Case c; c.flanks_ok = false; c.pk_r0 = -1;
    CHECK(!gates(c).pk && gates(c).int32_can && gates(c).k == 0 && gates(c).cp_try);
    c.flanks_ok = true; c.pk_r0 = 0;
    CHECK(settled(c, false, true).pk && !settled(c, false, true).int32_can && !settled(c, true, false).pk);
    c.pk_r0 = 14;
    CHECK(settled(c).pk && settled(c).pk_r0 == 14 && !settled(c, false, true).pk);
    c.pk_r0 = c.L - 1; CHECK(gates(c).pk);
    c.pk_r0 = c.L; CHECK(!gates(c).pk && gates(c).int32_can);
    c.pk_r0 = c.L + 50; CHECK(!gates(c).pk);
  }
  // a trace wants a launch per row; so does the forced full recurrence
  { Case c; c.tracing = true; CHECK(nothing_in_one_launch(settled(c)) && settled(c).pk_r0 == -1 && settled(c).tracing && settled(c).pack_now); }
  { Case c; c.force_chain = true; CHECK(nothing_in_one_launch(settled(c)) && settled(c).pk_r0 == -1); }
  // the switches, one at a time, on one GPU and on two ranks
  {
    Case one, two; two.multi = true; two.peer_ready = true; two.nranks = 2;
    setenv("RAMX_NO_PERSISTENT", "1", 1);
    CHECK(nothing_in_one_launch(settled(one)) && nothing_in_one_launch(settled(two)));
    unsetenv("RAMX_NO_PERSISTENT"); setenv("RAMX_NO_PEER", "1", 1);
    CHECK(settled(one).int32_can && settled(one).pk && settled(one).k == 16 && nothing_in_one_launch(settled(two)));
    unsetenv("RAMX_NO_PEER"); setenv("RAMX_NO_PK_MULTI", "1", 1);
    CHECK(settled(one).pk && !settled(two).pk && settled(two).int32_can && settled(two).k == 16);
    unsetenv("RAMX_NO_PK_MULTI"); setenv("RAMX_NO_CP_DEVICE", "1", 1);
    CHECK(!gates(one).cp_try && gates(one).k == 0 && settled(one).pk && !settled(one).pack_now && !gates(two).cp_try && settled(two).int32_can);
    unsetenv("RAMX_NO_CP_DEVICE"); setenv("RAMX_NO_PK", "1", 1);
    CHECK(!gates(one).pk && gates(one).int32_can && gates(one).k == 16);
    unsetenv("RAMX_NO_PK"); setenv("RAMX_NO_CP", "1", 1);
    CHECK(gates(one).cp_try && gates(one).k == 0 && gates(one).pk);
    unsetenv("RAMX_NO_CP"); setenv("RAMX_CP_DEVICE_MAXN", "149", 1);
    CHECK(gates(one).cp_try && gates(one).k == 0);
    setenv("RAMX_CP_DEVICE_MAXN", "150", 1);
    CHECK(gates(one).k == 16);
    unsetenv("RAMX_CP_DEVICE_MAXN");
  }
  // 50,000 flanks at W = 40: four lanes per flank need 391 workgroups, two need 196.  With two the packed rows go first where
  // they can run -- unless RAMX_CP_K asks for the lanes -- and begin_direction's first piece is all that is packed
  {
    Case c; c.W = 40; c.Nx = 50000; c.cus = 400;
    CHECK(gates(c).k == 4 && gates(c).nb == 391 && settled(c).k == 4 && settled(c).pack_now);
    c.cus = 256;
    CHECK(gates(c).k == 2 && gates(c).nb == 196 && settled(c).k == 0 && settled(c).pk && !settled(c).pack_now);
    CHECK(settled(c, true, false).k == 2 && settled(c, true, false).pack_now);
    setenv("RAMX_NO_PK", "1", 1);
    CHECK(settled(c).k == 2 && !settled(c).pk);
    unsetenv("RAMX_NO_PK"); setenv("RAMX_CP_K", "2", 1);
    CHECK(settled(c).k == 2 && settled(c).pk && settled(c).pack_now);
    c.cus = 400;
    CHECK(settled(c).k == 2);
    unsetenv("RAMX_CP_K");
    c.cus = 100;
    CHECK(gates(c).k == 0 && gates(c).cp_try && settled(c).pk);
  }
  // the class table itself: a matrix whose 36 entries [candidate][A C G T a c g t N] are pairwise distinct (the `distinct` system
  // of tests/class_table.py) through class_tab -- tab[class][candidate] = matrix[candidate][code(class)] -- entry by entry
  static const int distinct[4][RAMX_NCLASS] = { {  12, -18, -10, -21,   8, -16,  -8, -24, -1 }, { -19,  11, -20,  -7, -14,   7, -22,  -5,  2 },
                                                {  -6, -17,  10, -15,  -4, -25,   6, -12, -2 }, { -23,  -9, -13,   9, -26, -11,  -3,   5,  1 } };
  static int32_t matrix[100 * 100];
  for (int i = 0; i < 100 * 100; i++) matrix[i] = 1000 + i;      // (nothing outside [0..3] x {0..7, 99} may show in the table)
  for (int k = 0; k < 4; k++)
    for (int c = 0; c < RAMX_NCLASS; c++) matrix[k * 100 + (c == 8 ? 99 : c)] = distinct[k][c];
  ramx_params prm = {};
  prm.matrix = matrix;
  {
    class_tab(&prm, g_tab);
    static const int want[RAMX_NCLASS][4] = { { 12, -19, -6, -23 }, { -18, 11, -17, -9 }, { -10, -20, 10, -13 }, { -21, -7, -15, 9 },      // A C G T
                                              { 8, -14, -4, -26 }, { -16, 7, -25, -11 }, { -8, -22, 6, -3 }, { -24, -5, -12, 5 },          // a c g t
                                              { -1, 2, -2, 1 } };                                                                          // N
    for (int c = 0; c < RAMX_NCLASS; c++)
      for (int k = 0; k < 4; k++) CHECK(g_tab[c][k] == want[c][k]);
    DirRoute rt = settled(base);
    CHECK(rt.int32_can && rt.pk && rt.k == 16 && fast_pack_ok(g_tab, base.go, base.ge, base.L, base.W));
  }
  // one lone extreme entry -- in a lower-case class, in N, in an upper-case class: the int8 range closes the fast band and the
  // cell-parallel kernel wherever the entry sits, the packed rows' plan sees it as P or mn (admitted at W = 14, refused at
  // W = 80, where the table without it is admitted: tests/score_gates.py and tests/test_class_table_ref.py say the same)
  {
    static const int where[3][2] = { { 6, 2 }, { 8, 1 }, { 1, 1 } };
    static const int values[4] = { 127, 128, -128, -129 };
    Case wide; wide.W = 80;
    CHECK(gates(wide).pk && gates(wide).k > 0);
    for (int w = 0; w < 3; w++)
      for (int v = 0; v < 4; v++)
      {
        const int code = where[w][0] == 8 ? 99 : where[w][0], cand = where[w][1];
        const int32_t kept = matrix[cand * 100 + code];
        matrix[cand * 100 + code] = values[v];
        class_tab(&prm, g_tab);
        const bool int8 = values[v] >= -128 && values[v] <= 127;
        CHECK(g_tab[where[w][0]][cand] == values[v]);
        CHECK((fast_pack_ok(g_tab, base.go, base.ge, base.L, base.W) != 0) == int8);
        CHECK((ramx_cp_max_family(base.W, base.go, base.ge, g_tab, base.L) > 0) == int8);
        DirRoute rt = settled(base);
        CHECK(rt.int32_can && rt.pk && (rt.k == 16) == int8 && (rt.k == 0) == !int8);
        CHECK(!gates(wide).pk && gates(wide).int32_can && (gates(wide).k > 0) == int8);
        matrix[cand * 100 + code] = kept;
      }
    class_tab(&prm, g_tab);
  }
  if (g_failed) return 1;
  printf("route_gates: ok\n");
  return 0;
}
