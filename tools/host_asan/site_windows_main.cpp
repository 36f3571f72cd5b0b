// The window arithmetic of the site-window analyses (ramx_dev_tsd, ramx_dev_period, ramx_dev_term): window_flank against its
// definition by enumeration, check_sites at each of its edges and tile_group at the edges of its budget (all static in
// ramx_device.hip), under ASan + UBSan.  Host code only: nothing here touches a GPU.  Built and run by tools/host_asan/run.sh.
#include "../../repeatafterme_amd/csrc/ramx_device.hip"

static int g_failed;      // (every case is looked at: one wrong window does not hide the next)
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); g_failed++; } } while (0)

// the definition: t of [t_first, t_last] belongs to the window if and only if start + step * t lies inside the bounds
static bool window_is(long long start, int step, bool compl_, long long t_first, long long t_last, long long bound_lo, long long bound_hi)
{
  ramx_flank f, zero;
  memset(&f, 0x5a, sizeof(f));                  // (whatever was there is gone)
  window_flank(f, start, step, compl_, t_first, t_last, bound_lo, bound_hi);
  bool ok = f.start == start && f.step == step && (f.compl_ != 0) == compl_;
  long long any = 0;
  for (long long t = t_first; t <= t_last; t++)
  {
    const long long p = start + step * t;
    const bool in = bound_lo <= p && p <= bound_hi;
    any += in;
    ok = ok && in == (f.t_lo <= t && t <= f.t_hi);
  }
  // no t outside [t_first, t_last], and the empty window is the one the pack kernels know
  ok = ok && (any ? f.t_lo >= t_first && f.t_hi <= t_last && f.t_hi - f.t_lo + 1 == any : f.t_lo == 1 && f.t_hi == 0);
  // nothing else is set
  memset(&zero, 0, sizeof(zero));
  zero.start = f.start; zero.step = f.step; zero.compl_ = f.compl_; zero.t_lo = f.t_lo; zero.t_hi = f.t_hi;
  return ok && memcmp(&f, &zero, sizeof(f)) == 0;
}

static int sites_rc(ramx_tsd_site a, ramx_tsd_site b)
{
  const ramx_tsd_site s[2] = { a, b };
  return check_sites("site_windows", s, 2);
}

int main()
{
  // both steps; starts inside, at and beyond either bound; bounds that cut the low end, the high end, both, nothing and
  // everything (far away, or empty); t_first negative (the TSD's slack) and zero; t_last below t_first (no t at all)
  long long cases = 0, empty = 0, cut = 0;
  for (int step : { 1, -1 })
    for (long long bound_lo : { 90LL, 100LL, 120LL })
      for (long long bound_hi : { bound_lo - 1, bound_lo, 110LL, 140LL, 1000LL })
        for (long long start = 80; start <= 150; start++)
          for (long long t_first : { -7LL, 0LL })
            for (long long t_last : { -8LL, -1LL, 0LL, 5LL, 40LL })
            {
              CHECK(window_is(start, step, step < 0, t_first, t_last, bound_lo, bound_hi));
              ramx_flank f;
              window_flank(f, start, step, false, t_first, t_last, bound_lo, bound_hi);
              cases++;
              empty += f.t_lo > f.t_hi;
              cut += f.t_lo <= f.t_hi && (f.t_lo > t_first || f.t_hi < t_last);
            }
  CHECK(cases == 2 * 3 * 5 * 71 * 2 * 5 && empty > 1000 && cut > 1000 && cases - empty - cut > 1000);
  // at the ends of the range of positions nothing overflows (UBSan is the judge): the TSD's windows of a site that ends at
  // RAMX_TSD_POS_MAX or begins at -RAMX_TSD_POS_MAX, in bounds as wide as they may be; the period's window without bounds
  const long long M = RAMX_TSD_POS_MAX;
  CHECK(window_is(M + 1, 1, false, -7, 46, -M, M) && window_is(-M - 1, -1, false, -7, 46, -M, M));
  CHECK(window_is(M - 1, -1, false, -7, 46, -M, M) && window_is(-M + 1, 1, false, -7, 46, -M, M));
  CHECK(window_is(M + 1, 1, false, -7, 46, -M, -M) && window_is(-M - 1, -1, true, -7, 46, M, M));
  CHECK(window_is(-M, 1, false, 0, 65535, -M, M) && window_is(M - 65535, 1, false, 0, 65535, -M, M));
  {
    ramx_flank f;
    window_flank(f, M + 1, 1, false, -7, 46, -M, M);
    CHECK(f.t_lo == -7 && f.t_hi == -1);
    // the padding of a tile: the empty site has no window, whatever the analysis asks of it
    window_flank(f, NO_SITE.lo - 1, -1, false, -7, 46, NO_SITE.seq_lo, NO_SITE.seq_hi);
    CHECK(f.t_lo == 1 && f.t_hi == 0);
    window_flank(f, NO_SITE.hi + 1, 1, false, -7, 46, NO_SITE.seq_lo, NO_SITE.seq_hi);
    CHECK(f.t_lo == 1 && f.t_hi == 0);
    window_flank(f, NO_SITE.hi, -1, true, 0, -1, NO_SITE.seq_lo, NO_SITE.seq_hi);
    CHECK(f.t_lo == 1 && f.t_hi == 0 && f.compl_ == 1 && f.step == -1);
  }
  // the sites: seq_lo <= lo <= hi + 1, hi <= seq_hi, within +-RAMX_TSD_POS_MAX; each edge and the step past it
  const ramx_tsd_site good = { 10, 20, 0, 30 };
  CHECK(check_sites("site_windows", NULL, 0) == RAMX_OK && sites_rc(good, good) == RAMX_OK);
  CHECK(sites_rc(good, { 21, 20, 0, 30 }) == RAMX_OK && sites_rc(good, { 22, 20, 0, 30 }) == RAMX_ERR_ARG);          // lo <= hi + 1
  CHECK(sites_rc(good, { 10, 20, 10, 30 }) == RAMX_OK && sites_rc(good, { 10, 20, 11, 30 }) == RAMX_ERR_ARG);        // seq_lo <= lo
  CHECK(sites_rc(good, { 10, 20, 0, 20 }) == RAMX_OK && sites_rc(good, { 10, 20, 0, 19 }) == RAMX_ERR_ARG);          // hi <= seq_hi
  CHECK(sites_rc(good, { 10, 9, 10, 9 }) == RAMX_OK && sites_rc({ 10, 20, 0, 19 }, good) == RAMX_ERR_ARG);           // an empty site; the first one
  CHECK(sites_rc(good, { -M, M, -M, M }) == RAMX_OK);
  CHECK(sites_rc(good, { -M, M, -M - 1, M }) == RAMX_ERR_ARG && sites_rc(good, { -M, M, -M, M + 1 }) == RAMX_ERR_ARG);
  CHECK(strstr(ramx_last_error(), "site_windows: site 1:") != NULL);
  // the budget: one tile must fit, the group is what fits, at most all tiles; unset, 1 GiB
  {
    int group = -1;
    unsetenv("RAMX_TERM_BYTES");
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, 1000, &group) == RAMX_OK && group == 5);
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, (size_t)1 << 29, &group) == RAMX_OK && group == 2);
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, ((size_t)1 << 30) + 1, &group) == RAMX_ERR_UNSUPPORTED && group == 2);
    setenv("RAMX_TERM_BYTES", "2999", 1);
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, 1000, &group) == RAMX_OK && group == 2);
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, 2999, &group) == RAMX_OK && group == 1);
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, 3000, &group) == RAMX_ERR_UNSUPPORTED);
    setenv("RAMX_TERM_BYTES", "0", 1);                                         // (not a budget: the default)
    CHECK(tile_group("site_windows", "RAMX_TERM_BYTES", "things", 5, 3000, &group) == RAMX_OK && group == 5);
    unsetenv("RAMX_TERM_BYTES");
  }
  if (g_failed) return 1;
  printf("site windows: ok (%lld windows by enumeration)\n", cases);
  return 0;
}
