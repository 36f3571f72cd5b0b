// Host-side memory safety of replay_plan (static in ramx_device.hip): the corner layouts of tests/test_gpu_replay_corners.py and
// the argument errors, on heap arrays of exactly the size the contract asks for, under ASan + UBSan.  Host code only: nothing
// here touches a GPU.  Built and run by tools/host_asan/run.sh.
#include "../../repeatafterme_amd/csrc/ramx_device.hip"

#include <cassert>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main()
{
  const int L = 30;
  ReplayPlan pl;
  // zero families over 128 padded flanks: no array is looked at
  CHECK(replay_plan("t", 128, NULL, NULL, 0, L, NULL, NULL, NULL, true, pl) == RAMX_OK);
  CHECK(pl.tiles == 2 && pl.maxrows == 0 && pl.tile_fam.size() == 2 && pl.tile_fam[0].x == -1 && pl.tile_fam[1].x == -1);
  // a family without flanks, alone over no flanks at all and behind another at fam_first == n_padded
  {
    std::vector<int8_t> cons((size_t)L, 2);
    std::vector<int32_t> first{0}, count{0}, rows{10};
    CHECK(replay_plan("t", 0, first.data(), count.data(), 1, L, cons.data(), rows.data(), NULL, true, pl) == RAMX_OK);
    CHECK(pl.tiles == 0 && pl.maxrows == 10 && pl.tile_fam.size() == 1 && pl.tile_fam[0].x == -1);
    CHECK(pl.fam_desc[0].x == 0 && pl.fam_desc[0].y == 0 && pl.fam_desc[0].z == 10);
  }
  {
    std::vector<int8_t> cons((size_t)2 * L, 1);
    std::vector<int32_t> first{0, 128}, count{70, 0}, rows{12, 10};
    CHECK(replay_plan("t", 128, first.data(), count.data(), 2, L, cons.data(), rows.data(), NULL, true, pl) == RAMX_OK);
    CHECK(pl.tiles == 2 && pl.maxrows == 12 && pl.tile_fam.size() == 2);
    CHECK(pl.tile_fam[0].x == 0 && pl.tile_fam[0].y == 64 && pl.tile_fam[1].x == 0 && pl.tile_fam[1].y == 6);
    CHECK(pl.fam_desc[1].x == 2 && pl.fam_desc[1].y == 0 && pl.fam_desc[1].z == 10);
    // the same layout with only the second family running: the first one's tiles belong to none, with and without the checks
    const char run[2] = {0, 1};
    for (int check = 0; check < 2; check++)
    {
      CHECK(replay_plan("t", 128, first.data(), count.data(), 2, L, cons.data(), rows.data(), run, check != 0, pl) == RAMX_OK);
      CHECK(pl.maxrows == 10 && pl.tile_fam[0].x == -1 && pl.tile_fam[1].x == -1 && pl.fam_desc[0].y == 0);
    }
  }
  // one thing wrong each: RAMX_ERR_ARG and its message, nothing read or written beyond the arrays
  struct { std::vector<int32_t> first, count, rows; int bad_base; const char *msg; } bad[] = {
    { {0, 64}, {70, 10}, {10, 10}, -1, "t: families 0 and 1 overlap" },
    { {0}, {70}, {L + 1}, -1, "t: rows[0] = 31 outside [0, L = 30]" },
    { {32}, {70}, {10}, -1, "t: bad family layout" },
    { {64}, {70}, {10}, -1, "t: bad family layout" },
    { {0}, {-1}, {10}, -1, "t: bad family layout" },
    { {0}, {70}, {10}, 3, "t: consensus base outside A C G T (family 0, column 3)" },
  };
  for (auto &b : bad)
  {
    const int nf = (int)b.first.size();
    std::vector<int8_t> cons((size_t)nf * L, 0);
    if (b.bad_base >= 0) cons[(size_t)b.bad_base] = 4;
    CHECK(replay_plan("t", 128, b.first.data(), b.count.data(), nf, L, cons.data(), b.rows.data(), NULL, true, pl) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), b.msg) == 0);
  }
  {
    std::vector<int32_t> first{0}, count{70}, rows{10};
    CHECK(replay_plan("t", 128, first.data(), count.data(), 1, L, NULL, rows.data(), NULL, true, pl) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), "t: cons missing") == 0);
  }
  printf("replay_plan: ok\n");
  return 0;
}
