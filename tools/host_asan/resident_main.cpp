// Host-side memory safety of the pure parts of the calls that answer from the resident planes (plane_list and upper_blocks,
// static in ramx_device.hip): a family's plane list at the edges of its contract, every refusal with its message, the planes'
// word offsets by enumeration, and the block lists of the Gram and the pair matrix, on heap arrays of exactly the size the
// contract asks for, under ASan + UBSan.  Host code only: nothing here touches a GPU.  Built and run by tools/host_asan/run.sh.
#include "../../repeatafterme_amd/csrc/ramx_device.hip"

#include <set>
#include <utility>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// the first P planes of a replay in (row, class) order, from plane `skip` on
static std::vector<ramx_plane> first_planes(int P, int skip = 0)
{
  std::vector<ramx_plane> v((size_t)P);
  for (int i = 0; i < P; i++) v[(size_t)i] = ramx_plane{ (skip + i) / RAMX_PLANE_CLASSES, (skip + i) % RAMX_PLANE_CLASSES };
  return v;
}

static int check_offsets(const ResidentFam &rf, const std::vector<ramx_plane> &pl, const std::vector<long long> &at, size_t at0)
{
  CHECK(at.size() == at0 + pl.size());
  for (size_t i = 0; i < pl.size(); i++)
    CHECK(at[at0 + i] == rf.base + ((long long)pl[i].row * 8 + pl[i].cls) * rf.tiles);
  return 0;
}

static int check_blocks(int f, int n, int side)
{
  std::vector<int4> block(1, make_int4(-7, -7, -7, -7));            // what is there stays
  upper_blocks(block, f, n, side);
  const int nb = (n + side - 1) / side;
  CHECK(block.size() == 1 + (size_t)nb * (nb + 1) / 2 && block[0].x == -7 && block[0].w == -7);
  std::set<std::pair<int, int>> seen;
  for (size_t i = 1; i < block.size(); i++)
  {
    CHECK(block[i].x == f && block[i].w == 0 && 0 <= block[i].y && block[i].y <= block[i].z && block[i].z < nb);
    CHECK(seen.insert(std::make_pair(block[i].y, block[i].z)).second);
  }
  return 0;
}

int main()
{
  const ResidentFam wide{ 300, 3, 128, 130, 4096 };                 // 2,400 planes of three words
  const ResidentFam no_tiles{ 300, 0, 320, 0, 11296 };
  const ResidentFam no_rows{ 0, 2, 0, 100, 0 };
  const ResidentFam far{ 40, 5, 384, 300, (1LL << 31) + 12345 };    // its planes begin beyond 2^31 words
  std::vector<long long> at;
  // P = 0, 1 and the limit, the list an array of exactly P planes; one more is refused for its number before the list is read
  for (int P : { 0, 1, 2048 })
    for (const ResidentFam *rf : { &wide, &no_tiles, &far })
    {
      if (P > rf->rows * RAMX_PLANE_CLASSES) continue;
      const std::vector<ramx_plane> pl = first_planes(P, 3);
      const size_t at0 = at.size();
      CHECK(plane_list("t", 1, *rf, P ? pl.data() : NULL, P, &at) == RAMX_OK);
      if (check_offsets(*rf, pl, at, at0)) return 1;
      CHECK(plane_list("t", 1, *rf, P ? pl.data() : NULL, P, NULL) == RAMX_OK && at.size() == at0 + (size_t)P);    // checked, not listed
    }
  {
    const std::vector<ramx_plane> pl = first_planes(2049);
    CHECK(plane_list("t", 3, wide, pl.data(), 2049, &at) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), "t: family 3: 2049 planes outside [0, 2048]") == 0);
    CHECK(plane_list("t", 3, wide, NULL, 2049, &at) == RAMX_ERR_ARG);                        // the number before the arguments
    CHECK(strcmp(ramx_last_error(), "t: family 3: 2049 planes outside [0, 2048]") == 0);
    CHECK(plane_list("t", 3, wide, NULL, -1, &at) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), "t: family 3: -1 planes outside [0, 2048]") == 0);
    CHECK(plane_list("t", 2, wide, NULL, 1, &at) == RAMX_ERR_ARG);                           // what the caller found wrong
    CHECK(strcmp(ramx_last_error(), "t: family 2: bad argument") == 0);
  }
  // a family without rows has no plane to ask for; without planes asked it passes
  {
    const size_t at0 = at.size();
    CHECK(plane_list("t", 0, no_rows, NULL, 0, &at) == RAMX_OK && at.size() == at0);
    const std::vector<ramx_plane> pl = first_planes(1);
    CHECK(plane_list("t", 0, no_rows, pl.data(), 1, &at) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), "t: family 0, plane 0: (row 0, class 0) outside the resident replay (0 rows, classes 0..7)") == 0);
  }
  // one thing wrong each, in the last plane of a heap array of exactly that many: range before order within a plane
  struct { std::vector<ramx_plane> pl; const char *msg; } bad[] = {
    { { { -1, 0 } }, "t: family 3, plane 0: (row -1, class 0) outside the resident replay (300 rows, classes 0..7)" },
    { { { 2, 6 }, { 300, 0 } }, "t: family 3, plane 1: (row 300, class 0) outside the resident replay (300 rows, classes 0..7)" },
    { { { 2, 6 }, { 2, -1 } }, "t: family 3, plane 1: (row 2, class -1) outside the resident replay (300 rows, classes 0..7)" },
    { { { 2, 6 }, { 2, 8 } }, "t: family 3, plane 1: (row 2, class 8) outside the resident replay (300 rows, classes 0..7)" },
    { { { 2, 6 }, { 2, 7 }, { 2, 7 } }, "t: family 3, plane 2: the planes are not strictly increasing in (row, class)" },
    { { { 2, 6 }, { 1, 7 } }, "t: family 3, plane 1: the planes are not strictly increasing in (row, class)" },
    { { { 2, 6 }, { 2, 5 } }, "t: family 3, plane 1: the planes are not strictly increasing in (row, class)" },
  };
  for (auto &b : bad)
  {
    CHECK(plane_list("t", 3, wide, b.pl.data(), (int)b.pl.size(), &at) == RAMX_ERR_ARG);
    CHECK(strcmp(ramx_last_error(), b.msg) == 0);
    CHECK(plane_list("t", 3, wide, b.pl.data(), (int)b.pl.size(), NULL) == RAMX_ERR_ARG);   // the same without the offsets
    CHECK(strcmp(ramx_last_error(), b.msg) == 0);
  }
  // every plane of the family beyond 2^31 words, in pieces, against the definition
  {
    const std::vector<ramx_plane> all = first_planes(far.rows * RAMX_PLANE_CLASSES);
    std::vector<long long> got;
    CHECK(plane_list("t", 0, far, all.data(), (int)all.size(), &got) == RAMX_OK);
    if (check_offsets(far, all, got, 0)) return 1;
    CHECK(got.front() == far.base && got.back() == far.base + (long long)(far.rows * 8 - 1) * far.tiles && got.front() > INT_MAX);
  }
  // the block lists: n on both sides of one and of two block sizes, nothing for n = 0
  for (int side : { RAMX_GRAM_BLOCK, RAMX_DIST_BLOCK, 3 })
    for (int n : { 0, 1, side - 1, side, side + 1, 2 * side - 1, 2 * side, 2 * side + 1, 2048 })
      if (check_blocks(5, n, side)) return 1;
  printf("resident: ok\n");
  return 0;
}
