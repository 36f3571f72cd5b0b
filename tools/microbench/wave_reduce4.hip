// wave_sum4_nonneg31 / wave_max4_i32 (four values reduced together: two v_permlane swaps, then four DPP steps inside the rows)
// against four wave_sum_nonneg31 / five wave_max_i32_dpp chains, as the packed-row kernel used them (ramx_kernels_common.h):
// every result compared on random and corner inputs, then both timed (s_memtime around a dependent chain of reductions,
// 1 and 2 waves per SIMD).
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -I include -I repeatafterme_amd/csrc tools/microbench/wave_reduce4.hip -o tools/microbench/wave_reduce4
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define RAMX_SECONDARY_TU 1
#include "ramx_kernels_common.h"

// in: [cases][4][64]; out: [cases][16] = old sums, new sums (long long), then [cases][8] old maxima, new maxima
__global__ void check_kernel(const int *in, long long *sums, int *maxs, int cases, int nonneg)
{
  const int lane = threadIdx.x & 63;
  for (int cs = blockIdx.x; cs < cases; cs += gridDim.x)
  {
    int v[4];
    for (int c = 0; c < 4; c++) v[c] = in[(cs * 4 + c) * 64 + lane];
    if (nonneg)
    {
      long long t[4];
      wave_sum4_nonneg31(v, t);
      for (int c = 0; c < 4; c++)
      {
        const long long o = wave_sum_nonneg31(v[c]);
        if (lane == 0) { sums[cs * 8 + c] = o; sums[cs * 8 + 4 + c] = t[c]; }
      }
    }
    int m[4];
    wave_max4_i32(v, m);
    for (int c = 0; c < 4; c++)
    {
      const int o = wave_max_i32_dpp(v[c]);
      if (lane == 0) { maxs[cs * 8 + c] = o; maxs[cs * 8 + 4 + c] = m[c]; }
    }
  }
}

// a chain of reductions, each fed by the one before (as the kernel's are by the row): WHICH 0 old sums, 1 new sums, 2 old maxima
// (four candidates + the shared deletion term), 3 new maxima
template <int WHICH>
__global__ void time_kernel(int *out, unsigned long long *cyc, int iters, int seed)
{
  const int lane = threadIdx.x & 63;
  int v[4], me = lane * 7 + seed;
  for (int c = 0; c < 4; c++) v[c] = ((lane * 2654435761u) >> (c + 3)) & 0x3fffffff;
  int acc = 0;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; it++)
  {
    if (WHICH == 0)
    {
      long long t[4];
      for (int c = 0; c < 4; c++) t[c] = wave_sum_nonneg31(v[c]);
      for (int c = 0; c < 4; c++) { acc += (int)t[c]; v[c] = (v[c] ^ (int)t[c]) & 0x3fffffff; }
    }
    if (WHICH == 1)
    {
      long long t[4];
      wave_sum4_nonneg31(v, t);
      for (int c = 0; c < 4; c++) { acc += (int)t[c]; v[c] = (v[c] ^ (int)t[c]) & 0x3fffffff; }
    }
    if (WHICH == 2)
    {
      const int mx = wave_max_i32_dpp(me);
      int b[4];
      for (int c = 0; c < 4; c++) b[c] = imax(wave_max_i32_dpp(v[c]), mx);
      for (int c = 0; c < 4; c++) { acc += b[c]; v[c] = (v[c] + b[c] + lane) & 0x3fffffff; }
      me = (me + b[0]) & 0x3fffffff;
    }
    if (WHICH == 3)
    {
      int b[4], w[4];
      for (int c = 0; c < 4; c++) w[c] = imax(v[c], me);
      wave_max4_i32(w, b);
      for (int c = 0; c < 4; c++) { acc += b[c]; v[c] = (v[c] + b[c] + lane) & 0x3fffffff; }
      me = (me + b[0]) & 0x3fffffff;
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc + v[0] + v[1] + v[2] + v[3];
  if (lane == 0) cyc[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main()
{
  // ---- inputs: corners first, then random -------------------------------------------------------
  std::vector<int> in;
  std::vector<int> nonneg_case;
  auto add_case = [&](const int (&v)[4][64], bool nn) { for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) in.push_back(v[c][l]); nonneg_case.push_back(nn); };
  int v[4][64];
  memset(v, 0, sizeof v); add_case(v, true);                                                        // all 0
  for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) v[c][l] = INT_MAX;
  add_case(v, true);                                                                                // all 2^31 - 1
  for (int one = 0; one < 64; one++)                                                                // one lane set, a different value per candidate
  {
    memset(v, 0, sizeof v);
    for (int c = 0; c < 4; c++) v[c][one] = INT_MAX - c * 1000003 - one;
    add_case(v, true);
  }
  memset(v, 0, sizeof v);
  for (int c = 0; c < 4; c++) { v[c][31] = 0x7fff0000 + c; v[c][32] = 0x0000ffff - c; v[c][63] = INT_MAX - 17 * c; }
  add_case(v, true);                                                                                // lanes 31 / 32 / 63
  for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) v[c][l] = INT_MIN;
  add_case(v, false);                                                                               // maxima: all INT_MIN
  for (int one = 0; one < 64; one += 7)
  {
    for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) v[c][l] = INT_MIN;
    for (int c = 0; c < 4; c++) v[c][(one + 16 * c) & 63] = INT_MIN + 1 + c;
    add_case(v, false);                                                                             // one lane just above INT_MIN
  }
  for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) v[c][l] = -1 - l * 33554432 / 64 * (c + 1);
  add_case(v, false);                                                                               // negative ramps
  srand(12345);
  auto rnd = []() { return (unsigned)rand() ^ ((unsigned)rand() << 11) ^ ((unsigned)rand() << 22); };
  for (int k = 0; k < 4000; k++)
  {
    const bool nn = (k & 1) == 0;
    const unsigned mask = (k % 5 == 0) ? 0xffffu : 0xffffffffu;                                      // some with small values only
    for (int c = 0; c < 4; c++) for (int l = 0; l < 64; l++) v[c][l] = nn ? (int)(rnd() & mask & 0x7fffffffu) : (int)rnd();
    add_case(v, nn);
  }
  const int cases = (int)nonneg_case.size();

  int *d_in, *d_max, *d_out; long long *d_sum; unsigned long long *d_cyc;
  CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_sum, (size_t)cases * 8 * 8)); CK(hipMalloc(&d_max, (size_t)cases * 8 * 4));
  CK(hipMalloc(&d_out, 1 << 20)); CK(hipMalloc(&d_cyc, 1 << 12));
  CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  std::vector<long long> hs((size_t)cases * 8);
  std::vector<int> hm((size_t)cases * 8);
  int bad = 0;
  // (every case goes through both kinds of reduction; the sums of a case with negative values mean nothing and are not compared)
  hipLaunchKernelGGL(check_kernel, dim3(64), dim3(64), 0, 0, d_in, d_sum, d_max, cases, 1);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(hs.data(), d_sum, hs.size() * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(hm.data(), d_max, hm.size() * 4, hipMemcpyDeviceToHost));
  for (int cs = 0; cs < cases; cs++)
    for (int c = 0; c < 4; c++)
    {
      long long s = 0; int m = INT_MIN;
      for (int l = 0; l < 64; l++) { const int x = in[((size_t)cs * 4 + c) * 64 + l]; s += x; m = x > m ? x : m; }
      if (nonneg_case[cs] && (hs[cs * 8 + c] != s || hs[cs * 8 + 4 + c] != s))
      { if (bad++ < 10) printf("SUM MISMATCH case %d value %d: host %lld old %lld new %lld\n", cs, c, s, hs[cs * 8 + c], hs[cs * 8 + 4 + c]); }
      if (hm[cs * 8 + c] != m || hm[cs * 8 + 4 + c] != m)
      { if (bad++ < 10) printf("MAX MISMATCH case %d value %d: host %d old %d new %d\n", cs, c, m, hm[cs * 8 + c], hm[cs * 8 + 4 + c]); }
    }
  printf("%d cases (%d corner, 4000 random) x 4 values: sums and maxima, old and new, against the host: %s\n", cases, cases - 4000, bad ? "MISMATCH" : "all equal");
  if (bad) return 1;

  // ---- timing -------------------------------------------------------------------------------------
  const int iters = 2000;
  const char *nm[4] = { "4 x wave_sum_nonneg31", "wave_sum4_nonneg31", "5 x wave_max_i32_dpp", "wave_max4_i32" };
  for (int which = 0; which < 4; which++)
  {
    printf("%-24s", nm[which]);
    for (int wps = 1; wps <= 2; wps++)
    {
      const int threads = 256 * wps;
      std::vector<unsigned long long> h(threads / 64);
      for (int rep = 0; rep < 2; rep++)
      {
        if (which == 0) hipLaunchKernelGGL(time_kernel<0>, dim3(1), dim3(threads), 0, 0, d_out, d_cyc, iters, 3);
        if (which == 1) hipLaunchKernelGGL(time_kernel<1>, dim3(1), dim3(threads), 0, 0, d_out, d_cyc, iters, 3);
        if (which == 2) hipLaunchKernelGGL(time_kernel<2>, dim3(1), dim3(threads), 0, 0, d_out, d_cyc, iters, 3);
        if (which == 3) hipLaunchKernelGGL(time_kernel<3>, dim3(1), dim3(threads), 0, 0, d_out, d_cyc, iters, 3);
        CK(hipDeviceSynchronize());
      }
      CK(hipMemcpy(h.data(), d_cyc, h.size() * 8, hipMemcpyDeviceToHost));
      unsigned long long mx = 0;
      for (auto x : h) if (x > mx) mx = x;
      printf("  %dw/SIMD: %7.1f ticks (s_memtime) per reduction of four", wps, (double)mx / iters);
    }
    printf("\n");
  }
  return 0;
}
