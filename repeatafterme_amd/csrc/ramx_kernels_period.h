// ramx_kernels_period.h -- tandem periodicity of the extended copies (include/ramx.h, ramx_period): for every segment the best
// tract of 8-base blocks over every period p, the ungapped local self-alignment on every diagonal of the segment's dot plot
// (device code of libramx; included by ramx_period.hip only).
//
// The segments were packed as flanks (W = 0: eight 4-bit classes a word, transposed: word k of 64 segments is 256 contiguous
// bytes).  Two kernels:
//   ramx_period_squeeze_kernel: one wave per tile of 64 segments, a lane per segment.  A lane reads its window word by word
//   (the wave reads the rows coalesced) and writes its segment's own contiguous stream: four window words become one 64-bit word
//   of two bits a base and 32 validity bits.  Words behind the window are written as "no base", so a stream is SW words whatever
//   the segment's length.
//   ramx_period_scan_kernel: one workgroup per segment.  It stages the stream in LDS (the validity bits spread to the even bits,
//   so that both streams shift alike; 16 bytes per 32 bases, 32 KiB at the length limit) and gives the periods to the threads:
//   thread j takes p = 1 + j, 1 + j + 256, ...  For its period a thread walks the segment 32 bases a step: the word at offset
//   32 w is the same for every lane (one LDS address), the word at 32 w + p is a funnel shift of two neighbouring words by a
//   lane-dependent amount (neighbouring lanes read the same or the next LDS word); a xor folded to a bit per base and the two
//   validity masks give the agreeing and disagreeing pairs, four popcount pairs their numbers per block of eight, and the scan
//   of the contract runs over the blocks.  Pairs that do not exist need no mask: offset j + p >= n is "no base" in the stream.
//   A thread keeps its best tract; the candidates of a workgroup are ordered by ONE key (score, then the smaller period -- within
//   a period the scan itself orders them), reduced as a maximum through LDS, and the thread that holds it writes the record with
//   two 16-byte stores.  No atomics, no scratch, and no order of evaluation shows.
#pragma once

#include "ramx_period_api.h"
#include "ramx_kernels_squeeze.h"       // tsd_squeeze

static_assert(sizeof(ramx_period) == 32, "ramx_period is 8 words");
static_assert(RAMX_PERIOD_LEN_MAX <= 65536 && RAMX_PERIOD_PMAX <= 8192, "the key holds a score of 16 bits above a period of 13");

// bit 3 of eight 4-bit fields clear -> eight bits: bit i set iff the class of field i is below 8 (a base)
__device__ __forceinline__ unsigned period_valid8(unsigned a)
{
  unsigned v = (~a >> 3) & 0x11111111u;
  v = (v | (v >> 3)) & 0x03030303u;
  v = (v | (v >> 6)) & 0x000f000fu;
  return (v | (v >> 12)) & 0xffu;
}
// sixteen bits -> the even bits of 32
__device__ __forceinline__ unsigned period_spread16(unsigned x)
{
  x &= 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}

__global__ __launch_bounds__(64) void ramx_period_squeeze_kernel(const PeriodArgs pa)
{
  const int seg = blockIdx.x * 64 + threadIdx.x;                 // < Np
  const unsigned *win = pa.win + seg;
  unsigned long long *bs = pa.bases + (size_t)seg * pa.SW;
  unsigned *vs = pa.valid + (size_t)seg * pa.SW;
  for (int w = 0; w < pa.SW; w++)
  {
    unsigned long long b = 0;
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
      const int k = 1 + 4 * w + i;                               // word 0 is the pad word in front of the segment
      const unsigned a = k < pa.KW ? win[(size_t)k * pa.Np] : 0x88888888u;
      b |= (unsigned long long)tsd_squeeze(a) << (16 * i);
      v |= period_valid8(a) << (8 * i);
    }
    bs[w] = b;
    vs[w] = v;
  }
}

__global__ __launch_bounds__(RAMX_PERIOD_THREADS) void ramx_period_scan_kernel(const PeriodArgs pa)
{
  extern __shared__ unsigned long long period_lds[];             // [nw + PAD] bases, then [nw + PAD] validity on the even bits
  __shared__ unsigned keys[RAMX_PERIOD_THREADS];
  const int seg = blockIdx.x, tid = threadIdx.x;                 // seg < n
  const int n = pa.len[seg], nw = (n + 31) >> 5, nl = nw + RAMX_PERIOD_PAD;      // nw <= SW
  unsigned long long *Lb = period_lds, *Lv = period_lds + nl;
  {
    const unsigned long long *bs = pa.bases + (size_t)seg * pa.SW;
    const unsigned *vs = pa.valid + (size_t)seg * pa.SW;
    for (int w = tid; w < nl; w += RAMX_PERIOD_THREADS)
    {
      unsigned long long b = 0, v = 0;
      if (w < nw)
      {
        b = bs[w];
        const unsigned vv = vs[w];
        v = (unsigned long long)period_spread16(vv) | ((unsigned long long)period_spread16(vv >> 16) << 32);
      }
      Lb[w] = b; Lv[w] = v;
    }
  }
  __syncthreads();
  const unsigned long long even = 0x5555555555555555ull;
  const int pm = pa.pmax < n - 1 ? pa.pmax : n - 1, mm = pa.mm;
  int best_s = 0, best_p = 0, best_b0 = 0, best_b1 = 0, best_a = 0;
  for (int p = 1 + tid; p <= pm; p += RAMX_PERIOD_THREADS)
  {
    const int words = (n - p + 31) >> 5, q0 = p >> 5, r = 2 * (p & 31);      // q0 + words <= nw: the reads end inside the padding
    unsigned long long lo_b = Lb[q0], lo_v = Lv[q0];
    int run = 0, run_b0 = 0, run_a = 0;
    for (int w = 0; w < words; w++)
    {
      const unsigned long long hi_b = Lb[q0 + w + 1], hi_v = Lv[q0 + w + 1];
      // the 32 bases at offsets 32 w + p .. (a shift by 64 - r in two steps: r may be 0)
      const unsigned long long B = (lo_b >> r) | ((hi_b << 1) << (63 - r)), VB = (lo_v >> r) | ((hi_v << 1) << (63 - r));
      const unsigned long long x = Lb[w] ^ B, both = Lv[w] & VB;
      const unsigned long long diff = (x | (x >> 1)) & even;
      const unsigned long long agr = both & ~diff, dis = both & diff;
      lo_b = hi_b; lo_v = hi_v;
#pragma unroll
      for (int k = 0; k < 4; k++)
      {
        const int a = __popc((unsigned)(agr >> (16 * k)) & 0xffffu), dd = __popc((unsigned)(dis >> (16 * k)) & 0xffffu);
        const int s = a - mm * dd, b = 4 * w + k;
        // (blocks behind the last pair score 0 and hold no pair: they record nothing)
        if (run <= 0) { run = s; run_b0 = b; run_a = a; } else { run += s; run_a += a; }
        if (run > best_s) { best_s = run; best_p = p; best_b0 = run_b0; best_b1 = b; best_a = run_a; }
      }
    }
  }
  // the contract's order across periods in one key: the larger score, then the smaller period (a thread's periods ascend and it
  // records on strict improvement only); 0: nothing found
  const unsigned key = best_s > 0 ? ((unsigned)best_s << 13) | (unsigned)(RAMX_PERIOD_PMAX - best_p) : 0u;
  keys[tid] = key;
  __syncthreads();
  for (int s = RAMX_PERIOD_THREADS / 2; s > 0; s >>= 1)
  {
    if (tid < s) { const unsigned o = keys[tid + s]; if (o > keys[tid]) keys[tid] = o; }
    __syncthreads();
  }
  const unsigned top = keys[0];
  const bool found = (int)(top >> 13) >= pa.min_score;            // (min_score >= 1: top == 0 is never found)
  int4 *rec = reinterpret_cast<int4 *>(pa.out + seg);
  if (!found)
  {
    if (tid == 0) { rec[0] = make_int4(0, 0, 0, 0); rec[1] = make_int4(0, 0, 0, 0); }
    return;
  }
  if (key != top) return;                                         // the periods differ between threads: one thread holds it
  const int last = n - best_p - 1, end = 8 * best_b1 + 7 < last ? 8 * best_b1 + 7 : last;
  rec[0] = make_int4(best_p, best_s, 8 * best_b0, end);
  rec[1] = make_int4(best_a, (best_a - best_s) / mm, 0, 0);
}
