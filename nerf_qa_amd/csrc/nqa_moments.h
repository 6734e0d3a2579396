// Statistics accumulation shared by the NHWC statistics kernels (nqa_pool_stats.hip: pairs; nqa_group_stats.hip: one
// reference against its K renders).  Device code only.
#pragma once
#include "nqa_common.h"

namespace nqa {

// The reference takes the variance by a second pass over (f - mean)
// (DISTS_pt.py:137-138); a one-pass sum of f^2 in fp32 would cancel catastrophically for a
// channel whose spread is small next to its mean.  Each thread therefore accumulates SHIFTED
// moments in fp32 -- sum(f-p), sum((f-p)^2), sum((fx-px)(fy-py)) with the pivot p = the
// thread's first sample of that channel, so the sums are of the order of the variance -- and
// converts them to raw fp64 sums once, at the end; block partials and the final combine are
// fp64.  Every feature byte is read once and the error stays relative to the variance.
typedef __attribute__((ext_vector_type(2))) float f32x2;

template <int N>
struct ShiftedMoments {  // N channels held as N/2 float pairs, so every update is packed (v_pk_*_f32)
  f32x2 px[N / 2], py[N / 2];  // pivots
  f32x2 s1x[N / 2], s1y[N / 2], s2x[N / 2], s2y[N / 2], sxy[N / 2];
  int n;
  __device__ inline void init() {
    n = 0;
#pragma unroll
    for (int e = 0; e < N / 2; ++e) px[e] = py[e] = s1x[e] = s1y[e] = s2x[e] = s2y[e] = sxy[e] = (f32x2){0.f, 0.f};
  }
  __device__ inline void add2(int e2, f32x2 x, f32x2 y) {
    const f32x2 dx = x - px[e2], dy = y - py[e2];
    s1x[e2] += dx;
    s1y[e2] += dy;
    s2x[e2] = dx * dx + s2x[e2];
    s2y[e2] = dy * dy + s2y[e2];
    sxy[e2] = dx * dy + sxy[e2];
  }
  // raw sum s of channel e, s = {sum x, sum y, sum x^2, sum y^2, sum xy}
  __device__ inline double raw(int e, int s) const {
    const int e2 = e >> 1, k = e & 1;
    const double p = px[e2][k], q = py[e2][k], nn = n, ax = s1x[e2][k], ay = s1y[e2][k];
    switch (s) {
      case 0: return ax + nn * p;
      case 1: return ay + nn * q;
      case 2: return (double)s2x[e2][k] + 2.0 * p * ax + nn * p * p;
      case 3: return (double)s2y[e2][k] + 2.0 * q * ay + nn * q * q;
      // the two cross terms are summed FIRST: each product of two floats is exact in fp64, so their sum rounds once,
      // the same way with x and y exchanged, and for y == x it is 2 p ax exactly -- sum xy is then sum x^2 bit for bit
      // (added one after the other to sxy, the last bit depended on which image was called x)
      default: return (double)sxy[e2][k] + (q * ax + p * ay) + nn * p * q;
    }
  }
};
// one loaded 16-byte channel group as float pairs
template <typename P, typename V>
__device__ inline void unpack2(const V &v, f32x2 (&out)[P::CPC / 2]) {
#pragma unroll
  for (int e = 0; e < P::CPC / 2; ++e) out[e] = (f32x2){P::to_f(v[2 * e]), P::to_f(v[2 * e + 1])};
}

// Block reduction of the per-thread raw sums over the pixel lanes -> part[(b*nblk+blk)*C*5 ...].
template <int CPC>
__device__ inline void reduce_store(const ShiftedMoments<CPC> &m, double *red, int tid, int G, int PL, int C,
                                    double *dst) {
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < CPC; ++e) red[tid * CPC + e] = m.raw(e, s);
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
      const int cg = c / CPC, ce = c % CPC;
      double sum = 0.0;
      for (int q = 0; q < PL; ++q) sum += red[(q * G + cg) * CPC + ce];
      dst[(size_t)c * 5 + s] = sum;
    }
  }
}

}  // namespace nqa
