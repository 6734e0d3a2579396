// Backward of the per-channel DISTS statistics on caller-provided float32 NCHW maps for gfx950: the gradient of
// forward_from_feats (nerf_qa/DISTS_pytorch/DISTS_pt.py:181-202) with respect to the twelve feature maps, which the
// reference's no-reference models train through (nerf_qa/model_nr_v8.py:258-265).
//
//   stats_coef_kernel      one wave per (pair, global channel): folds the per-block fp64 partial sums that
//                          stats_nchw_kernel left in the forward's scratch into mx, my, vx, vy, cov, and, with the
//                          upstream dL/dS1, dL/dS2, into six fp64 numbers per plane
//   stats_grad_kernel      all six taps in one launch: gx = ox + a (x - mx) + b (y - my), gy = oy + a (y - my) + b (x - mx)
//
// With S1 = (2 mx my + c1) / (mx^2 + my^2 + c1), S2 = (2 cov + c2) / (vx + vy + c2), vx = E[x^2] - mx^2 and
// cov = E[xy] - mx my (the forward's own expressions, finalize_kernel):
//   a = 2 g2 dS2/dv / N,  b = g2 dS2/dcov / N,  ox = g1 dS1/dmx / N,  oy = g1 dS1/dmy / N.
// For a near-identical pair the two S2 terms (a ~ -b) cancel to a small remainder; the centring and the affine
// combination are therefore fp64 and rounded to float once, so the remainder keeps float accuracy whatever N.
// No atomics: every output element is written by exactly one thread, so results are bitwise repeatable.
#include <string.h>

#include "nqa_common.h"

namespace nqa {

// coefficient record of one (pair, channel) plane: {mx, my, a, b, ox, oy}
#define NQA_COEF 6

// grid (cdiv(ctot, 4), B), 256 threads.  coef: tap k's planes start at B * coff[k]; plane b * C[k] + c.
__global__ __launch_bounds__(256) void stats_coef_kernel(const double *__restrict__ part, StageDesc d,
                                                         const float *__restrict__ g_s1, const float *__restrict__ g_s2,
                                                         double *__restrict__ coef) {
  const int b = blockIdx.y, B = gridDim.y;
  const int lane = threadIdx.x & 63;
  const int gc = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gc >= d.ctot) return;
  const PlaneMoments m = plane_moments(part, d, b, gc, lane);  // (finalize_kernel's own fold)
  if (lane) return;
  const int k = m.k, c = m.c;
  const double inv = m.inv, mx = m.mx, my = m.my, vx = m.vx, vy = m.vy, cov = m.cov;
  const double c1 = 1e-6, c2 = 1e-6;
  const double n1 = 2.0 * mx * my + c1, d1 = mx * mx + my * my + c1;
  const double ds1_dmx = (2.0 * my * d1 - 2.0 * mx * n1) / (d1 * d1);
  const double ds1_dmy = (2.0 * mx * d1 - 2.0 * my * n1) / (d1 * d1);
  const double n2 = 2.0 * cov + c2, d2 = vx + vy + c2;
  const double ds2_dcov = 2.0 / d2, ds2_dv = -n2 / (d2 * d2);
  const double g1 = g_s1[(size_t)b * d.ctot + gc], g2 = g_s2[(size_t)b * d.ctot + gc];
  double *o = coef + ((size_t)B * d.coff[k] + (size_t)b * d.c[k] + c) * NQA_COEF;
  o[0] = mx;
  o[1] = my;
  o[2] = 2.0 * g2 * ds2_dv * inv;
  o[3] = g2 * ds2_dcov * inv;
  o[4] = g1 * ds1_dmx * inv;
  o[5] = g1 * ds1_dmy * inv;
}

// What stats_grad_kernel needs of the six taps.  Tap k owns blocks [blk0[k], blk0[k+1]) (none when it has no
// gradient to write); each block covers STATS_GRAD_UNITS consecutive units of the tap's (B * C * HW) elements, a unit
// being 4 floats (vec[k]: HW % 4 == 0 and every pointer 16-byte aligned) or 1.
#define STATS_GRAD_VPT 4
#define STATS_GRAD_UNITS (256 * STATS_GRAD_VPT)
struct StatsGradDesc {
  const float *x[NQA_NUM_TAPS], *y[NQA_NUM_TAPS];
  float *gx[NQA_NUM_TAPS], *gy[NQA_NUM_TAPS];
  long units[NQA_NUM_TAPS];    // units of the tap
  long coef_off[NQA_NUM_TAPS];  // first plane record of the tap (B * coff[k])
  int hw[NQA_NUM_TAPS];
  int vec[NQA_NUM_TAPS];
  int blk0[NQA_NUM_TAPS + 1];
};

__global__ __launch_bounds__(256) void stats_grad_kernel(StatsGradDesc d, const double *__restrict__ coef) {
  const int blk = blockIdx.x;
  int k = 0;
  while (k + 1 < NQA_NUM_TAPS && blk >= d.blk0[k + 1]) ++k;
  const int hw = d.hw[k];
  const int W = d.vec[k] ? 4 : 1;
  const long u0 = (long)(blk - d.blk0[k]) * STATS_GRAD_UNITS;
  const long e0 = u0 * W;               // first element of the block
  const long plane0 = e0 / hw;          // (one 64-bit division per block)
  const long r0 = e0 - plane0 * hw;     // e0's offset inside that plane
  const float *__restrict__ X = d.x[k];
  const float *__restrict__ Y = d.y[k];
  float *__restrict__ GX = d.gx[k];
  float *__restrict__ GY = d.gy[k];
  const double *__restrict__ cf = coef + d.coef_off[k] * NQA_COEF;
  const long units = d.units[k];
  if (W == 4) {
    f32x4 xv[STATS_GRAD_VPT], yv[STATS_GRAD_VPT];
#pragma unroll
    for (int v = 0; v < STATS_GRAD_VPT; ++v) {  // all loads first
      const long u = u0 + v * 256 + threadIdx.x;
      if (u < units) {
        xv[v] = *reinterpret_cast<const f32x4 *>(X + u * 4);
        yv[v] = *reinterpret_cast<const f32x4 *>(Y + u * 4);
      }
    }
#pragma unroll
    for (int v = 0; v < STATS_GRAD_VPT; ++v) {
      const long u = u0 + v * 256 + threadIdx.x;
      if (u >= units) continue;
      const unsigned rel = (unsigned)(r0 + (u - u0) * 4);  // < HW + 4 * STATS_GRAD_UNITS
      const double *q = cf + (plane0 + rel / (unsigned)hw) * NQA_COEF;  // (a unit never straddles two planes: HW % 4 == 0)
      const double mx = q[0], my = q[1], a = q[2], b = q[3], ox = q[4], oy = q[5];
      f32x4 gx, gy;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double dx = (double)xv[v][j] - mx, dy = (double)yv[v][j] - my;
        gx[j] = (float)fma(b, dy, fma(a, dx, ox));
        gy[j] = (float)fma(b, dx, fma(a, dy, oy));
      }
      if (GX) *reinterpret_cast<f32x4 *>(GX + u * 4) = gx;
      if (GY) *reinterpret_cast<f32x4 *>(GY + u * 4) = gy;
    }
  } else {
#pragma unroll
    for (int v = 0; v < STATS_GRAD_VPT; ++v) {
      const long u = u0 + v * 256 + threadIdx.x;
      if (u >= units) continue;
      const unsigned rel = (unsigned)(r0 + (u - u0));
      const double *q = cf + (plane0 + rel / (unsigned)hw) * NQA_COEF;
      const double dx = (double)X[u] - q[0], dy = (double)Y[u] - q[1];
      const double a = q[2], b = q[3];
      if (GX) GX[u] = (float)fma(b, dy, fma(a, dx, q[4]));
      if (GY) GY[u] = (float)fma(b, dx, fma(a, dy, q[5]));
    }
  }
}

// ---------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------
int stats_coef(const double *part, const StageDesc &d, int B, const float *g_s1, const float *g_s2, double *coef,
               hipStream_t st) {
  dim3 grid(cdiv(d.ctot, 4), B);
  TimedLaunch t(NQA_K_STATS, st);
  stats_coef_kernel<<<grid, 256, 0, st>>>(part, d, g_s1, g_s2, coef);
  return check_launch("stats_coef");
}

int stats_grad(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B,
               const int C[NQA_NUM_TAPS], const int HW[NQA_NUM_TAPS], const double *coef, float *const gx[NQA_NUM_TAPS],
               float *const gy[NQA_NUM_TAPS], hipStream_t st) {
  StatsGradDesc d;
  memset(&d, 0, sizeof(d));
  long coff = 0;
  int nblk = 0;
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    const long elems = (long)B * C[k] * HW[k];
    const uintptr_t al = (uintptr_t)fx[k] | (uintptr_t)fy[k] | (uintptr_t)gx[k] | (uintptr_t)gy[k];
    d.x[k] = fx[k];
    d.y[k] = fy[k];
    d.gx[k] = gx[k];
    d.gy[k] = gy[k];
    d.vec[k] = (HW[k] % 4 == 0 && (al & 15) == 0) ? 1 : 0;
    d.units[k] = d.vec[k] ? elems / 4 : elems;
    d.coef_off[k] = coff;
    d.hw[k] = HW[k];
    d.blk0[k] = nblk;
    if (gx[k] || gy[k]) nblk += (int)((d.units[k] + STATS_GRAD_UNITS - 1) / STATS_GRAD_UNITS);
    coff += (long)B * C[k];
  }
  d.blk0[NQA_NUM_TAPS] = nblk;
  if (!nblk) return NQA_OK;
  TimedLaunch t(NQA_K_STATS, st);
  stats_grad_kernel<<<nblk, 256, 0, st>>>(d, coef);
  return check_launch("stats_grad");
}

}  // namespace nqa
