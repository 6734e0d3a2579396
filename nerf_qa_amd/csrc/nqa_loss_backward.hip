// DISTS as a LOSS (DISTS.forward(x, y, require_grad=True) inside an optimisation, nerf_qa/DISTS_pytorch/DISTS_pt.py:105-108)
// for gfx950: what the loss path of nerf_qa_amd/autograd.py needs beyond the chain kernels of nqa_backward.hip.
//
//   loss_stats_sums_kernel   the five fp64 sums behind DISTS_pt.py:131-139 of a pair of float NHWC taps, per block
//   loss_stats_fold_kernel   one wave per (pair, channel): folds them into S1 and S2 themselves (fp64, rounded to float once):
//                            the forward of a loss against a prepared target, whose partials the backward then starts from
//   loss_stats_coef_kernel   one wave per (pair, channel): folds them (plane_moments, the forward's own fold) into the
//                            six fp64 numbers {mx, my, a, b, ox, oy} of nqa_stats_backward.hip
//   loss_stats_grad_kernel   gx = (x > 0) * (ox + a (x - mx) + b (y - my)), gy likewise with x and y swapped: the affine
//                            map centred and combined in fp64 and rounded to float once, the tap's own ReLU folded in
//   loss_stats_grad_y_add_kernel   gy += that kernel's gy: the DISTS term of a tap gradient that already holds another
//                            metric's (the pair loss of nerf_qa_amd/pair.py), one float add on top of the same fp64 chain
//   absmax_partial_kernel    per (image, block) the largest |g| as its bit pattern (which orders like the value)
//   exponent_finish_kernel   per image: k with max|g| 2^k in [128, 256) (0 for a zero or non-finite maximum), and the
//                            running total of the chain
//   absmax_partial_half_kernel, exponent_finish_half_kernel   the same for the half gradient chain (grad_precision "f16"):
//                            half maps read as such, and k with max|g| 2^k in [8, 16)
//
// The statistics' gradient is the NHWC counterpart of stats_coef_kernel + stats_grad_kernel and keeps their arithmetic
// contract; the exponents replace the host's float(t.abs().max()) of autograd.pyramid_backward, so a loss step enqueues
// without a single device -> host read.  All of it is HBM-streaming code: 16-byte accesses per lane, one writer per
// output element, no atomics (bitwise repeatable), and no image of a batch ever meets another in one accumulation.
#include "nqa_common.h"

namespace nqa {

#define NQA_COEF 6  // coefficient record of one (pair, channel) plane: {mx, my, a, b, ox, oy} (nqa_stats_backward.hip)

// Thread layout shared by the sums and the gradient kernel: G = C / 4 channel groups of 16 bytes, PL = 256 / G pixels
// side by side; thread (pl, g) walks the pixels p_begin + pl, + PL, ... of the block's range with its four channels.

// grid (nblk, B).  part[((b * nblk + blk) * C + c) * 5 + s], s = {sum x, sum y, sum x^2, sum y^2, sum xy}.
__global__ __launch_bounds__(256) void loss_stats_sums_kernel(const float *__restrict__ tx, const float *__restrict__ ty,
                                                              int HW, int C, int ppb, double *__restrict__ part) {
  __shared__ double red[256 * 4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int G = C / 4, PL = 256 / G;
  const int g = tid % G, pl = tid / G;
  const int p_begin = blk * ppb;
  const int p_end = min(HW, p_begin + ppb);
  const float *px = tx + (size_t)b * HW * C + g * 4;
  const float *py = ty + (size_t)b * HW * C + g * 4;
  double s[5][4];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[q][e] = 0.0;
#pragma unroll 4
  for (int p = p_begin + pl; p < p_end; p += PL) {
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(px + (size_t)p * C);
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(py + (size_t)p * C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)xv[e], y = (double)yv[e];
      s[0][e] += x;
      s[1][e] += y;
      s[2][e] = fma(x, x, s[2][e]);
      s[3][e] = fma(y, y, s[3][e]);
      s[4][e] = fma(x, y, s[4][e]);
    }
  }
  // fold the PL pixel lanes of each channel group, in a fixed order
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid * 4 + e] = s[q][e];
    __syncthreads();
    if (pl == 0) {
      for (int j = 1; j < PL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[q][e] += red[(j * G + g) * 4 + e];
    }
    __syncthreads();
  }
  if (pl == 0) {
    double *o = part + (((size_t)b * nblk + blk) * C + g * 4) * 5;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int q = 0; q < 5; ++q) o[e * 5 + q] = s[q][e];
  }
}

// grid (cdiv(C, 4), B), 256 threads = 4 waves = 4 channels, laid out as loss_stats_coef_kernel.  s1 / s2 point at the tap's
// first column of pair 0; pair b's row starts s_stride floats further.  One writer per output, no atomics.
__global__ __launch_bounds__(256) void loss_stats_fold_kernel(const double *__restrict__ part, StageDesc d,
                                                              float *__restrict__ s1, float *__restrict__ s2, long s_stride) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= d.ctot) return;
  const PlaneMoments m = plane_moments(part, d, b, c, lane);
  if (lane) return;
  const double mx = m.mx, my = m.my, vx = m.vx, vy = m.vy, cov = m.cov;
  const double c1 = 1e-6, c2 = 1e-6;
  s1[(size_t)b * s_stride + c] = (float)((2.0 * mx * my + c1) / (mx * mx + my * my + c1));
  s2[(size_t)b * s_stride + c] = (float)((2.0 * cov + c2) / (vx + vy + c2));
}

// grid (cdiv(C, 4), B), 256 threads = 4 waves = 4 channels.  g_s1 / g_s2 point at the tap's first column of pair 0;
// pair b's row starts g_stride floats further.  coef: plane b * C + c.
__global__ __launch_bounds__(256) void loss_stats_coef_kernel(const double *__restrict__ part, StageDesc d,
                                                              const float *__restrict__ g_s1, const float *__restrict__ g_s2,
                                                              long g_stride, double *__restrict__ coef) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= d.ctot) return;
  const PlaneMoments m = plane_moments(part, d, b, c, lane);
  if (lane) return;
  const double inv = m.inv, mx = m.mx, my = m.my, vx = m.vx, vy = m.vy, cov = m.cov;
  const double c1 = 1e-6, c2 = 1e-6;
  const double n1 = 2.0 * mx * my + c1, d1 = mx * mx + my * my + c1;
  const double ds1_dmx = (2.0 * my * d1 - 2.0 * mx * n1) / (d1 * d1);
  const double ds1_dmy = (2.0 * mx * d1 - 2.0 * my * n1) / (d1 * d1);
  const double n2 = 2.0 * cov + c2, d2 = vx + vy + c2;
  const double ds2_dcov = 2.0 / d2, ds2_dv = -n2 / (d2 * d2);
  const double g1 = g_s1[(size_t)b * g_stride + c], g2 = g_s2[(size_t)b * g_stride + c];
  double *o = coef + ((size_t)b * d.ctot + c) * NQA_COEF;
  o[0] = mx;
  o[1] = my;
  o[2] = 2.0 * g2 * ds2_dv * inv;
  o[3] = g2 * ds2_dcov * inv;
  o[4] = g1 * ds1_dmx * inv;
  o[5] = g1 * ds1_dmy * inv;
}

// grid (nblk, B).  gx / gy: either may be null (nothing is computed for it).
__global__ __launch_bounds__(256) void loss_stats_grad_kernel(const float *__restrict__ tx, const float *__restrict__ ty,
                                                              int HW, int C, int ppb, const double *__restrict__ coef,
                                                              float *__restrict__ gx, float *__restrict__ gy) {
  const int tid = threadIdx.x;
  const int b = blockIdx.y, blk = blockIdx.x;
  const int G = C / 4, PL = 256 / G;
  const int g = tid % G, pl = tid / G;
  const int p_begin = blk * ppb;
  const int p_end = min(HW, p_begin + ppb);
  double mx[4], my[4], ca[4], cb[4], ox[4], oy[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double *q = coef + ((size_t)b * C + g * 4 + e) * NQA_COEF;
    mx[e] = q[0];
    my[e] = q[1];
    ca[e] = q[2];
    cb[e] = q[3];
    ox[e] = q[4];
    oy[e] = q[5];
  }
  const size_t base = (size_t)b * HW * C + g * 4;
#pragma unroll 4
  for (int p = p_begin + pl; p < p_end; p += PL) {
    const size_t at = base + (size_t)p * C;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(tx + at);
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(ty + at);
    f32x4 ux, uy;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double dx = (double)xv[e] - mx[e], dy = (double)yv[e] - my[e];
      ux[e] = xv[e] > 0.f ? (float)fma(cb[e], dy, fma(ca[e], dx, ox[e])) : 0.f;
      uy[e] = yv[e] > 0.f ? (float)fma(cb[e], dx, fma(ca[e], dy, oy[e])) : 0.f;
    }
    if (gx) *reinterpret_cast<f32x4 *>(gx + at) = ux;
    if (gy) *reinterpret_cast<f32x4 *>(gy + at) = uy;
  }
}

// grid (nblk, B), the plan and thread layout of loss_stats_grad_kernel.  gy += u, u the float that kernel writes for the y
// side (the same fp64 chain, rounded to float once, 0 where y <= 0), then ONE float add: a tap gradient that is already
// there (A-DISTS' for the same tap) takes the DISTS term without a pass of its own.  Each thread reads and writes its own
// 16 bytes of gy and nobody else's.
__global__ __launch_bounds__(256) void loss_stats_grad_y_add_kernel(const float *__restrict__ tx,
                                                                    const float *__restrict__ ty, int HW, int C, int ppb,
                                                                    const double *__restrict__ coef, float *__restrict__ gy) {
  const int tid = threadIdx.x;
  const int b = blockIdx.y, blk = blockIdx.x;
  const int G = C / 4, PL = 256 / G;
  const int g = tid % G, pl = tid / G;
  const int p_begin = blk * ppb;
  const int p_end = min(HW, p_begin + ppb);
  double mx[4], my[4], ca[4], cb[4], oy[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double *q = coef + ((size_t)b * C + g * 4 + e) * NQA_COEF;
    mx[e] = q[0];
    my[e] = q[1];
    ca[e] = q[2];
    cb[e] = q[3];
    oy[e] = q[5];
  }
  const size_t base = (size_t)b * HW * C + g * 4;
#pragma unroll 4
  for (int p = p_begin + pl; p < p_end; p += PL) {
    const size_t at = base + (size_t)p * C;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(tx + at);
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(ty + at);
    f32x4 acc = *reinterpret_cast<const f32x4 *>(gy + at);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double dx = (double)xv[e] - mx[e], dy = (double)yv[e] - my[e];
      const float u = yv[e] > 0.f ? (float)fma(cb[e], dx, fma(ca[e], dy, oy[e])) : 0.f;
      acc[e] = acc[e] + u;
    }
    *reinterpret_cast<f32x4 *>(gy + at) = acc;
  }
}

// ---- the renormalisation exponents ----------------------------------------------------------------------------------
// |float| as an unsigned integer orders like the value, every NaN above +inf: the maximum needs no float compare.
// grid (nblk, n); g: n images of `units` 16-byte units each.
// G: the element type of g.  A half's |bits| order like its value too (every NaN above +inf); the partial is then the
// 15-bit pattern of the largest |half|.
template <typename G>
__device__ __forceinline__ void absmax_partial_body(const u32x4 *__restrict__ g, long units, unsigned *__restrict__ part) {
  __shared__ unsigned red[4];
  const int img = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const u32x4 *p = g + (size_t)img * units;
  unsigned m = 0;
#pragma unroll 4
  for (long u = (long)blk * 256 + threadIdx.x; u < units; u += (long)nblk * 256) {
    const u32x4 v = p[u];
    if constexpr (sizeof(G) == 4) {
      m = max(max(m, v[0] & 0x7fffffffu), max(v[1] & 0x7fffffffu, max(v[2] & 0x7fffffffu, v[3] & 0x7fffffffu)));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) m = max(m, max(v[e] & 0x7fffu, (v[e] >> 16) & 0x7fffu));
    }
  }
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)img * nblk + blk] = max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void absmax_partial_kernel(const u32x4 *__restrict__ g, long units,
                                                             unsigned *__restrict__ part) {
  absmax_partial_body<float>(g, units, part);
}
// 16-byte units of eight halves
__global__ __launch_bounds__(256) void absmax_partial_half_kernel(const u32x4 *__restrict__ g, long units,
                                                                  unsigned *__restrict__ part) {
  absmax_partial_body<_Float16>(g, units, part);
}

// grid n, one wave per image.  kexp[img] = k; ktot[img] += k when ktot is given (one writer per image).
// G: whose bit patterns the partials are; TOP: max|g| 2^k lies in [2^(TOP-1), 2^TOP) -- 8 for the split16 chain's
// [128, 256), 4 for the half chain's [8, 16).
template <typename G, int TOP>
__device__ __forceinline__ void exponent_finish_body(const unsigned *__restrict__ part, int nblk, int *__restrict__ kexp,
                                                     int *__restrict__ ktot) {
  const int img = blockIdx.x;
  unsigned m = 0;
  for (int i = threadIdx.x; i < nblk; i += 64) m = max(m, part[(size_t)img * nblk + i]);
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
  if (threadIdx.x) return;
  int k = 0;
  if constexpr (sizeof(G) == 4) {
    if (m != 0 && m < 0x7f800000u) {
      // max = f 2^e with f in [0.5, 1) (frexp), from the bits: a normal float's biased exponent - 126; a subnormal one is
      // m 2^-149 with its highest set bit at 31 - clz(m)
      const int e = (m >> 23) ? (int)(m >> 23) - 126 : (31 - __clz((int)m)) - 148;
      k = TOP - e;
    }
  } else {
    if (m != 0 && m < 0x7c00u) {
      // the same from a half's bits: a normal half's biased exponent - 14; a subnormal one is m 2^-24
      const int e = (m >> 10) ? (int)(m >> 10) - 14 : (31 - __clz((int)m)) - 23;
      k = TOP - e;
    }
  }
  kexp[img] = k;
  if (ktot) ktot[img] += k;
}

__global__ __launch_bounds__(64) void exponent_finish_kernel(const unsigned *__restrict__ part, int nblk,
                                                             int *__restrict__ kexp, int *__restrict__ ktot) {
  exponent_finish_body<float, 8>(part, nblk, kexp, ktot);
}
// the half chain's window [8, 16), from a float or a half map's partials
template <typename G>
__global__ __launch_bounds__(64) void exponent_finish_half_kernel(const unsigned *__restrict__ part, int nblk,
                                                                  int *__restrict__ kexp, int *__restrict__ ktot) {
  exponent_finish_body<G, 4>(part, nblk, kexp, ktot);
}

// ---------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------
// blocks per pair of the sums kernel: enough to fill the device, few enough that the fold stays small
static int loss_sums_nblk(int HW, int C) {
  const int PL = 256 / (C / 4);
  const int n = cdiv(HW, PL * 8);
  return n < 1024 ? n : 1024;
}
static int loss_sums_ppb(int HW, int C) {
  const int PL = 256 / (C / 4);
  return cdiv(cdiv(HW, loss_sums_nblk(HW, C)), PL) * PL;
}

// The partials of one tap pair: [B][nblk][C][5] doubles.  The coefficient records behind them: [B][C][NQA_COEF].
size_t loss_stats_partials_doubles(int B, int HW, int C) {
  const int nblk = cdiv(HW, loss_sums_ppb(HW, C));
  return (size_t)B * nblk * C * 5;
}
size_t loss_stats_coef_doubles(int B, int C) { return (size_t)B * C * NQA_COEF; }
size_t loss_stats_backward_doubles(int B, int HW, int C) {
  return loss_stats_partials_doubles(B, HW, C) + loss_stats_coef_doubles(B, C);
}

static StageDesc loss_stage_desc(int HW, int C) {
  StageDesc d = {};
  d.nblk[0] = cdiv(HW, loss_sums_ppb(HW, C));
  d.hw[0] = HW;
  d.c[0] = C;
  d.nstage = 1;
  d.ctot = C;
  return d;
}

static int loss_stats_sums(const float *tx, const float *ty, int B, int HW, int C, double *part, hipStream_t st) {
  const int ppb = loss_sums_ppb(HW, C), nblk = cdiv(HW, ppb);
  TimedLaunch t(NQA_K_STATS, st);
  loss_stats_sums_kernel<<<dim3(nblk, B), 256, 0, st>>>(tx, ty, HW, C, ppb, part);
  return check_launch("loss_stats_sums");
}

// sums, then S1 / S2 from them; `part` stays as the backward's starting point
int loss_stats_target(const float *tx, const float *ty, int B, int HW, int C, double *part, float *s1, float *s2,
                      long s_stride, hipStream_t st) {
  int rc;
  if ((rc = loss_stats_sums(tx, ty, B, HW, C, part, st))) return rc;
  TimedLaunch t(NQA_K_STATS, st);
  loss_stats_fold_kernel<<<dim3(cdiv(C, 4), B), 256, 0, st>>>(part, loss_stage_desc(HW, C), s1, s2, s_stride);
  return check_launch("loss_stats_fold");
}

static int loss_stats_coef(int B, int HW, int C, const double *part, const float *g_s1, const float *g_s2, long g_stride,
                           double *coef, hipStream_t st) {
  TimedLaunch t(NQA_K_STATS, st);
  loss_stats_coef_kernel<<<dim3(cdiv(C, 4), B), 256, 0, st>>>(part, loss_stage_desc(HW, C), g_s1, g_s2, g_stride, coef);
  return check_launch("loss_stats_coef");
}

// the coefficients from partials that are already there, then the gradient
int loss_stats_backward_from(const float *tx, const float *ty, int B, int HW, int C, const double *part, const float *g_s1,
                             const float *g_s2, long g_stride, double *coef, float *gx, float *gy, hipStream_t st) {
  int rc;
  if ((rc = loss_stats_coef(B, HW, C, part, g_s1, g_s2, g_stride, coef, st))) return rc;
  const int PL = 256 / (C / 4), gppb = PL * 8;
  TimedLaunch t(NQA_K_STATS, st);
  loss_stats_grad_kernel<<<dim3(cdiv(HW, gppb), B), 256, 0, st>>>(tx, ty, HW, C, gppb, coef, gx, gy);
  return check_launch("loss_stats_grad");
}

// the same for the y side alone, ADDED into a gradient that is already in gy
int loss_stats_grad_y_add(const float *tx, const float *ty, int B, int HW, int C, const double *part, const float *g_s1,
                          const float *g_s2, long g_stride, double *coef, float *gy, hipStream_t st) {
  int rc;
  if ((rc = loss_stats_coef(B, HW, C, part, g_s1, g_s2, g_stride, coef, st))) return rc;
  const int PL = 256 / (C / 4), gppb = PL * 8;
  TimedLaunch t(NQA_K_STATS, st);
  loss_stats_grad_y_add_kernel<<<dim3(cdiv(HW, gppb), B), 256, 0, st>>>(tx, ty, HW, C, gppb, coef, gy);
  return check_launch("loss_stats_grad_y_add");
}

int loss_stats_backward(const float *tx, const float *ty, int B, int HW, int C, const float *g_s1, const float *g_s2,
                        long g_stride, double *ws, float *gx, float *gy, hipStream_t st) {
  double *part = ws, *coef = ws + loss_stats_partials_doubles(B, HW, C);
  int rc;
  if ((rc = loss_stats_sums(tx, ty, B, HW, C, part, st))) return rc;
  return loss_stats_backward_from(tx, ty, B, HW, C, part, g_s1, g_s2, g_stride, coef, gx, gy, st);
}

int grad_exponent_nblk(long per_image) {
  const long n = (per_image / 4 + 256 * 8 - 1) / (256 * 8);
  return n < 1 ? 1 : n > 512 ? 512 : (int)n;
}

int grad_exponent(const float *g, int n, long per_image, unsigned *ws, int *kexp, int *ktot, hipStream_t st) {
  const int nblk = grad_exponent_nblk(per_image);
  int rc;
  {
    TimedLaunch t(NQA_K_POOL, st);
    absmax_partial_kernel<<<dim3(nblk, n), 256, 0, st>>>(reinterpret_cast<const u32x4 *>(g), per_image / 4, ws);
    if ((rc = check_launch("absmax_partial"))) return rc;
  }
  TimedLaunch t(NQA_K_POOL, st);
  exponent_finish_kernel<<<n, 64, 0, st>>>(ws, nblk, kexp, ktot);
  return check_launch("exponent_finish");
}

// the half chain's exponents: max|g| 2^k in [8, 16); g float (per_image % 4 == 0) or half (per_image % 8 == 0)
int grad_exponent_half(const void *g, int g_half, int n, long per_image, unsigned *ws, int *kexp, int *ktot, hipStream_t st) {
  const int nblk = grad_exponent_nblk(per_image);
  const u32x4 *units = static_cast<const u32x4 *>(g);
  int rc;
  {
    TimedLaunch t(NQA_K_POOL, st);
    if (g_half) absmax_partial_half_kernel<<<dim3(nblk, n), 256, 0, st>>>(units, per_image / 8, ws);
    else absmax_partial_kernel<<<dim3(nblk, n), 256, 0, st>>>(units, per_image / 4, ws);
    if ((rc = check_launch("absmax_partial"))) return rc;
  }
  TimedLaunch t(NQA_K_POOL, st);
  if (g_half) exponent_finish_half_kernel<_Float16><<<n, 64, 0, st>>>(ws, nblk, kexp, ktot);
  else exponent_finish_half_kernel<float><<<n, 64, 0, st>>>(ws, nblk, kexp, ktot);
  return check_launch("exponent_finish_half");
}

}  // namespace nqa
