// A-DISTS as a LOSS with the gradient on y alone (ADISTS.forward(x, y) with a fixed frame x and a render y that is being
// optimised; nerf_qa_amd/autograd.py, adists_backward_y) for gfx950: ONE stage of the head's backward, from the raw
// planar maps and what the forward's staged entry points leave (q, the channel weights, x's probability map) to dL/dY.
//
// With x fixed, the texture probabilities p and the channel weights w are constants; only the windowed T / S terms
// (ADISTS.py:165-183) and F.normalize of y (:167) are differentiated (the contract is in include/nqa.h).
//
//   windowed stage (H, W >= the window n of the call, 3 .. 63; the entry point without a window passes 21)
//     window_moments_forward          the five raw window means (nqa_window_moments_n.hip, which picks the kernels)
//     adists_ts_coef_kernel           pointwise over map positions: the upstreams g1, g3, g4 of E[y], E[y^2], E[xy], written
//                                     over those three maps
//     window_moments_backward         P = W^T g1 + 2 Y W^T g3 + X W^T g4, the one-sided three-pass call
//     adists_ts_dot_kernel            per block the fp64 partial of <P, Y> of one plane
//     adists_ts_fold_kernel           one wave per plane folds them in a fixed order: s = a_y^2 <P, Y>, 0 under the clamp
//     adists_ts_apply_kernel          gy = P - Y s, times the ReLU mask (Y > 0); planar out, or
//     adists_ts_apply_nhwc_kernel     the same through a 32 channel x 64 pixel LDS tile into an NHWC map
//   global stage (a map under the window in either direction)
//     adists_ts_global_kernel         one block per plane does all of it from q's plain moments
//
// Everything here streams: 16-byte accesses where the rows allow them (W % 4 == 0), one writer per element, no atomics
// (bitwise repeatable), and no plane ever meets another pair's numbers.  The per-position arithmetic is fp64 on the
// float moments (two divisions per position; the kernels stay bandwidth-bound), rounded to float once.
#include <math.h>

#include "nqa_common.h"

namespace nqa {

static constexpr int kCoefPerBlock = 1024;  // map positions per block of the coefficient and planar apply kernels
static constexpr int kDotPerBlock = 4096;   // plane elements per block of the dot-product partials
static constexpr double kEps = 1e-6;        // ADISTS.py:182-183
static constexpr float kClamp = 1e12f;      // a_y = 1 / max(||Y||, 1e-12) sits here when F.normalize clamps

// Upstreams of the raw moments E[y], E[y^2], E[xy] at one position from the normalised moments there.
// a = dL/dT, bc = dL/dS of this position and channel.
__device__ inline void ts_upstreams(double xm, double ym, double xv, double yv, double cov, double ax, double ay, double a,
                                    double bc, double &g1, double &g3, double &g4) {
  const double r1 = 1.0 / (xm * xm + ym * ym + kEps);
  const double t = (2.0 * xm * ym + kEps) * r1;
  const double dt_dym = (2.0 * xm - 2.0 * ym * t) * r1;
  const double r2 = 1.0 / (xv + yv + kEps);
  const double s = (2.0 * cov + kEps) * r2;
  const double ds_dcov = 2.0 * r2, ds_dyv = -s * r2;
  const double g_ym = a * dt_dym - bc * (xm * ds_dcov + 2.0 * ym * ds_dyv);
  g1 = ay * g_ym;
  g3 = ay * ay * (bc * ds_dyv);
  g4 = ax * ay * (bc * ds_dcov);
}

struct PlaneScalars {
  int b, c;
  double ax, ay, wc, ub;
  size_t qo, st;
};
// q [8][B][ctot], wgt [B][ctot]: the stage's channels start at coff (the forward's convention)
__device__ inline PlaneScalars plane_scalars(int p, int B, int C, const float *__restrict__ q, const float *__restrict__ wgt,
                                             int ctot, int coff, const float *__restrict__ u) {
  PlaneScalars s;
  s.b = p / C;
  s.c = p % C;
  s.st = (size_t)B * ctot;
  s.qo = (size_t)s.b * ctot + coff + s.c;
  s.ax = (double)q[s.qo];
  s.ay = (double)q[s.st + s.qo];
  s.wc = (double)wgt[s.qo];
  s.ub = (double)u[s.b];
  return s;
}

// grid P * nblk, nblk = cdiv(hw, 1024); block = (plane, 1024 positions), thread = 4 adjacent positions.
// mom: the five window means, moment m of plane p at (m * P + p) * hw; g1, g3, g4 replace moments 1, 3, 4.
__global__ __launch_bounds__(256) void adists_ts_coef_kernel(float *__restrict__ mom, int B, int C, int hw, int nblk,
                                                             const float *__restrict__ q, const float *__restrict__ wgt,
                                                             int ctot, int coff, const float *__restrict__ ps,
                                                             const float *__restrict__ u, int vec) {
  const int p = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int i0 = blk * kCoefPerBlock + threadIdx.x * 4;
  if (i0 >= hw) return;
  const PlaneScalars sc = plane_scalars(p, B, C, q, wgt, ctot, coff, u);
  const double scale = sc.ub * sc.wc / (double)hw;
  const size_t P = (size_t)B * C;
  float *m[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) m[k] = mom + ((size_t)k * P + p) * hw + i0;
  const float *pp = ps + (size_t)sc.b * hw + i0;
  float v[6][4];
  if (vec) {  // (hw % 4 == 0 and 16-byte aligned planes: the four positions are inside together)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4 *>(k < 5 ? m[k] : pp);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = t[e];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = i0 + e < hw ? (k < 5 ? m[k][e] : pp[e]) : 0.f;
  }
  float o[3][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double xm = sc.ax * (double)v[0][e], ym = sc.ay * (double)v[1][e];
    const double xv = sc.ax * sc.ax * (double)v[2][e] - xm * xm, yv = sc.ay * sc.ay * (double)v[3][e] - ym * ym;
    const double cov = sc.ax * sc.ay * (double)v[4][e] - xm * ym;
    const double pr = (double)v[5][e];
    double g1, g3, g4;
    ts_upstreams(xm, ym, xv, yv, cov, sc.ax, sc.ay, scale * (1.0 - pr), scale * pr, g1, g3, g4);
    o[0][e] = (float)g1;
    o[1][e] = (float)g3;
    o[2][e] = (float)g4;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float *dst = m[k == 0 ? 1 : k == 1 ? 3 : 4];
    if (vec) {
      *reinterpret_cast<f32x4 *>(dst) = f32x4{o[k][0], o[k][1], o[k][2], o[k][3]};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < hw) dst[e] = o[k][e];
    }
  }
}

// Sum of one double per thread over the block, folded in a fixed order; valid in every thread.
__device__ inline double block_total(double s, double *red /* [4] */) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __syncthreads();  // (red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid P * nblk, nblk = cdiv(HW, 4096).  part[p * nblk + blk] = sum over the block's elements of pm * y.
__global__ __launch_bounds__(256) void adists_ts_dot_kernel(const float *__restrict__ pm, const float *__restrict__ y, int HW,
                                                            int nblk, int vec, double *__restrict__ part) {
  __shared__ double red[4];
  const int p = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const float *a = pm + (size_t)p * HW, *b = y + (size_t)p * HW;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kDotPerBlock / 1024; ++j) {
    const int i0 = blk * kDotPerBlock + j * 1024 + threadIdx.x * 4;
    if (i0 >= HW) continue;
    if (vec) {
      const f32x4 av = *reinterpret_cast<const f32x4 *>(a + i0), bv = *reinterpret_cast<const f32x4 *>(b + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fma((double)av[e], (double)bv[e], s);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < HW) s = fma((double)a[i0 + e], (double)b[i0 + e], s);
    }
  }
  s = block_total(s, red);
  if (threadIdx.x == 0) part[(size_t)p * nblk + blk] = s;
}

// grid cdiv(P, 4), one wave per plane.  sdot[p] = a_y^2 <P, Y>, or 0 where F.normalize clamps (||Y|| < 1e-12).
__global__ __launch_bounds__(256) void adists_ts_fold_kernel(const double *__restrict__ part, int nblk, int P, int B, int C,
                                                             const float *__restrict__ q, int ctot, int coff,
                                                             double *__restrict__ sdot) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  double s = 0.0;
  for (int i = lane; i < nblk; i += 64) s += part[(size_t)p * nblk + i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane) return;
  const float ay = q[(size_t)B * ctot + (size_t)(p / C) * ctot + coff + p % C];
  sdot[p] = ay >= kClamp ? 0.0 : (double)ay * (double)ay * s;
}

__device__ inline float ts_apply(float pv, float yv, double s, int mask) {
  const float r = (float)((double)pv - (double)yv * s);
  return (mask && !(yv > 0.f)) ? 0.f : r;
}

// grid P * nblk, nblk = cdiv(HW, 1024): planar gy = pm - y * sdot[plane], masked.
__global__ __launch_bounds__(256) void adists_ts_apply_kernel(const float *__restrict__ pm, const float *__restrict__ y,
                                                              int HW, int nblk, int vec, const double *__restrict__ sdot,
                                                              int mask, float *__restrict__ gy) {
  const int p = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int i0 = blk * kCoefPerBlock + threadIdx.x * 4;
  if (i0 >= HW) return;
  const double s = sdot[p];
  const size_t at = (size_t)p * HW + i0;
  if (vec) {
    const f32x4 av = *reinterpret_cast<const f32x4 *>(pm + at), bv = *reinterpret_cast<const f32x4 *>(y + at);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ts_apply(av[e], bv[e], s, mask);
    *reinterpret_cast<f32x4 *>(gy + at) = o;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < HW) gy[at + e] = ts_apply(pm[at + e], y[at + e], s, mask);
  }
}

// grid (cdiv(HW, 64), C / 32, B): the same values into an NHWC map (B, HW, C).  Thread (px, cc) reads pixel px of the
// channels cc, cc + 4, ... of the tile (rows of 64 floats per channel); thread (c, pl) writes channel c of the pixels
// pl, pl + 8, ... (32 adjacent floats per pixel).  The tile's row stride of 65 keeps both sides free of bank conflicts.
__global__ __launch_bounds__(256) void adists_ts_apply_nhwc_kernel(const float *__restrict__ pm, const float *__restrict__ y,
                                                                   int HW, int C, const double *__restrict__ sdot, int mask,
                                                                   float *__restrict__ gy) {
  __shared__ float tile[32 * 65];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 32, b = blockIdx.z;
  {
    const int px = threadIdx.x & 63, cc = threadIdx.x >> 6;
    const bool in = r0 + px < HW;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int cl = cc + 4 * i;
      const size_t plane = (size_t)b * C + c0 + cl;
      float v = 0.f;
      if (in) v = ts_apply(pm[plane * HW + r0 + px], y[plane * HW + r0 + px], sdot[plane], mask);
      tile[cl * 65 + px] = v;
    }
  }
  __syncthreads();
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int px = pl + 8 * i;
    if (r0 + px < HW) gy[((size_t)b * HW + r0 + px) * C + c0 + cl] = tile[cl * 65 + px];
  }
}

// grid P, one block per plane: the global branch (ADISTS.py:176-180).  q rows 3..7 = mean_x mean_y var_x var_y cov of
// the raw maps; one probability per pair; P(r) = (g1 + 2 Y(r) g3 + X(r) g4) / HW is never stored.
__global__ __launch_bounds__(256) void adists_ts_global_kernel(const float *__restrict__ x, const float *__restrict__ y, int B,
                                                               int C, int HW, const float *__restrict__ q,
                                                               const float *__restrict__ wgt, int ctot, int coff,
                                                               const float *__restrict__ ps, const float *__restrict__ u,
                                                               int mask, int nhwc, float *__restrict__ gy) {
  __shared__ double red[4];
  const int p = blockIdx.x;
  const PlaneScalars sc = plane_scalars(p, B, C, q, wgt, ctot, coff, u);
  const double xm = sc.ax * (double)q[3 * sc.st + sc.qo], ym = sc.ay * (double)q[4 * sc.st + sc.qo];
  const double xv = sc.ax * sc.ax * (double)q[5 * sc.st + sc.qo], yv = sc.ay * sc.ay * (double)q[6 * sc.st + sc.qo];
  const double cov = sc.ax * sc.ay * (double)q[7 * sc.st + sc.qo];
  const double pr = (double)ps[sc.b], scale = sc.ub * sc.wc;
  double g1, g3, g4;
  ts_upstreams(xm, ym, xv, yv, cov, sc.ax, sc.ay, scale * (1.0 - pr), scale * pr, g1, g3, g4);
  const double inv = 1.0 / (double)HW;
  g1 *= inv;
  g3 *= 2.0 * inv;
  g4 *= inv;
  const float *X = x + (size_t)p * HW, *Y = y + (size_t)p * HW;
  double s = 0.0;
  for (int r = threadIdx.x; r < HW; r += 256) {
    const double yr = (double)Y[r];
    s = fma(fma(yr, g3, fma((double)X[r], g4, g1)), yr, s);
  }
  s = block_total(s, red);
  const float ayf = q[sc.st + sc.qo];
  const double sd = ayf >= kClamp ? 0.0 : sc.ay * sc.ay * s;
  for (int r = threadIdx.x; r < HW; r += 256) {
    const float yf = Y[r];
    const double yr = (double)yf;
    const float v = (float)(fma(yr, g3, fma((double)X[r], g4, g1)) - yr * sd);
    const size_t at = nhwc ? ((size_t)sc.b * HW + r) * C + sc.c : (size_t)p * HW + r;
    gy[at] = (mask && !(yf > 0.f)) ? 0.f : v;
  }
}

// ---------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------
struct TsPlan {
  bool windowed;
  size_t P, HW, hw;
  int nblk_coef, nblk_dot, nblk_apply;
  size_t off_sdot, off_pm, off_mom, bytes;  // byte offsets into the workspace
};

static TsPlan ts_plan(int B, int C, int H, int W, int win) {
  TsPlan t = {};
  t.windowed = H >= win && W >= win;
  t.P = (size_t)B * C;
  t.HW = (size_t)H * W;
  if (!t.windowed) {
    t.bytes = 16;  // (nothing is kept; 0 is the refusal)
    return t;
  }
  t.hw = (size_t)(H - win + 1) * (W - win + 1);
  t.nblk_coef = (int)((t.hw + kCoefPerBlock - 1) / kCoefPerBlock);
  t.nblk_dot = (int)((t.HW + kDotPerBlock - 1) / kDotPerBlock);
  t.nblk_apply = (int)((t.HW + kCoefPerBlock - 1) / kCoefPerBlock);
  t.off_sdot = align_up(t.P * t.nblk_dot * sizeof(double), 16);
  t.off_pm = t.off_sdot + align_up(t.P * sizeof(double), 16);
  t.off_mom = t.off_pm + align_up(t.P * t.HW * sizeof(float), 16);
  t.bytes = t.off_mom + align_up(5 * t.P * t.hw * sizeof(float), 16);
  return t;
}

// whether every flat grid of the stage fits a launch (P * blocks per plane under 2^31)
bool adists_ts_backward_fits(int B, int C, int H, int W, int window) {
  const TsPlan t = ts_plan(B, C, H, W, window);
  const size_t lim = (size_t)1 << 31;
  if (t.P >= lim) return false;
  if (!t.windowed) return true;
  return t.P * (size_t)t.nblk_apply < lim && t.P * (size_t)t.nblk_coef < lim;
}

size_t adists_ts_backward_bytes(int B, int C, int H, int W, int window) { return ts_plan(B, C, H, W, window).bytes; }

// `kernels` goes to the two window-moments calls, which decide what a window of 21 runs
int adists_ts_backward(const float *x, const float *y, int B, int C, int H, int W, int window, MomentsKernels kernels,
                       const float *q, const float *wgt, int ctot, int coff, const float *ps, const float *u, int mask,
                       int out_nhwc, void *ws, float *gy, hipStream_t st) {
  const TsPlan t = ts_plan(B, C, H, W, window);
  const int P = (int)t.P, HW = (int)t.HW;
  if (!t.windowed) {
    TimedLaunch tl(NQA_K_ADISTS, st);
    adists_ts_global_kernel<<<P, 256, 0, st>>>(x, y, B, C, HW, q, wgt, ctot, coff, ps, u, mask, out_nhwc, gy);
    return check_launch("adists_ts_global");
  }
  char *base = static_cast<char *>(ws);
  double *part = reinterpret_cast<double *>(base), *sdot = reinterpret_cast<double *>(base + t.off_sdot);
  float *pm = reinterpret_cast<float *>(base + t.off_pm), *mom = reinterpret_cast<float *>(base + t.off_mom);
  const int hw = (int)t.hw, vec = (W & 3) == 0;
  // the moment maps are planes of hw floats: 16-byte accesses there need hw % 4 == 0 as well, which W % 4 == 0 implies
  // for a window of 21 (and of any n with (n - 1) % 4 == 0) and for no other
  const int vec_m = vec && (t.hw & 3) == 0;
  int rc;
  if ((rc = window_moments_forward(x, y, P, H, W, window, kernels, mom, st))) return rc;
  {
    TimedLaunch tl(NQA_K_ADISTS, st);
    adists_ts_coef_kernel<<<(unsigned)(t.P * t.nblk_coef), 256, 0, st>>>(mom, B, C, hw, t.nblk_coef, q, wgt, ctot, coff, ps, u,
                                                                         vec_m);
    if ((rc = check_launch("adists_ts_coef"))) return rc;
  }
  const float *const g[5] = {nullptr, mom + t.P * t.hw, nullptr, mom + 3 * t.P * t.hw, mom + 4 * t.P * t.hw};
  if ((rc = window_moments_backward(x, y, P, H, W, window, kernels, g, nullptr, pm, st))) return rc;
  {
    TimedLaunch tl(NQA_K_ADISTS, st);
    adists_ts_dot_kernel<<<(unsigned)(t.P * t.nblk_dot), 256, 0, st>>>(pm, y, HW, t.nblk_dot, vec, part);
    if ((rc = check_launch("adists_ts_dot"))) return rc;
  }
  {
    TimedLaunch tl(NQA_K_ADISTS, st);
    adists_ts_fold_kernel<<<cdiv(P, 4), 256, 0, st>>>(part, t.nblk_dot, P, B, C, q, ctot, coff, sdot);
    if ((rc = check_launch("adists_ts_fold"))) return rc;
  }
  TimedLaunch tl(NQA_K_ADISTS, st);
  if (out_nhwc) {
    adists_ts_apply_nhwc_kernel<<<dim3(cdiv(HW, 64), C / 32, B), 256, 0, st>>>(pm, y, HW, C, sdot, mask, gy);
    return check_launch("adists_ts_apply_nhwc");
  }
  adists_ts_apply_kernel<<<(unsigned)(t.P * t.nblk_apply), 256, 0, st>>>(pm, y, HW, t.nblk_apply, vec, sdot, mask, gy);
  return check_launch("adists_ts_apply");
}

}  // namespace nqa
