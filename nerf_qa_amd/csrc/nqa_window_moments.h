// What the two window-moments files share: nqa_window_moments.hip (the 21-tap kernels) and nqa_window_moments_n.hip (the
// generic kernels, and window_moments_forward / _backward, which choose between the two).  The kernels themselves share
// nothing but store4: DESIGN.md 4.21 has what became of the attempts to share more.
#pragma once

#include "nqa_common.h"

namespace nqa {

// 4 floats of one row: a 16-byte store where the row allows it, else the elements that are inside
__device__ inline void store4(float *row, int c, int nc, bool vec, const float (&v)[4]) {
  if (vec) {
    if (c < nc) *reinterpret_cast<f32x4 *>(row + c) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < nc) row[c + e] = v[e];
  }
}

// The upstream maps of a backward call as the kernel argument WG (WindowGrads or WindowGradsN: two types, because the
// type is part of a kernel's name), without the maps the wanted sides do not read: g0, g2 without gx; g1, g3 without gy.
template <typename WG>
inline WG wanted_grads(const float *const g[5], const float *gx, const float *gy) {
  WG wg;
  for (int q = 0; q < 5; ++q) wg.g[q] = g[q];
  if (!gx) wg.g[0] = wg.g[2] = nullptr;
  if (!gy) wg.g[1] = wg.g[3] = nullptr;
  return wg;
}

// The planes ride gridDim.z, 65535 at most: one launch of gx x gy x planes blocks per chunk of P.  launch(grid, p0)
// starts the kernel `what` on the planes from p0.
template <typename F>
inline int launch_plane_chunks(const char *what, int P, int gx, int gy, hipStream_t st, F launch) {
  constexpr int kMaxGridZ = 65535;
  for (int p0 = 0; p0 < P; p0 += kMaxGridZ) {
    const dim3 grid(gx, gy, P - p0 < kMaxGridZ ? P - p0 : kMaxGridZ);
    TimedLaunch t(NQA_K_ADISTS, st);
    launch(grid, p0);
    if (int rc = check_launch(what)) return rc;
  }
  return 0;
}

// the 21-tap launchers (nqa_window_moments.hip); window_moments_forward / _backward are their only callers
int window_moments_forward_21(const float *x, const float *y, int P, int H, int W, float *out, hipStream_t st);
int window_moments_backward_21(const float *x, const float *y, int P, int H, int W, const float *const g[5], float *gx,
                               float *gy, hipStream_t st);

}  // namespace nqa
