// Backward pass of the DISTS pyramid for gfx950: what DISTS.forward(x, y, require_grad=True) needs beyond the forward
// kernels (nerf_qa/DISTS_pytorch/DISTS_pt.py:105-108: the reference simply runs forward_once WITH autograd).
//
// The chain, per conv layer from relu5_3 down (driven by nerf_qa_amd/autograd.py, which re-runs the forward layer by
// layer to have the activations -- the fast fused forward keeps none):
//   relu_mask_split16   g * (act > 0) as split16 records            d(ReLU), and the input format of the next conv
//   conv3x3_split_generic (nqa_conv.hip)                             d(conv)/d(input) = conv with the flipped, transposed
//                                                                    weights, three-term split products (float accuracy)
//   l2pool_backward     g_tap += x * sum_o w(o) g_o / y_o            d(sqrt(hanning3x3_s2(x^2) + 1e-12)), DISTS_pt.py:22-25
//   conv1_1_backward    64 channels -> the 3 image planes            d(conv1_1), NCHW float out
// The loss path's second rung (grad_precision "f16") runs the same chain on plain half gradient maps: relu_mask_f16 in
// place of relu_mask_split16, conv3x3_half_generic (nqa_conv.hip: the forward's f16 implicit GEMM, one MFMA per product),
// and the half-input forms of the pool seam and of conv1_1's gradient, which differ from the float ones by the load alone.
// None of this is on the scoring hot path (no full-reference caller of the reference asks for image gradients); the
// kernels are plain HBM-streaming code.
#include "nqa_common.h"

namespace nqa {

__device__ static inline float split16_value(const char *pixel, int c) {  // channel c of a split16 pixel record
  const char *p = pixel + (c >> 4) * 64 + ((c >> 3) & 1) * 16 + (c & 7) * 2;
  return (float)*reinterpret_cast<const _Float16 *>(p) + (float)*reinterpret_cast<const _Float16 *>(p + 32);
}

// out = split16(g * (act > 0)); one thread per (pixel, 4 channels).  act is float (a tapped map) or split16.
// SCALED: g is multiplied by 2^kexp[image] first (an exact power of two read from device memory: the renormalisation of
// the loss path, which the host-scaled chain applies as a separate pass over g).
template <bool SCALED>
__global__ __launch_bounds__(256) void relu_mask_split16_kernel(const float *__restrict__ g, const void *__restrict__ act,
                                                                int act_split, long npix, int C, long pix_per_image,
                                                                const int *__restrict__ kexp, char *__restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int G = C / 4;
  if (idx >= npix * G) return;
  const long p = idx / G;
  const int c = (int)(idx - p * G) * 4;
  f32x4 gv = *reinterpret_cast<const f32x4 *>(g + p * C + c);
  if constexpr (SCALED) {
    const int k = kexp[p / pix_per_image];
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = ldexpf(gv[e], k);
  }
  float a[4];
  if (act_split) {
    const char *rec = static_cast<const char *>(act) + p * (long)C * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = split16_value(rec, c + e);
  } else {
    const f32x4 av = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(act) + p * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = av[e];
  }
  store_split4(out + p * (long)C * 4, c, a[0] > 0.f ? gv[0] : 0.f, a[1] > 0.f ? gv[1] : 0.f, a[2] > 0.f ? gv[2] : 0.f,
               a[3] > 0.f ? gv[3] : 0.f);
}

// The half chain's mask + encode: out = (_Float16)(g * 2^kexp[image]) where act > 0, else 0 -- a plain NHWC half map, one
// rounding (to nearest even) of an exactly scaled value.  One thread per (pixel, 8 channels): 16 bytes of out, of a half g
// and of each half of a split16 act; a float g or act moves as two 16-byte pieces.  One writer per element.
// GT: the element type of g (float: a tap's gradient or a pool seam's output; _Float16: the previous convolution's).
template <typename GT>
__global__ __launch_bounds__(256) void relu_mask_f16_kernel(const GT *__restrict__ g, const void *__restrict__ act,
                                                            int act_split, long npix, int C, long pix_per_image,
                                                            const int *__restrict__ kexp, _Float16 *__restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int G8 = C / 8;
  if (idx >= npix * G8) return;
  const long p = idx / G8;
  const int c = (int)(idx - p * G8) * 8;
  const int k = kexp[p / pix_per_image];
  float gv[8];
  if constexpr (sizeof(GT) == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(g + p * C + c), b = *reinterpret_cast<const f32x4 *>(g + p * C + c + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = a[e], gv[4 + e] = b[e];
  } else {
    const f16x8 v = *reinterpret_cast<const f16x8 *>(g + p * C + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) gv[e] = (float)v[e];
  }
  float a[8];
  if (act_split) {
    // channels c .. c+7 (c % 8 == 0) of a split16 record: 16 bytes of hi, their lo 32 bytes further
    const char *rec = static_cast<const char *>(act) + p * (long)C * 4 + (c >> 4) * 64 + ((c >> 3) & 1) * 16;
    const f16x8 hi = *reinterpret_cast<const f16x8 *>(rec), lo = *reinterpret_cast<const f16x8 *>(rec + 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = (float)hi[e] + (float)lo[e];
  } else {
    const float *ap = static_cast<const float *>(act) + p * C + c;
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ap), a1 = *reinterpret_cast<const f32x4 *>(ap + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = a0[e], a[4 + e] = a1[e];
  }
  f16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = a[e] > 0.f ? (_Float16)ldexpf(gv[e], k) : (_Float16)0.f;
  *reinterpret_cast<f16x8 *>(out + p * C + c) = o;
}

// g_x[iy, ix, c] += x[iy, ix, c] * sum over the (up to four) pooled pixels o whose 3x3 window holds (iy, ix) of
// w(o; iy, ix) * g_y[o, c] / y[o, c],  w = hanning3x3 / 16, y = the pooled value.  y is formed HERE from x in float: the
// forward's pooled map is split16, whose lo half is a subnormal half (absolute step 2^-24) for values below 2^-3 -- a
// pooled value of 5e-4 read from it is off by up to 2^-14 (6e-5 of the gradient; 1.3 % at the sqrt(1e-12) floor).
__device__ static inline void l2pool_value4(const float *__restrict__ x, int n, int H, int W, int C, int oy, int ox, int c,
                                            float (&y)[4]) {
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int sy = 2 * oy - 1 + ky;
    if ((unsigned)sy >= (unsigned)H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int sx = 2 * ox - 1 + kx;
      if ((unsigned)sx >= (unsigned)W) continue;
      const float wgt = (ky == 1 ? 0.5f : 0.25f) * (kx == 1 ? 0.5f : 0.25f);
      const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (((long)n * H + sy) * W + sx) * C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = fmaf(wgt * v[e], v[e], s[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = sqrtf(s[e] + 1e-12f);
}

// four consecutive gradient elements as floats: GT = float (16 bytes) or _Float16 (8 bytes; half -> float is exact)
template <typename GT>
__device__ static inline f32x4 load_grad4(const GT *__restrict__ p) {
  if constexpr (sizeof(GT) == 4) {
    return *reinterpret_cast<const f32x4 *>(p);
  } else {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    const h4 v = *reinterpret_cast<const h4 *>(p);
    const f32x4 o = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    return o;
  }
}

// SCALED: gx_out = gx_in * 2^ktot[image] + pool gradient (gx_in: the tap's own gradient, brought into the running scale
// of the chain here); otherwise gx_in == gx_out and the pool gradient is added in place.
// GT: the element type of the pooled map's gradient gy (float, or _Float16 behind the half chain's convolutions).
template <bool SCALED, typename GT>
__device__ __forceinline__ void l2pool_backward_body(const float *__restrict__ x, const GT *__restrict__ gy, int H, int W,
                                                     int C, int Ho, int Wo, long total, const float *gx_in,
                                                     const int *__restrict__ ktot, float *gx) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int G = C / 4;
  const int c = (int)(idx % G) * 4;
  long t = idx / G;
  const int ix = (int)(t % W);
  t /= W;
  const int iy = (int)(t % H);
  const int n = (int)(t / H);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // output rows oy with |2 oy - iy| <= 1: iy even -> oy = iy/2 (centre row, weight 1/2); iy odd -> oy = (iy-1)/2 and
  // (iy+1)/2 (edge rows, weight 1/4 each)
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int oy = (iy & 1) ? (iy - 1) / 2 + a : (a == 0 ? iy / 2 : -1);
    if (oy < 0 || oy >= Ho) continue;
    const float wy = (iy & 1) ? 0.25f : 0.5f;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ox = (ix & 1) ? (ix - 1) / 2 + b : (b == 0 ? ix / 2 : -1);
      if (ox < 0 || ox >= Wo) continue;
      const float wgt = wy * ((ix & 1) ? 0.25f : 0.5f);
      const long o = ((long)n * Ho + oy) * Wo + ox;
      const f32x4 gv = load_grad4<GT>(gy + o * C + c);
      float yv[4];
      l2pool_value4(x, n, H, W, C, oy, ox, c, yv);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += wgt * gv[e] / yv[e];
    }
  }
  const long xi = (((long)n * H + iy) * W + ix) * C + c;
  const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + xi);
  f32x4 o = *reinterpret_cast<const f32x4 *>(gx_in + xi);
  if constexpr (SCALED) {
    const int k = ktot[n];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ldexpf(o[e], k);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] += xv[e] * acc[e];
  *reinterpret_cast<f32x4 *>(gx + xi) = o;
}

template <bool SCALED>
__global__ __launch_bounds__(256) void l2pool_backward_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                              int H, int W, int C, int Ho, int Wo, long total,
                                                              const float *gx_in, const int *__restrict__ ktot,
                                                              float *gx) {
  l2pool_backward_body<SCALED, float>(x, gy, H, W, C, Ho, Wo, total, gx_in, ktot, gx);
}
// the scaled form behind a half data-gradient convolution
__global__ __launch_bounds__(256) void l2pool_backward_half_kernel(const float *__restrict__ x,
                                                                   const _Float16 *__restrict__ gy, int H, int W, int C,
                                                                   int Ho, int Wo, long total, const float *gx_in,
                                                                   const int *__restrict__ ktot, float *gx) {
  l2pool_backward_body<true, _Float16>(x, gy, H, W, C, Ho, Wo, total, gx_in, ktot, gx);
}

// d(conv1_1)/d(normalised image): gimg[n, c, y, x] = sum_{ky,kx,co} gm[n, y+1-ky, x+1-kx, co] * w[co, c, ky, kx], then
// divided by std[c] (the input normalisation (x - mean) / std, DISTS_pt.py:92).  gm = g * (relu1_1 > 0), float NHWC.
// One wave per output pixel: lane = output channel co of gm, 27 products per lane, wave sums.
// SCALED: gm is the UNMASKED gradient; it is multiplied by 2^kexp[image] and masked with relu1_1 > 0 (act0: split16
// records, or null for no mask) as it is read, and 2^-ktot[image] is taken out of the result.
// GT: the element type of gm (float, or _Float16: the half chain's last map).
template <bool SCALED, typename GT>
__device__ __forceinline__ void conv1_1_backward_body(const GT *__restrict__ gm, const float *__restrict__ w, int H, int W,
                                                      long npix, const char *__restrict__ act0,
                                                      const int *__restrict__ kexp, const int *__restrict__ ktot,
                                                      float *__restrict__ gimg) {
  const int lane = threadIdx.x & 63;
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= npix) return;
  const long HW = (long)H * W;
  const int n = (int)(pix / HW);
  const long r = pix - (long)n * HW;
  const int y = (int)(r / W), x = (int)(r - (long)y * W);
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int sy = y + 1 - ky;
    if ((unsigned)sy >= (unsigned)H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int sx = x + 1 - kx;
      if ((unsigned)sx >= (unsigned)W) continue;
      const long src = ((long)n * H + sy) * W + sx;
      float gv = (float)gm[src * 64 + lane];
      if constexpr (SCALED) {
        gv = ldexpf(gv, kexp[n]);
        if (act0 && !(split16_value(act0 + src * 256, lane) > 0.f)) gv = 0.f;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fmaf(gv, w[((lane * 3 + c) * 3 + ky) * 3 + kx], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, 64);
  if (lane == 0) {
    const float sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o = acc[c] / sd[c];
      if constexpr (SCALED) o = ldexpf(o, -ktot[n]);
      gimg[((long)n * 3 + c) * HW + r] = o;
    }
  }
}

template <bool SCALED>
__global__ __launch_bounds__(256) void conv1_1_backward_kernel(const float *__restrict__ gm, const float *__restrict__ w,
                                                               int H, int W, long npix, const char *__restrict__ act0,
                                                               const int *__restrict__ kexp, const int *__restrict__ ktot,
                                                               float *__restrict__ gimg) {
  conv1_1_backward_body<SCALED, float>(gm, w, H, W, npix, act0, kexp, ktot, gimg);
}
__global__ __launch_bounds__(256) void conv1_1_backward_half_kernel(const _Float16 *__restrict__ gm,
                                                                    const float *__restrict__ w, int H, int W, long npix,
                                                                    const char *__restrict__ act0,
                                                                    const int *__restrict__ kexp,
                                                                    const int *__restrict__ ktot, float *__restrict__ gimg) {
  conv1_1_backward_body<true, _Float16>(gm, w, H, W, npix, act0, kexp, ktot, gimg);
}

int relu_mask_split16(const float *g, const void *act, int act_split, long npix, int C, void *out, hipStream_t st) {
  const long total = npix * (C / 4);
  relu_mask_split16_kernel<false><<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      g, act, act_split, npix, C, npix, nullptr, static_cast<char *>(out));
  return check_launch("relu_mask_split16");
}

int relu_mask_split16_scaled(const float *g, const void *act, int act_split, int n, long pix_per_image, int C,
                             const int *kexp, void *out, hipStream_t st) {
  const long npix = (long)n * pix_per_image, total = npix * (C / 4);
  TimedLaunch t(NQA_K_POOL, st);
  relu_mask_split16_kernel<true><<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      g, act, act_split, npix, C, pix_per_image, kexp, static_cast<char *>(out));
  return check_launch("relu_mask_split16_scaled");
}

int l2pool_backward(const float *x, const void * /*y_split16: not read, see the kernel*/, const float *gy, int n, int H,
                    int W, int C, float *gx, hipStream_t st) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long total = (long)n * H * W * (C / 4);
  l2pool_backward_kernel<false><<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(x, gy, H, W, C, Ho, Wo, total, gx,
                                                                                       nullptr, gx);
  return check_launch("l2pool_backward");
}

int l2pool_backward_scaled(const float *x, const float *gy, const float *g_tap, const int *ktot, int n, int H, int W,
                           int C, float *out, hipStream_t st) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long total = (long)n * H * W * (C / 4);
  TimedLaunch t(NQA_K_POOL, st);
  l2pool_backward_kernel<true><<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(x, gy, H, W, C, Ho, Wo, total, g_tap,
                                                                                      ktot, out);
  return check_launch("l2pool_backward_scaled");
}

int conv1_1_backward(const float *gm, const float *w_oihw, int n, int H, int W, float *gimg, hipStream_t st) {
  const long npix = (long)n * H * W;
  conv1_1_backward_kernel<false><<<dim3((unsigned)((npix + 3) / 4)), 256, 0, st>>>(gm, w_oihw, H, W, npix, nullptr,
                                                                                   nullptr, nullptr, gimg);
  return check_launch("conv1_1_backward");
}

int conv1_1_backward_scaled(const float *g, const void *act0_split16, const float *w_oihw, const int *kexp,
                            const int *ktot, int n, int H, int W, float *gimg, hipStream_t st) {
  const long npix = (long)n * H * W;
  TimedLaunch t(NQA_K_POOL, st);
  conv1_1_backward_kernel<true><<<dim3((unsigned)((npix + 3) / 4)), 256, 0, st>>>(
      g, w_oihw, H, W, npix, static_cast<const char *>(act0_split16), kexp, ktot, gimg);
  return check_launch("conv1_1_backward_scaled");
}

// ---- the half chain (grad_precision "f16"): the same steps on half gradient maps ----
int relu_mask_f16_scaled(const void *g, int g_half, const void *act, int act_split, int n, long pix_per_image, int C,
                         const int *kexp, void *out, hipStream_t st) {
  const long npix = (long)n * pix_per_image, total = npix * (C / 8);
  const dim3 grid((unsigned)((total + 255) / 256));
  TimedLaunch t(NQA_K_POOL, st);
  if (g_half)
    relu_mask_f16_kernel<_Float16><<<grid, 256, 0, st>>>(static_cast<const _Float16 *>(g), act, act_split, npix, C,
                                                         pix_per_image, kexp, static_cast<_Float16 *>(out));
  else
    relu_mask_f16_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float *>(g), act, act_split, npix, C, pix_per_image,
                                                      kexp, static_cast<_Float16 *>(out));
  return check_launch("relu_mask_f16_scaled");
}

int l2pool_backward_scaled_half(const float *x, const void *gy_f16, const float *g_tap, const int *ktot, int n, int H, int W,
                                int C, float *out, hipStream_t st) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long total = (long)n * H * W * (C / 4);
  TimedLaunch t(NQA_K_POOL, st);
  l2pool_backward_half_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(
      x, static_cast<const _Float16 *>(gy_f16), H, W, C, Ho, Wo, total, g_tap, ktot, out);
  return check_launch("l2pool_backward_scaled_half");
}

int conv1_1_backward_scaled_half(const void *g_f16, const void *act0_split16, const float *w_oihw, const int *kexp,
                                 const int *ktot, int n, int H, int W, float *gimg, hipStream_t st) {
  const long npix = (long)n * H * W;
  TimedLaunch t(NQA_K_POOL, st);
  conv1_1_backward_half_kernel<<<dim3((unsigned)((npix + 3) / 4)), 256, 0, st>>>(
      static_cast<const _Float16 *>(g_f16), w_oihw, H, W, npix, static_cast<const char *>(act0_split16), kexp, ktot, gimg);
  return check_launch("conv1_1_backward_scaled_half");
}

}  // namespace nqa
