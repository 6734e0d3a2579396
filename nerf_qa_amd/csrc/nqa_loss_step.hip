// The DISTS loss step against a PREPARED TARGET as two calls (include/nqa.h, "the prepared-target loss step"): what
// nerf_qa_amd/autograd.py's dists_target_forward / dists_target_backward enqueue launch by launch from Python (one kept
// pyramid of y, the statistics of nerf_qa/DISTS_pytorch/DISTS_pt.py:130-141 against the target's taps, their gradient,
// the gradient chain down to the image), driven from the host code below on ONE caller-owned state block.
//
// Nothing here computes a number of the metric: every launch goes through the library's own entry points, with the
// arguments the Python path gives them, in its order -- so S1, S2 and dL/dy are that path's bit for bit -- and each
// keeps its timing class.  What is new is the plan of the state block (step_plan), one check of every argument before
// the first launch, and four small kernels that stand where the Python path has a torch expression:
//   step_zero_kernel      the five one-pixel dummy maps of tap 0 (torch.zeros) and the chain's running exponents
//   step_cols3_kernel     S1 / S2 of the image: columns 0..2 of the (B, 8) rows into the (B, 1475) rows
//   step_pad8_kernel      the upstream gradient of tap 0: columns 0..2 of (B, 1475), five zeros behind them
//   step_add_kernel       gy += the image term of tap 0 (one float add per element, torch's gimg + gy0)
// and score_backward_kernel, the derivative of score_kernel (nqa_pool_stats.hip) towards S1 and S2, for a caller without
// autograd.  All of them are plain loads and vector stores, one writer per element, counted as NQA_K_PREP.
#include "nqa_common.h"

namespace nqa {

__global__ __launch_bounds__(256) void step_zero_kernel(unsigned *__restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 0u;
}

// in (B, 8) -> out (B, stride): columns 0..2
__global__ __launch_bounds__(256) void step_cols3_kernel(const float *__restrict__ a1, const float *__restrict__ a2, int B,
                                                         long stride, float *__restrict__ s1, float *__restrict__ s2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 3) return;
  const int b = i / 3, c = i % 3;
  s1[(size_t)b * stride + c] = a1[b * 8 + c];
  s2[(size_t)b * stride + c] = a2[b * 8 + c];
}

// in (B, stride) -> out (B, 8): columns 0..2, then zeros
__global__ __launch_bounds__(256) void step_pad8_kernel(const float *__restrict__ g1, const float *__restrict__ g2, int B,
                                                        long stride, float *__restrict__ o1, float *__restrict__ o2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 8) return;
  const int b = i / 8, c = i % 8;
  o1[i] = c < 3 ? g1[(size_t)b * stride + c] : 0.f;
  o2[i] = c < 3 ? g2[(size_t)b * stride + c] : 0.f;
}

__global__ __launch_bounds__(256) void step_add_kernel(float *__restrict__ acc, const float *__restrict__ term, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) acc[i] = acc[i] + term[i];
}

// one block per pair.  w = sum(alpha) + sum(beta) as score_kernel forms it (per-thread fp64 partial sums over c = tid,
// tid + 256, ..., the same tree), rounded to float; then g_s1[b][c] = -g_score[b] * (alpha[c] / w), g_s2 likewise: a
// float quotient and a float product.
__global__ __launch_bounds__(256) void score_backward_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                             const float *__restrict__ g_score, int ctot,
                                                             float *__restrict__ g_s1, float *__restrict__ g_s2) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  double w = 0.0;
  for (int c = tid; c < ctot; c += 256) w += (double)alpha[c] + (double)beta[c];
  red[tid] = w;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const float wf = (float)red[0];
  const float ng = -g_score[b];
  for (int c = tid; c < ctot; c += 256) {
    g_s1[(size_t)b * ctot + c] = ng * (alpha[c] / wf);
    g_s2[(size_t)b * ctot + c] = ng * (beta[c] / wf);
  }
}

static int step_zero(void *out, long n, hipStream_t st) {
  TimedLaunch t(NQA_K_PREP, st);
  step_zero_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(static_cast<unsigned *>(out), n);
  return check_launch("step_zero");
}

// ---- the state block ------------------------------------------------------------------------------------------------
// Offsets in bytes from the start of the state, every region on a multiple of 256.
//   KEPT, written by the forward and only read by the backward:
//     act[l]     layer l's activation of y, l = 0..12 (NHWC, 4 bytes per element: float for the tapped layers 1, 3, 6, 9,
//                12 -- these ARE y's taps -- split16 records otherwise)
//     part[k]    tap k + 1's per-block fp64 partials (nqa_dists_stats_target_bytes)
//     sums0      tap 0's per-block fp64 sums (nqa_stats_scratch_bytes of the image and five one-pixel maps)
//     dummy      B zero floats: the one-pixel maps
//   SCRATCH behind it, one area laid out twice: the forward's temporaries are dead when it returns, and the backward
//   writes only here.
//     forward    pooled[s] the four L2-pooled maps (split16), a1 / a2 the (B, 8) similarities of tap 0
//     backward   gtap[k] the five masked tap gradients, gy0 tap 0's image term, g1p / g2p its (B, 8) upstream, coef /
//                coef0 the fp64 coefficient records, kexp / ktot the chain's exponents, expws the exponent reduction's
//                partials, gm the masked (split16 or half) operand of a data-gradient convolution, ga / gb its
//                float or half result, ping-pong
struct StepPlan {
  int h[5], w[5];
  size_t act[NQA_NUM_CONVS], part[5], part_bytes[5], sums0, sums0_bytes, dummy;
  size_t pooled[4], a1, a2;
  size_t gtap[5], gy0, g1p, g2p, coef, coef_bytes, coef0, coef0_bytes, kexp, ktot, expws, expws_bytes, gm, ga, gb;
  size_t kept, total;
};

static const int kTapLayer[5] = {1, 3, 6, 9, 12};
static const int kImgC[NQA_NUM_TAPS] = {3, 1, 1, 1, 1, 1};

static bool rung_valid(int grad_prec) { return grad_prec == NQA_PREC_F32S || grad_prec == NQA_PREC_F16; }

// The plan for (B, H, W, rung), or the code of the refusal with the message set under `who`.
static int step_plan(const char *who, int B, int H, int W, int grad_prec, StepPlan *p) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535) {
    set_error("%s: non-positive size or more than 65535 pairs (B=%d H=%d W=%d)", who, B, H, W);
    return NQA_E_ARG;
  }
  if (!rung_valid(grad_prec)) {
    set_error("%s: grad_prec %d is neither NQA_PREC_F32S nor NQA_PREC_F16", who, grad_prec);
    return NQA_E_ARG;
  }
  p->h[0] = H;
  p->w[0] = W;
  for (int s = 1; s < 5; ++s) {
    p->h[s] = (p->h[s - 1] + 1) / 2;
    p->w[s] = (p->w[s - 1] + 1) / 2;
  }
  // what the layers' own entry points refuse: a map of 2^31 bytes (their in-image byte offsets are 32-bit); and more
  // elements in a batch of maps than one launch of the element-wise kernels covers
  for (int l = 0; l < NQA_NUM_CONVS; ++l) {
    const int s = kConvs[l].stage, c = l == 0 ? 64 : (kConvs[l].cin > kConvs[l].cout ? kConvs[l].cin : kConvs[l].cout);
    if ((long)p->h[s] * p->w[s] * c * 4 >= (1L << 31)) {
      set_error("%s: %d x %d frames are too large: layer %d's %d x %d map of %d channels reaches 2^31 bytes", who, H, W, l,
                p->h[s], p->w[s], c);
      return NQA_E_SHAPE;
    }
  }
  if ((long)B * H * W * 64 > (1L << 36)) {
    set_error("%s: %d frames of %d x %d are more than one step takes (B * H * W * 64 > 2^36 elements): slice the batch", who,
              B, H, W);
    return NQA_E_SHAPE;
  }
  size_t at = 0;
  auto take = [&at](size_t bytes) {
    const size_t o = at;
    at = align_up(at + bytes, 256);
    return o;
  };
  size_t big = 0;  // the largest map a chain buffer holds, in elements
  for (int l = 0; l < NQA_NUM_CONVS; ++l) {
    const int s = kConvs[l].stage;
    const size_t px = (size_t)B * p->h[s] * p->w[s];
    p->act[l] = take(px * kConvs[l].cout * 4);
    const size_t e = px * (kConvs[l].cin > kConvs[l].cout ? kConvs[l].cin : kConvs[l].cout);
    if (l > 0 && e > big) big = e;
  }
  for (int k = 0; k < 5; ++k) {
    p->part_bytes[k] = nqa_dists_stats_target_bytes(B, p->h[k], p->w[k], kChns[k + 1]);
    p->part[k] = take(p->part_bytes[k]);
  }
  const int Hk[NQA_NUM_TAPS] = {H, 1, 1, 1, 1, 1}, Wk[NQA_NUM_TAPS] = {W, 1, 1, 1, 1, 1};
  p->sums0_bytes = nqa_stats_scratch_bytes(B, kImgC, Hk, Wk);
  p->sums0 = take(p->sums0_bytes);
  p->dummy = take((size_t)B * 4);
  p->kept = at;
  // the forward's temporaries
  for (int s = 0; s < 4; ++s) p->pooled[s] = take((size_t)B * p->h[s + 1] * p->w[s + 1] * kChns[s + 1] * 4);
  p->a1 = take((size_t)B * 8 * 4);
  p->a2 = take((size_t)B * 8 * 4);
  const size_t fwd_end = at;
  // the backward's, over the same area
  at = p->kept;
  size_t expws = 0;
  for (int k = 0; k < 5; ++k) {
    p->gtap[k] = take((size_t)B * p->h[k] * p->w[k] * kChns[k + 1] * 4);
    const size_t c = nqa_dists_stats_nhwc_backward_from_bytes(B, kChns[k + 1]);  // (one record buffer serves the taps in turn)
    if (k == 0 || c > p->coef_bytes) p->coef_bytes = c;
  }
  for (int l = 1; l < NQA_NUM_CONVS; ++l) {  // every map the exponent is taken of: g_taps[4], then each layer's input gradient
    const int s = kConvs[l].stage;
    const size_t a = nqa_grad_exponent_bytes(B, (long)p->h[s] * p->w[s] * kConvs[l].cin);
    const size_t b = nqa_grad_exponent_bytes(B, (long)p->h[s] * p->w[s] * kConvs[l].cout);
    if (a > expws) expws = a;
    if (b > expws) expws = b;
    if (l > 1 && kConvs[l].stage != kConvs[l - 1].stage) {  // behind a pool seam: the previous stage's tap
      const size_t t = nqa_grad_exponent_bytes(B, (long)p->h[s - 1] * p->w[s - 1] * kConvs[l].cin);
      if (t > expws) expws = t;
    }
  }
  p->gy0 = take((size_t)B * 3 * H * W * 4);
  p->g1p = take((size_t)B * 8 * 4);
  p->g2p = take((size_t)B * 8 * 4);
  p->coef = take(p->coef_bytes);
  p->coef0_bytes = nqa_stats_backward_bytes(B, kImgC);
  p->coef0 = take(p->coef0_bytes);
  p->kexp = take((size_t)B * 4);
  p->ktot = take((size_t)B * 4);
  p->expws_bytes = expws;
  p->expws = take(expws);
  p->gm = take(big * (grad_prec == NQA_PREC_F16 ? 2 : 4));
  p->ga = take(big * 4);  // (float behind a pool seam on both rungs)
  p->gb = take(big * 4);
  p->total = at > fwd_end ? at : fwd_end;
  return NQA_OK;
}

// What the two calls check alike, in this order: null pointers, the sizes and the rung, the shape, alignment, the
// state's size.  0 with the plan filled, or the code.
static int step_check(const char *who, bool null_ptr, const void *const *x_taps, int B, int H, int W, int grad_prec,
                      uintptr_t align4, uintptr_t align16, const void *state, size_t state_bytes, StepPlan *p) {
  if (null_ptr || !x_taps) {
    set_error("%s: null pointer", who);
    return NQA_E_ARG;
  }
  for (int k = 0; k < 5; ++k) {
    if (!x_taps[k]) {
      set_error("%s: null pointer (tap %d of the target)", who, k + 1);
      return NQA_E_ARG;
    }
    align16 |= (uintptr_t)x_taps[k];
  }
  if (int rc = step_plan(who, B, H, W, grad_prec, p)) return rc;
  if ((align4 & 3) || (align16 & 15) || ((uintptr_t)state & 255)) {
    set_error("%s: misaligned buffer (the state on 256 bytes, the taps and the packed layers on 16, every float array on 4)",
              who);
    return NQA_E_ARG;
  }
  if (state_bytes < p->total) {
    set_error("%s: state %zu < %zu bytes", who, state_bytes, p->total);
    return NQA_E_WORKSPACE;
  }
  return NQA_OK;
}

}  // namespace nqa

using namespace nqa;

extern "C" {

size_t nqa_dists_target_step_bytes(int B, int H, int W, int grad_prec) {
  StepPlan p = {};
  return step_plan("dists_target_step_bytes", B, H, W, grad_prec, &p) ? 0 : p.total;
}

int nqa_dists_target_step_forward(const float *x_nchw, const void *const *x_taps, const float *y_nchw, int B, int H, int W,
                                  const void *packed_w, int grad_prec, void *state, size_t state_bytes, float *s1, float *s2,
                                  void *stream) {
  const char *who = "dists_target_step_forward";
  StepPlan p = {};
  if (int rc = step_check(who, !x_nchw || !y_nchw || !packed_w || !state || !s1 || !s2, x_taps, B, H, W, grad_prec,
                          (uintptr_t)x_nchw | (uintptr_t)y_nchw | (uintptr_t)s1 | (uintptr_t)s2, (uintptr_t)packed_w, state,
                          state_bytes, &p))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(state);
  const int prec = NQA_PREC_F32S;
  int rc;
  // ---- one kept pyramid of y, layer by layer (autograd._pyramid_forward, keep=True) ----
  if ((rc = nqa_conv1_1(y_nchw, B, H, W, packed_w, prec, base + p.act[0], stream))) return rc;
  const void *in = base + p.act[0];
  for (int l = 1; l < NQA_NUM_CONVS; ++l) {
    const int s = kConvs[l].stage;
    if ((rc = nqa_conv3x3_relu(in, B, p.h[s], p.w[s], l, packed_w, prec, base + p.act[l], stream))) return rc;
    in = base + p.act[l];
    if (kConvs[l].last && s < 4) {
      if ((rc = nqa_l2pool(in, B, p.h[s], p.w[s], kConvs[l].cout, prec, base + p.pooled[s], stream))) return rc;
      in = base + p.pooled[s];
    }
  }
  // ---- taps 1..5: the sums and their fold (autograd.dists_target_stats) ----
  for (int k = 0; k < 5; ++k) {
    const int off = kChnOff[k + 1];
    if ((rc = nqa_dists_stats_target(static_cast<const float *>(x_taps[k]),
                                     reinterpret_cast<const float *>(base + p.act[kTapLayer[k]]), B, p.h[k], p.w[k],
                                     kChns[k + 1], base + p.part[k], p.part_bytes[k], s1 + off, s2 + off, NQA_TOTAL_CHNS,
                                     stream)))
      return rc;
  }
  // ---- tap 0: the images through the NCHW statistics beside five one-pixel zero maps (autograd._image_stats) ----
  if ((rc = step_zero(base + p.dummy, B, st))) return rc;
  const float *zero = reinterpret_cast<const float *>(base + p.dummy);
  const float *fx[NQA_NUM_TAPS] = {x_nchw, zero, zero, zero, zero, zero};
  const float *fy[NQA_NUM_TAPS] = {y_nchw, zero, zero, zero, zero, zero};
  const int Hk[NQA_NUM_TAPS] = {H, 1, 1, 1, 1, 1}, Wk[NQA_NUM_TAPS] = {W, 1, 1, 1, 1, 1};
  float *a1 = reinterpret_cast<float *>(base + p.a1), *a2 = reinterpret_cast<float *>(base + p.a2);
  if ((rc = nqa_dists_stats_nchw(fx, fy, B, kImgC, Hk, Wk, base + p.sums0, p.sums0_bytes, a1, a2, stream))) return rc;
  TimedLaunch t(NQA_K_PREP, st);
  step_cols3_kernel<<<cdiv(B * 3, 256), 256, 0, st>>>(a1, a2, B, NQA_TOTAL_CHNS, s1, s2);
  return check_launch("step_cols3");
}

int nqa_dists_target_step_backward(const float *x_nchw, const void *const *x_taps, const float *y_nchw, int B, int H, int W,
                                   const float *g_s1, const float *g_s2, const void *const *grad_layers,
                                   const float *w0_oihw_dev, int grad_prec, void *state, size_t state_bytes, float *gy_nchw,
                                   void *stream) {
  const char *who = "dists_target_step_backward";
  StepPlan p = {};
  uintptr_t a16 = 0;
  bool null_ptr = !x_nchw || !y_nchw || !g_s1 || !g_s2 || !grad_layers || !w0_oihw_dev || !state || !gy_nchw;
  for (int l = 0; grad_layers && l < 12; ++l) {
    null_ptr = null_ptr || !grad_layers[l];
    a16 |= (uintptr_t)grad_layers[l];
  }
  if (int rc = step_check(who, null_ptr, x_taps, B, H, W, grad_prec,
                          (uintptr_t)x_nchw | (uintptr_t)y_nchw | (uintptr_t)g_s1 | (uintptr_t)g_s2 | (uintptr_t)w0_oihw_dev |
                              (uintptr_t)gy_nchw,
                          a16, state, state_bytes, &p))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(state);
  const bool half = grad_prec == NQA_PREC_F16;
  int rc;
  // ---- taps 1..5: coefficients and gradient from the kept partials (autograd._dists_y_tap_grads) ----
  for (int k = 0; k < 5; ++k) {
    const int off = kChnOff[k + 1];
    if ((rc = nqa_dists_stats_nhwc_backward_from(static_cast<const float *>(x_taps[k]),
                                                 reinterpret_cast<const float *>(base + p.act[kTapLayer[k]]), B, p.h[k],
                                                 p.w[k], kChns[k + 1], base + p.part[k], p.part_bytes[k], g_s1 + off,
                                                 g_s2 + off, NQA_TOTAL_CHNS, base + p.coef, p.coef_bytes, nullptr,
                                                 reinterpret_cast<float *>(base + p.gtap[k]), stream)))
      return rc;
  }
  // ---- tap 0 from its kept sums (autograd._image_stats_grad_from) ----
  float *g1p = reinterpret_cast<float *>(base + p.g1p), *g2p = reinterpret_cast<float *>(base + p.g2p);
  {
    TimedLaunch t(NQA_K_PREP, st);
    step_pad8_kernel<<<cdiv(B * 8, 256), 256, 0, st>>>(g_s1, g_s2, B, NQA_TOTAL_CHNS, g1p, g2p);
    if ((rc = check_launch("step_pad8"))) return rc;
  }
  float *gy0 = reinterpret_cast<float *>(base + p.gy0);
  {
    const float *zero = reinterpret_cast<const float *>(base + p.dummy);
    const float *fx[NQA_NUM_TAPS] = {x_nchw, zero, zero, zero, zero, zero};
    const float *fy[NQA_NUM_TAPS] = {y_nchw, zero, zero, zero, zero, zero};
    const int Hk[NQA_NUM_TAPS] = {H, 1, 1, 1, 1, 1}, Wk[NQA_NUM_TAPS] = {W, 1, 1, 1, 1, 1};
    float *const gx[NQA_NUM_TAPS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float *const gy[NQA_NUM_TAPS] = {gy0, nullptr, nullptr, nullptr, nullptr, nullptr};
    if ((rc = nqa_dists_stats_nchw_backward(fx, fy, B, kImgC, Hk, Wk, base + p.sums0, p.sums0_bytes, g1p, g2p, base + p.coef0,
                                            p.coef0_bytes, gx, gy, stream)))
      return rc;
  }
  // ---- the chain (autograd.pyramid_backward_device, masked=True): exponent, mask, conv, pool seam ----
  int *kexp = reinterpret_cast<int *>(base + p.kexp), *ktot = reinterpret_cast<int *>(base + p.ktot);
  if ((rc = step_zero(ktot, B, st))) return rc;
  auto exponent = [&](const void *g, bool g_half, long per_image) {
    return half ? nqa_grad_exponent_half(g, g_half, B, per_image, base + p.expws, p.expws_bytes, kexp, ktot, stream)
                : nqa_grad_exponent(static_cast<const float *>(g), B, per_image, base + p.expws, p.expws_bytes, kexp, ktot,
                                    stream);
  };
  const void *g = base + p.gtap[4];
  bool g_half = false;  // g is float at the top and behind a pool seam, the rung's own type behind a convolution
  if ((rc = exponent(g, g_half, (long)p.h[4] * p.w[4] * 512))) return rc;
  void *bufs[2] = {base + p.ga, base + p.gb};
  int cur = -1;  // which of bufs holds g (-1: neither)
  for (int l = 12; l >= 1; --l) {
    const int s = kConvs[l].stage, cin = kConvs[l].cin, cout = kConvs[l].cout;
    const long px = (long)p.h[s] * p.w[s];
    const int act_split = kConvs[l].last ? 0 : 1;  // a tapped layer's output is a float map
    void *gm = base + p.gm;
    void *out = bufs[cur == 0 ? 1 : 0];
    if (half) {
      if ((rc = nqa_relu_mask_f16_scaled(g, g_half, base + p.act[l], act_split, B, px, cout, kexp, gm, stream))) return rc;
      if ((rc = nqa_conv3x3_half(gm, B, p.h[s], p.w[s], cout, cin, grad_layers[l - 1], out, stream))) return rc;
    } else {
      if ((rc = nqa_relu_mask_split16_scaled(static_cast<const float *>(g), base + p.act[l], act_split, B, px, cout, kexp, gm,
                                             stream)))
        return rc;
      if ((rc = nqa_conv3x3_split(gm, B, p.h[s], p.w[s], cout, cin, grad_layers[l - 1], 0, static_cast<float *>(out), stream)))
        return rc;
    }
    g = out;
    g_half = half;
    cur = cur == 0 ? 1 : 0;
    long per_image = px * cin;
    if (kConvs[l - 1].stage != s) {  // the layer read the L2-pool of the previous stage's tap
      const int t = s - 1;           // tap t + 1 = stage t's
      float *seam = static_cast<float *>(bufs[cur == 0 ? 1 : 0]);
      const float *tap = reinterpret_cast<const float *>(base + p.act[kTapLayer[t]]);
      const float *gt = reinterpret_cast<const float *>(base + p.gtap[t]);
      rc = half ? nqa_l2pool_backward_scaled_half(tap, g, gt, ktot, B, p.h[t], p.w[t], cin, seam, stream)
                : nqa_l2pool_backward_scaled(tap, static_cast<const float *>(g), gt, ktot, B, p.h[t], p.w[t], cin, seam,
                                             stream);
      if (rc) return rc;
      g = seam;
      g_half = false;
      cur = cur == 0 ? 1 : 0;
      per_image = (long)p.h[t] * p.w[t] * cin;
    }
    if ((rc = exponent(g, g_half, per_image))) return rc;
  }
  rc = half ? nqa_conv1_1_backward_scaled_half(g, base + p.act[0], w0_oihw_dev, kexp, ktot, B, H, W, gy_nchw, stream)
            : nqa_conv1_1_backward_scaled(static_cast<const float *>(g), base + p.act[0], w0_oihw_dev, kexp, ktot, B, H, W,
                                          gy_nchw, stream);
  if (rc) return rc;
  // ---- the image term of tap 0 ----
  const long n = (long)B * 3 * H * W;
  TimedLaunch t(NQA_K_PREP, st);
  step_add_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, st>>>(gy_nchw, gy0, n);
  return check_launch("step_add");
}

int nqa_dists_score_backward(const float *alpha, const float *beta, const float *g_score, int B, float *g_s1, float *g_s2,
                             void *stream) {
  if (!alpha || !beta || !g_score || !g_s1 || !g_s2) {
    set_error("dists_score_backward: null pointer");
    return NQA_E_ARG;
  }
  if (B <= 0) {
    set_error("dists_score_backward: non-positive B=%d", B);
    return NQA_E_ARG;
  }
  if (((uintptr_t)alpha | (uintptr_t)beta | (uintptr_t)g_score | (uintptr_t)g_s1 | (uintptr_t)g_s2) & 3) {
    set_error("dists_score_backward: misaligned buffer (every float array on 4 bytes)");
    return NQA_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  TimedLaunch t(NQA_K_PREP, st);
  score_backward_kernel<<<B, 256, 0, st>>>(alpha, beta, g_score, NQA_TOTAL_CHNS, g_s1, g_s2);
  return check_launch("dists_score_backward");
}

}  // extern "C"
