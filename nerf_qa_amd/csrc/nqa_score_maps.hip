// Score-map targets of the no-reference dataset prep on the device (SURVEY.md section 8, row f4's only caller:
// nerf_nr_qa_prep_4.py:71-133).  Per frame, from the K A-DISTS distortion maps of its K renders:
//
//   v_k   = double(max(map_k, 1e-10f))                       :71   clamp on the float32 tensor, then .double()
//   mean  = (sum_k v_k) / K,  std = sqrt(sum_k (v_k - mean)^2 / (K - 1))        :74-75  (K = 1: NaN, as torch.std)
//   log_max_q = -log10(amin q), log_min_q = -log10(amax q)   :78-94  for q in the K maps, std, mean (NaN propagates)
//   byte  = trunc(255 * (log_max - (-log10 q)) / (log_max - log_min)) if the spread is > 0 else 0      :105-133
//   rgb   = (mean, map k, std) per render, HWC                :131-134
//
// Three kernels, all fp64 streaming work bound by HBM: moments (mean / std maps and per-block min / max partials),
// fold (the partials of a frame to its 2K + 4 logs), quantise (bytes).  No atomics, one writer per partial, every
// fold in a fixed order: the outputs are bitwise repeatable.
#include <math.h>

#include "nqa_common.h"

namespace nqa {

static constexpr int kSmThreads = 256;
static constexpr int kSmPix = 4;                       // pixels per thread
static constexpr int kSmBlockPix = kSmThreads * kSmPix;  // pixels per block
static constexpr int kSmMaxK = 256;

// amin / amax: a NaN on either side wins (fmin / fmax would drop it)
template <typename T>
__device__ inline T nan_min(T a, T b) {
  return (b < a || b != b) ? b : a;
}
template <typename T>
__device__ inline T nan_max(T a, T b) {
  return (b > a || b != b) ? b : a;
}

__device__ inline float clamp_map(float v) { return v < 1e-10f ? 1e-10f : v; }  // NaN stays NaN, as torch.clamp

// THE -log10 of this file: the fold kernel forms log_max / log_min with it and the quantise kernel maps every pixel
// with it, so the extreme pixels land exactly on the values the formula gives them.  Not inlined: one body, one
// instruction sequence, whatever the compiler does around the two call sites.
__device__ __attribute__((noinline)) double neg_log10(double v) { return -log10(v); }

// One byte of :109/:115/:129 + :133.  A non-finite quotient (an infinite or NaN extreme) is 0.
__device__ inline uint32_t quantise(double v, double log_max, double log_min) {
#pragma clang fp contract(off)
  const double spread = log_max - log_min;
  if (!(spread > 0.0)) return 0;
  const double q = 255.0 * (log_max - neg_log10(v)) / spread;
  if (!(fabs(q) < __builtin_inf())) return 0;  // NaN, inf
  return (uint32_t)(int)q & 255u;              // (a finite q is within [0, 255] up to rounding)
}

// grid (blocks of kSmBlockPix pixels, F).  Thread t of block b owns pixels b * kSmBlockPix + j * kSmThreads + t.
// part: (F, K + 2, 2, nblk) double -- quantity q = k for map k, K for std, K + 1 for mean; [0] min, [1] max.
__global__ __launch_bounds__(kSmThreads) void score_maps_moments_kernel(const float *__restrict__ maps, int K, int HW,
                                                                        double *__restrict__ mean_out,
                                                                        double *__restrict__ std_out,
                                                                        double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float s_min[kSmMaxK + 2][kSmThreads / 64], s_max[kSmMaxK + 2][kSmThreads / 64];
  __shared__ double s_dmin[2][kSmThreads / 64], s_dmax[2][kSmThreads / 64];
  const int f = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int base = blockIdx.x * kSmBlockPix + tid;
  const float *m = maps + (size_t)f * K * HW;
  const float inf = __builtin_inff();

  double sum[kSmPix];
#pragma unroll
  for (int j = 0; j < kSmPix; ++j) sum[j] = 0.0;
  for (int k = 0; k < K; ++k) {
    float mn = inf, mx = -inf;
#pragma unroll
    for (int j = 0; j < kSmPix; ++j) {
      const int i = base + j * kSmThreads;
      if (i < HW) {
        const float v = clamp_map(m[(size_t)k * HW + i]);
        sum[j] += (double)v;
        mn = nan_min(mn, v);
        mx = nan_max(mx, v);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      mn = nan_min(mn, __shfl_xor(mn, o));
      mx = nan_max(mx, __shfl_xor(mx, o));
    }
    if (lane == 0) {
      s_min[k][wave] = mn;
      s_max[k][wave] = mx;
    }
  }

  double smn = (double)inf, smx = -(double)inf, mmn = (double)inf, mmx = -(double)inf;
#pragma unroll
  for (int j = 0; j < kSmPix; ++j) {
    const int i = base + j * kSmThreads;
    if (i < HW) {
      const double mean = sum[j] / (double)K;
      double ss = 0.0;
      for (int k = 0; k < K; ++k) {
        const double d = (double)clamp_map(m[(size_t)k * HW + i]) - mean;
        ss += d * d;
      }
      const double sd = sqrt(ss / (double)(K - 1));  // K = 1: 0 / 0
      mean_out[(size_t)f * HW + i] = mean;
      std_out[(size_t)f * HW + i] = sd;
      smn = nan_min(smn, sd);
      smx = nan_max(smx, sd);
      mmn = nan_min(mmn, mean);
      mmx = nan_max(mmx, mean);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    smn = nan_min(smn, __shfl_xor(smn, o));
    smx = nan_max(smx, __shfl_xor(smx, o));
    mmn = nan_min(mmn, __shfl_xor(mmn, o));
    mmx = nan_max(mmx, __shfl_xor(mmx, o));
  }
  if (lane == 0) {
    s_dmin[0][wave] = smn;
    s_dmax[0][wave] = smx;
    s_dmin[1][wave] = mmn;
    s_dmax[1][wave] = mmx;
  }
  __syncthreads();
  for (int q = tid; q < K + 2; q += kSmThreads) {
    double mn, mx;
    if (q < K) {
      mn = (double)s_min[q][0], mx = (double)s_max[q][0];
      for (int w = 1; w < kSmThreads / 64; ++w) {
        mn = nan_min(mn, (double)s_min[q][w]);
        mx = nan_max(mx, (double)s_max[q][w]);
      }
    } else {
      mn = s_dmin[q - K][0], mx = s_dmax[q - K][0];
      for (int w = 1; w < kSmThreads / 64; ++w) {
        mn = nan_min(mn, s_dmin[q - K][w]);
        mx = nan_max(mx, s_dmax[q - K][w]);
      }
    }
    double *p = part + (((size_t)f * (K + 2) + q) * 2) * nblk + blockIdx.x;
    p[0] = mn;
    p[nblk] = mx;
  }
}

// grid (K + 2, F): one block folds the nblk partials of one quantity of one frame, thread t the partials t, t + 256, ...
// in ascending order, then a fixed tree over the threads; thread 0 writes the two logs.
__global__ __launch_bounds__(kSmThreads) void score_maps_fold_kernel(const double *__restrict__ part, int K, int nblk,
                                                                     double *__restrict__ logs) {
  __shared__ double s_mn[kSmThreads], s_mx[kSmThreads];
  const int q = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const double *p = part + (((size_t)f * (K + 2) + q) * 2) * nblk;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  for (int b = tid; b < nblk; b += kSmThreads) {
    mn = nan_min(mn, p[b]);
    mx = nan_max(mx, p[nblk + b]);
  }
  s_mn[tid] = mn;
  s_mx[tid] = mx;
  __syncthreads();
  for (int o = kSmThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_mn[tid] = nan_min(s_mn[tid], s_mn[tid + o]);
      s_mx[tid] = nan_max(s_mx[tid], s_mx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    double *l = logs + (size_t)f * (2 * K + 4);
    const int at_max = q < K ? q : 2 * K + 2 * (q - K), at_min = q < K ? K + q : at_max + 1;
    l[at_max] = neg_log10(s_mn[0]);
    l[at_min] = neg_log10(s_mx[0]);
  }
}

// grid (blocks of kSmBlockPix pixels, F * K).  A thread owns kSmPix CONSECUTIVE pixels of one render's image: their
// 3 * kSmPix bytes are three whole dwords where the address allows it (it does not at the ragged end of a plane, nor
// in an image that starts off a dword boundary: odd H * W), single bytes otherwise.
__global__ __launch_bounds__(kSmThreads) void score_maps_quantise_kernel(const float *__restrict__ maps,
                                                                         const double *__restrict__ mean,
                                                                         const double *__restrict__ sd,
                                                                         const double *__restrict__ logs, int K, int HW,
                                                                         uint8_t *__restrict__ rgb) {
  static_assert(kSmPix == 4, "twelve bytes = three dwords per thread");
  const int fk = blockIdx.y, f = fk / K, k = fk - f * K;
  const int i0 = (blockIdx.x * kSmThreads + threadIdx.x) * kSmPix;
  if (i0 >= HW) return;
  const double *l = logs + (size_t)f * (2 * K + 4);
  const double map_max = l[k], map_min = l[K + k], std_max = l[2 * K], std_min = l[2 * K + 1];
  const double mean_max = l[2 * K + 2], mean_min = l[2 * K + 3];
  const float *m = maps + (size_t)fk * HW;
  const double *mu = mean + (size_t)f * HW, *s = sd + (size_t)f * HW;
  const int n = HW - i0 < kSmPix ? HW - i0 : kSmPix;
  uint32_t b[3 * kSmPix];
#pragma unroll
  for (int j = 0; j < kSmPix; ++j) {
    const bool in = j < n;
    b[3 * j + 0] = in ? quantise(mu[i0 + j], mean_max, mean_min) : 0;
    b[3 * j + 1] = in ? quantise((double)clamp_map(m[i0 + j]), map_max, map_min) : 0;
    b[3 * j + 2] = in ? quantise(s[i0 + j], std_max, std_min) : 0;
  }
  uint8_t *out = rgb + ((size_t)fk * HW + i0) * 3;
  if (n == kSmPix && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 3 * kSmPix; ++j)
      if (j < 3 * n) out[j] = (uint8_t)b[j];
  }
}

// The workspace: mean (F, HW) double | std (F, HW) double | partials (F, K + 2, 2, nblk) double, each on 256 bytes.
struct ScoreMapsPlan {
  int HW, nblk;
  size_t plane_bytes, part_bytes;
};

// 0: the sizes run; otherwise the refusal's message is set under `who`.
static int score_maps_plan(const char *who, int F, int K, int H, int W, ScoreMapsPlan &p) {
  if (F <= 0 || K <= 0 || H <= 0 || W <= 0) {
    set_error("%s: non-positive size F=%d K=%d H=%d W=%d", who, F, K, H, W);
    return NQA_E_ARG;
  }
  if (K > kSmMaxK) {
    set_error("%s: K=%d renders per frame, more than %d", who, K, kSmMaxK);
    return NQA_E_ARG;
  }
  if ((long)F * K > 65535) {  // F * K rides in gridDim.y
    set_error("%s: F*K=%ld images, more than 65535", who, (long)F * K);
    return NQA_E_ARG;
  }
  if ((long)H * W >= (1L << 31) || (long)F * K * ((long)H * W) * 3 >= (1L << 31)) {
    set_error("%s: F*K*H*W*3 reaches 2^31 bytes (F=%d K=%d H=%d W=%d)", who, F, K, H, W);
    return NQA_E_ARG;
  }
  p.HW = H * W;
  p.nblk = cdiv(p.HW, kSmBlockPix);
  p.plane_bytes = align_up((size_t)F * p.HW * sizeof(double), 256);
  p.part_bytes = align_up((size_t)F * (K + 2) * 2 * p.nblk * sizeof(double), 256);
  return NQA_OK;
}

}  // namespace nqa

using namespace nqa;

extern "C" {

size_t nqa_score_maps_workspace_bytes(int F, int K, int H, int W) {
  ScoreMapsPlan p;
  if (score_maps_plan("score_maps_workspace_bytes", F, K, H, W, p)) return 0;
  return 2 * p.plane_bytes + p.part_bytes;
}

int nqa_score_maps(const float *maps, int F, int K, int H, int W, void *workspace, size_t workspace_bytes, uint8_t *rgb,
                   double *logs, void *stream) {
  if (!maps || !workspace || !rgb || !logs) {
    set_error("score_maps: null pointer");
    return NQA_E_ARG;
  }
  ScoreMapsPlan p;
  if (int rc = score_maps_plan("score_maps", F, K, H, W, p)) return rc;
  const size_t need = 2 * p.plane_bytes + p.part_bytes;
  if (workspace_bytes < need) {
    set_error("score_maps: workspace %zu < %zu bytes", workspace_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(workspace);
  double *mean = reinterpret_cast<double *>(base), *sd = reinterpret_cast<double *>(base + p.plane_bytes);
  double *part = reinterpret_cast<double *>(base + 2 * p.plane_bytes);
  TimedLaunch t(NQA_K_PREP, st);
  score_maps_moments_kernel<<<dim3(p.nblk, F), kSmThreads, 0, st>>>(maps, K, p.HW, mean, sd, part);
  score_maps_fold_kernel<<<dim3(K + 2, F), kSmThreads, 0, st>>>(part, K, p.nblk, logs);
  score_maps_quantise_kernel<<<dim3(p.nblk, F * K), kSmThreads, 0, st>>>(maps, mean, sd, logs, K, p.HW, rgb);
  return check_launch("score_maps");
}

}  // extern "C"
