// A-DISTS on gfx950: everything after the two VGG pyramids of ADISTS.forward
// (nerf_qa/ADISTS/ADISTS.py:137-197, as_map=False).
//
// The reference runs, per stage, 2 depthwise 21x21 Gaussian convolutions for the texture
// probability (compute_prob, :71-100) and 5 more for the windowed T/S maps (:165-183), on
// L2-normalised features.  Three observations shape the kernels here:
//   * the window is an outer product (:106-110), so each filter is two 21-tap passes;
//   * F.normalize(f, dim=(2,3)) is one scalar per (image, channel), so the windowed moments
//     of the normalised maps are the moments of the raw maps times inv_x, inv_y, inv_x^2 ...;
//     the raw x moments also give compute_prob's mean/variance -- one windowed pass serves both;
//   * D = sum_c w_c mean_hw((1-ps) T_c + ps S_c) = mean_hw((1-ps) TW + ps SW) with
//     TW = sum_c w_c T_c, SW = sum_c w_c S_c, so the heavy pass reduces over channels and
//     leaves three small (B,h-20,w-20) maps; the coarse-to-fine probability chain then
//     works on those maps only.
// Global per-(image,channel) sums come from the DISTS statistics kernels (fp64).
#include <math.h>
#include <string.h>

#include "nqa_regw.h"
#include "nqa_stages.h"

namespace nqa {

static constexpr int kWin = 21;                  // the window of the three specialised kernels, and of the old entry points
static constexpr int kWinMin = 3, kWinMax = 63;  // what the generic kernels take (nqa_window_n.h derives the upper end)
static constexpr int kChainBlocks = 1024;  // most blocks per image of the chain's reduction kernels

// tuning hook (nqa_set_conv_variant bit 3): the per-wave-loads form of the window pass, kept for A/B timing
static bool adists_window_legacy() { return tuning().window_legacy; }
static bool adists_window_generic() { return tuning().window_generic; }

struct Gauss {
  float g[kWin];
};

// ---------------------------------------------------------------------------------
// (b,3,H,W) float32 NCHW -> (b,H,W,4) float32 NHWC with a zero 4th channel (stage 0)
__global__ __launch_bounds__(256) void nchw3_to_nhwc4_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                             int HW) {
  const int p = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (p >= HW) return;
  const float *s = in + (size_t)n * 3 * HW;
  f32x4 v = {s[p], s[HW + p], s[2 * HW + p], 0.f};
  *reinterpret_cast<f32x4 *>(out + ((size_t)n * HW + p) * 4) = v;
}

// ---------------------------------------------------------------------------------
// Per (b, channel) scalars from the fp64 partial sums (layout of stats_*_kernel):
//   q[0]=inv_x  q[1]=inv_y   1/max(||f||_2, 1e-12)               (ADISTS.py:130,166-167)
//   q[2]=sum_x               for the entropy normalisation       (:132)
//   q[3..7]= mean_x mean_y var_x var_y cov of the RAW maps (population), for the global branch
// s: the five sums of one (pair, channel) over hw pixels; o its place in a row of q, st the row length.
__device__ inline void prep_store(const double (&s)[5], int hw, size_t o, size_t st, float *__restrict__ q) {
  const double inv = 1.0 / (double)hw;
  const double mx = s[0] * inv, my = s[1] * inv;
  q[0 * st + o] = (float)(1.0 / fmax(sqrt(s[2]), 1e-12));
  q[1 * st + o] = (float)(1.0 / fmax(sqrt(s[3]), 1e-12));
  q[2 * st + o] = (float)s[0];
  q[3 * st + o] = (float)mx;
  q[4 * st + o] = (float)my;
  q[5 * st + o] = (float)(s[2] * inv - mx * mx);
  q[6 * st + o] = (float)(s[3] * inv - my * my);
  q[7 * st + o] = (float)(s[4] * inv - mx * my);
}

__global__ __launch_bounds__(256) void adists_prep_kernel(const double *__restrict__ part, StageDesc d,
                                                          float *__restrict__ q /* [8][B][ctot] */, int B) {
  const int b = blockIdx.y;
  const int gc = blockIdx.x * 256 + threadIdx.x;
  if (gc >= d.ctot) return;
  int k = 0;
  while (k + 1 < d.nstage && gc >= d.coff[k + 1]) ++k;
  const int c = gc - d.coff[k];
  const double *p = part + d.part_off[k] + ((size_t)b * d.nblk[k] * d.c[k] + c) * 5;
  double s[5] = {0, 0, 0, 0, 0};
  for (int blk = 0; blk < d.nblk[k]; ++blk)
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] += p[(size_t)blk * d.c[k] * 5 + j];
  prep_store(s, d.hw[k], (size_t)b * d.ctot + gc, (size_t)B * d.ctot, q);
}

// The same scalars for the group forward, one WAVE per (pair, channel): the group statistics kernels cut a tap into
// strips that fit a block's registers (up to 8100 blocks per pair for relu1_2 at 1080p, where the pairwise passes leave
// at most ~1000), and one thread walking them alone took 2.8 ms of a 21 ms call.
// The lanes stride over the blocks and a shuffle tree adds them, the order of plane_moments / finalize_kernel.
__global__ __launch_bounds__(256) void adists_prep_group_kernel(const double *__restrict__ part, StageDesc d,
                                                                float *__restrict__ q /* [8][B][ctot] */, int B) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int gc = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gc >= d.ctot) return;
  int k = 0;
  while (k + 1 < d.nstage && gc >= d.coff[k + 1]) ++k;
  const int c = gc - d.coff[k];
  const double *p = part + d.part_off[k] + ((size_t)b * d.nblk[k] * d.c[k] + c) * 5;
  double s[5] = {0, 0, 0, 0, 0};
  for (int blk = lane; blk < d.nblk[k]; blk += 64)
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] += p[(size_t)blk * d.c[k] * 5 + j];
#pragma unroll
  for (int j = 0; j < 5; ++j)
    for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, 64);
  if (lane != 0) return;
  prep_store(s, d.hw[k], (size_t)b * d.ctot + gc, (size_t)B * d.ctot, q);
}

// ---------------------------------------------------------------------------------
// Spatial entropy of the x maps (ADISTS.py:127-133): p = relu(f)*inv; p /= sum(p)+c0;
// H = -sum p log2(p + c0).  Partial sums per block, part[(b*nblk+blk)*C + c].
template <typename P>
__global__ __launch_bounds__(256) void entropy_nhwc_kernel(const typename P::T *__restrict__ feat, int HW, int C,
                                                           int pix_per_block, const float *__restrict__ invx,
                                                           const float *__restrict__ sumx, int ctot,
                                                           double *__restrict__ part) {
  typedef typename P::T T;
  typedef __attribute__((ext_vector_type(P::CPC))) T tvec;
  __shared__ double red[256 * P::CPC];
  const int tid = threadIdx.x, b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int G = C / P::CPC, PL = 256 / G;
  const int g = tid % G, pl = tid / G;
  float inv[P::CPC], den[P::CPC];
#pragma unroll
  for (int e = 0; e < P::CPC; ++e) {
    inv[e] = invx[(size_t)b * ctot + g * P::CPC + e];
    den[e] = inv[e] * sumx[(size_t)b * ctot + g * P::CPC + e] + 1e-12f;
  }
  double acc[P::CPC];
#pragma unroll
  for (int e = 0; e < P::CPC; ++e) acc[e] = 0.0;
  const T *f = feat + (size_t)b * HW * C + g * P::CPC;
  const int p_end = min(HW, (blk + 1) * pix_per_block);
  for (int p = blk * pix_per_block + pl; p < p_end; p += PL) {
    const tvec v = *reinterpret_cast<const tvec *>(f + (size_t)p * C);
#pragma unroll
    for (int e = 0; e < P::CPC; ++e) {
      const float pn = fmaxf(P::to_f(v[e]), 0.f) * inv[e] / den[e];
      acc[e] += (double)(-pn * log2f(pn + 1e-12f));
    }
  }
#pragma unroll
  for (int e = 0; e < P::CPC; ++e) red[tid * P::CPC + e] = acc[e];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int cg = c / P::CPC, ce = c % P::CPC;
    double s = 0.0;
    for (int q = 0; q < PL; ++q) s += red[(q * G + cg) * P::CPC + ce];
    part[((size_t)b * nblk + blk) * C + c] = s;
  }
}

// Channel weights (ADISTS.py:134-135,154-160): per stage H/(sum_stage H + c0)*C, then over
// all 1475: /sum, clamp to mean +- 0.5*population std, /sum.  One block per image.
struct EntDesc {
  long part_off[NQA_NUM_TAPS];
  int nblk[NQA_NUM_TAPS];
  int c[NQA_NUM_TAPS];      // padded channel count used by the partial layout (stage 0: 4)
  int creal[NQA_NUM_TAPS];  // real channels
  int coff[NQA_NUM_TAPS];
  int ctot;
};

// fold the per-block entropy partials: one wave per (image, channel) -> hsum[b][ctot]
__global__ __launch_bounds__(256) void adists_entropy_fold_kernel(const double *__restrict__ part, EntDesc d,
                                                                  float *__restrict__ hsum) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int gc = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gc >= d.ctot) return;
  int k = 0;
  while (k + 1 < NQA_NUM_TAPS && gc >= d.coff[k + 1]) ++k;
  const int c = gc - d.coff[k];
  const double *p = part + d.part_off[k] + (size_t)b * d.nblk[k] * d.c[k] + c;
  double s = 0.0;
  for (int blk = lane; blk < d.nblk[k]; blk += 64) s += p[(size_t)blk * d.c[k]];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) hsum[(size_t)b * d.ctot + gc] = (float)s;
}

__global__ __launch_bounds__(256) void adists_weights_kernel(const float *__restrict__ hsum, EntDesc d,
                                                             float *__restrict__ wgt /* [B][ctot] */) {
  __shared__ float h[NQA_TOTAL_CHNS];
  __shared__ double red[256];
  __shared__ double bc[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  auto block_sum = [&](double v) -> double {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    return red[0];
  };
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    double loc = 0.0;
    for (int c = tid; c < d.creal[k]; c += 256) {
      const float s = hsum[(size_t)b * d.ctot + d.coff[k] + c];
      h[d.coff[k] + c] = s;
      loc += (double)s;
    }
    const float tot = (float)block_sum(loc);
    for (int c = tid; c < d.creal[k]; c += 256)
      h[d.coff[k] + c] = h[d.coff[k] + c] / (tot + 1e-12f) * (float)d.creal[k];
  }
  __syncthreads();
  double loc = 0.0;
  for (int c = tid; c < d.ctot; c += 256) loc += (double)h[c];
  const float s0 = (float)block_sum(loc);
  for (int c = tid; c < d.ctot; c += 256) h[c] = h[c] / s0;
  __syncthreads();
  loc = 0.0;
  for (int c = tid; c < d.ctot; c += 256) loc += (double)h[c];
  const float mean = (float)(block_sum(loc) / d.ctot);
  loc = 0.0;
  for (int c = tid; c < d.ctot; c += 256) {
    const float dv = h[c] - mean;
    loc += (double)(dv * dv);
  }
  const float sd = sqrtf((float)(block_sum(loc) / d.ctot));
  const float lo = mean - 0.5f * sd, hi = mean + 0.5f * sd;
  loc = 0.0;
  for (int c = tid; c < d.ctot; c += 256) {
    h[c] = fminf(fmaxf(h[c], lo), hi);
    loc += (double)h[c];
  }
  const float s1 = (float)block_sum(loc);
  (void)bc;
  for (int c = tid; c < d.ctot; c += 256) wgt[(size_t)b * d.ctot + c] = h[c] / s1;
}

// ---------------------------------------------------------------------------------
// The windowed pass for the NHWC taps (stages 1..5), lanes = channels.
//
// A wave owns one output column x of image pair b and a strip of up to 64 output rows, and walks
// down the input rows with one channel per lane (so every load is a coalesced 64-channel row of
// one pixel and nothing goes through LDS).  Per input row it takes the 21-tap HORIZONTAL sums of
// the five products from 21+21 neighbour loads, pushes them into a 21-row ring held in registers
// (105 VGPRs), and once the ring is full takes the 21-tap VERTICAL sums -- the ring is never
// rotated: slot s of phase j gets weight g[(s-j-1) mod 21], read as 21 consecutive scalars of a
// doubled table.  That is the separable minimum of 2 x 21 x 5 FMAs per (pixel, channel).
// T, S and the gamma term follow per lane; a 64-lane butterfly sums them over channels and the
// total is banked in the accumulator of lane (row - strip start), so the strip's three output
// columns leave as plain stores after the last channel block: no atomics, deterministic.
typedef __attribute__((ext_vector_type(2))) float f32x2;

// a / b to ~1.5 ulp from v_rcp_f32 and one Newton step: 4 instructions where the IEEE sequence is ~10.
// Used for the three quotients per (output row, channel) of the window pass (b > 0 there).
__device__ inline float div_nr(float a, float b) {
  float r = __builtin_amdgcn_rcpf(b);
  r = fmaf(fmaf(-b, r, 1.f), r, r);
  return a * r;
}

// One DPP move of a float (ctrl is an instruction immediate); lanes outside row_mask get 0.
template <int CTRL, int ROW_MASK>
__device__ inline float dpp0(float v) {
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
// Sum over the 64 lanes, valid in lane 63, broadcast through an SGPR: six DPP adds (quad swaps,
// half-row and row mirrors, then the two row broadcasts) instead of six LDS-crossbar bpermutes.
__device__ inline float wave_sum(float v) {
  v += dpp0<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v += dpp0<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v += dpp0<0x141, 0xF>(v);  // row_half_mirror
  v += dpp0<0x140, 0xF>(v);  // row_mirror: every lane of a 16-lane row holds the row's sum
  v += dpp0<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v += dpp0<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Three wave sums at once (same adds in the same order as wave_sum, valid in lane 63).  Written as one block of
// v_add_f32_dpp: left to hipcc each step is a zeroing move + a DPP move + an add, the three chains run one after
// the other and every DPP waits two states on the add before it (~42 vector instructions and ~15 s_nop per
// output row); interleaved, the other two chains ARE the two wait states (18 instructions, no s_nop).
__device__ inline void wave_sum3(float &a, float &b, float &c) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass would hand the block to the x86 assembler)
#define NQA_DPP3(CTRL, TAIL)                                        \
  "v_add_f32_dpp %0, %0, %0 " CTRL " bank_mask:0xf" TAIL "\n\t"     \
  "v_add_f32_dpp %1, %1, %1 " CTRL " bank_mask:0xf" TAIL "\n\t"     \
  "v_add_f32_dpp %2, %2, %2 " CTRL " bank_mask:0xf" TAIL "\n\t"
  asm volatile("s_nop 1\n\t"  // the operands may come straight out of the preceding vector instruction
               NQA_DPP3("quad_perm:[1,0,3,2] row_mask:0xf", " bound_ctrl:1")
               NQA_DPP3("quad_perm:[2,3,0,1] row_mask:0xf", " bound_ctrl:1")
               NQA_DPP3("row_half_mirror row_mask:0xf", " bound_ctrl:1")
               NQA_DPP3("row_mirror row_mask:0xf", " bound_ctrl:1")
               NQA_DPP3("row_bcast:15 row_mask:0xa", "")
               NQA_DPP3("row_bcast:31 row_mask:0xc", "")
               "s_nop 1"
               : "+v"(a), "+v"(b), "+v"(c));
#undef NQA_DPP3
  a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), 63));
  b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, b), 63));
  c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 63));
#endif
}

// The GROUP forms of the three window kernels and of the global branch (nqa_adists_forward_group): K renders per
// reference, pair b = r * K + k.  Pair b reads its x maps from reference image xi = b / K and its channel weights from
// row xi, its y maps and its q rows from pair b; tw / sw are written per pair, gamma -- a function of x alone -- once per
// reference, by the k = 0 pair, at image xi.  The pairwise kernels are the same bodies with xi = b, every pair writing
// its gamma.  The arithmetic of a pair is the same in both.
template <typename P, int C>  // C (64..512) is a template parameter so tap strides fold into load immediates
__global__ __launch_bounds__(256, 2) void adists_window_lanes_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, Gauss gw,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw) {
#define NQA_LANES_GROUP 0
#include "nqa_window_lanes_body.h"
#undef NQA_LANES_GROUP
}
template <typename P, int C>
__global__ __launch_bounds__(256, 2) void adists_window_lanes_group_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, Gauss gw,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int K) {
#define NQA_LANES_GROUP 1
#include "nqa_window_lanes_body.h"
#undef NQA_LANES_GROUP
}

// gaussian(21, 7) as ADISTS.py:102-104 builds it (float32(exp(.)) / float32 sum), as compile-time constants:
// make_gauss() recomputes the taps at run time and adists_run refuses to start if the two disagree.
// As literals the taps are instruction immediates (v_fmac_f32 / v_mul_f32 with a 32-bit constant): no scalar
// registers, no broadcast moves -- the packed-float form above kept them in SGPRs, spilled 40-80 of them and
// built a {w, w} register pair per tap for every v_pk_fma_f32, which on this chip issues at half the rate of
// v_fma_f32 anyway.
static constexpr float kG[kWin] = {
    0x1.8453aep-6f, 0x1.d76892p-6f, 0x1.185a34p-5f, 0x1.46b8bap-5f, 0x1.75117ap-5f, 0x1.a16246p-5f, 0x1.c987c2p-5f,
    0x1.eb6810p-5f, 0x1.02907ep-4f, 0x1.0a9a20p-4f, 0x1.0d5620p-4f, 0x1.0a9a20p-4f, 0x1.02907ep-4f, 0x1.eb6810p-5f,
    0x1.c987c2p-5f, 0x1.a16246p-5f, 0x1.75117ap-5f, 0x1.46b8bap-5f, 0x1.185a34p-5f, 0x1.d76892p-6f, 0x1.8453aep-6f};

// the last 21 rows' horizontal sums of the five products, one ring slot per row
struct WinRing {
  float s0[kWin], s1[kWin], s2[kWin], s3[kWin], s4[kWin];
};

// One input row of the separable window: horizontal 21-tap sums of (x, y, x^2, y^2, xy) into ring slot SLOT
// (a compile-time constant, so the ring stays in registers and is never rotated); when `full`, the vertical
// 21-tap sums over the ring -- slot s carries weight kG[(20 - SLOT + s) mod 21] at this phase -- and from them
// the gamma term (ADISTS.py:84-86), T and S (:182-183) of this lane's channel.
template <int SLOT>
__device__ inline void win_row(const float (&x)[kWin], const float (&y)[kWin], WinRing &rg, bool full, float ix,
                               float iy, float wc, float &gterm, float &tt, float &ss) {
  // the window is symmetric (kG[j] == kG[20-j]): the centre tap starts the five sums (no zero + fma), every
  // mirrored pair of taps adds its two samples / squares / products first and takes ONE weighted fma per sum:
  // 13 operations per pair where tap-by-tap took 14, and no accumulator initialisation
  constexpr int MID = kWin / 2;
  static_assert(kWin == 21 && kG[0] == kG[20] && kG[3] == kG[17] && kG[9] == kG[11], "the window must be symmetric");
  float h0, h1, h2, h3, h4;
  {
    const float gx = kG[MID] * x[MID], gy = kG[MID] * y[MID];
    h0 = gx;
    h1 = gy;
    h2 = gx * x[MID];
    h3 = gy * y[MID];
    h4 = gx * y[MID];
  }
#pragma unroll
  for (int j = 0; j < MID; ++j) {
    const int k = kWin - 1 - j;
    const float sx = x[j] + x[k], sy = y[j] + y[k];
    const float uu = fmaf(x[k], x[k], x[j] * x[j]), vv = fmaf(y[k], y[k], y[j] * y[j]);
    const float ww = fmaf(x[k], y[k], x[j] * y[j]);
    h0 = fmaf(kG[j], sx, h0);
    h1 = fmaf(kG[j], sy, h1);
    h2 = fmaf(kG[j], uu, h2);
    h3 = fmaf(kG[j], vv, h3);
    h4 = fmaf(kG[j], ww, h4);
  }
  rg.s0[SLOT] = h0;
  rg.s1[SLOT] = h1;
  rg.s2[SLOT] = h2;
  rg.s3[SLOT] = h3;
  rg.s4[SLOT] = h4;
  if (full) {
    // slot 0 starts the vertical sums (a product, not zero + fma)
    constexpr float w0 = kG[(kWin - 1 - SLOT) % kWin];
    float m0 = w0 * rg.s0[0], m1 = w0 * rg.s1[0], m2 = w0 * rg.s2[0], m3 = w0 * rg.s3[0], m4 = w0 * rg.s4[0];
#pragma unroll
    for (int sl = 1; sl < kWin; ++sl) {
      const float wv = kG[(kWin - 1 - SLOT + sl) % kWin];
      m0 = fmaf(wv, rg.s0[sl], m0);
      m1 = fmaf(wv, rg.s1[sl], m1);
      m2 = fmaf(wv, rg.s2[sl], m2);
      m3 = fmaf(wv, rg.s3[sl], m3);
      m4 = fmaf(wv, rg.s4[sl], m4);
    }
    gterm = div_nr(m2 - m0 * m0, m0 + 1e-12f);
    const float mx = ix * m0, my = iy * m1;
    const float vx = ix * ix * m2 - mx * mx, vy = iy * iy * m3 - my * my;
    const float cov = ix * iy * m4 - mx * my;
    tt = wc * div_nr(2.f * mx * my + 1e-6f, mx * mx + my * my + 1e-6f);
    ss = wc * div_nr(2.f * cov + 1e-6f, vx + vy + 1e-6f);
  }
}

// The same pass with the taps shared through LDS (the shipped form).  The kernel above lets every wave fetch its
// own 2 x 21 neighbour pixels per input row from L1: 42 wave-wide loads per output row, of which a block's four
// adjacent columns share 21 of every 24 pixels -- measured L1/TA-bound, and with workgroups dealt round-robin
// over the 8 XCDs every pixel was fetched into up to six L2s (rocprofv3: 32 GB fetched for a 4.2 GB tap,
// L2 hit rate 0.43, the dispatch HBM-bound at 5.6 TB/s).  Here
//   * workgroup ids are remapped so that the ids that share an XCD (equal mod 8) own a contiguous run of
//     column groups: neighbouring columns' rows hit one L2 (speed only; any placement is correct);
//   * a block (4 waves = 4 adjacent output columns) brings each input row's 24-pixel window of both images
//     into LDS ONCE by LDS-DMA (1-KB pieces, 3 per wave and row instead of 42 loads), three rows ahead of
//     their use in a four-slot ring, retired by a counted vmcnt + one barrier per row;
//   * the 42 taps of a wave are ds_read_b32 at immediate offsets from one address register.
// The arithmetic (horizontal sums, 21-row register ring, vertical sums, T / S / gamma, channel reduction) is
// the kernel above, instruction for instruction.

template <typename P, int C, bool GRP>  // (GRP: the group form, see adists_window_lanes_kernel)
__device__ __forceinline__ void window_lds_body(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, Gauss gw,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int nbx, int nby, int strip, int K) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)gw;  // the taps are the compile-time constants kG (checked against make_gauss() on the host)
  typedef typename P::T T;
  constexpr int SZ = (int)sizeof(T);
  constexpr int PXB = 64 * SZ;              // one pixel's 64-channel block, bytes
  constexpr int PPP = 1024 / PXB;           // pixels per 1-KB DMA piece: 4 (float) or 8 (16-bit)
  constexpr int PPI = SZ == 4 ? 6 : 4;      // pieces per image and row: 24 pixels (float), padded to 32 (16-bit)
  constexpr int WPX = PPI * PPP;            // window pixels held per image
  constexpr int NPW = 2 * PPI / 4;          // pieces per wave and row: 3 or 2
  constexpr int ROWB = 2 * WPX * PXB;       // one ring slot: both images' window of one input row
  constexpr int D = 3, R = D + 1;           // rows in flight ahead of the one being read; ring slots
  extern __shared__ __attribute__((aligned(16))) char smem_w[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware decode of the linear workgroup id -> (column group, row strip, image pair)
  int id = blockIdx.x;
  {
    const int nb = gridDim.x, qq = nb >> 3, rr8 = nb & 7, xcd = id & 7, local = id >> 3;
    id = (xcd < rr8 ? xcd * (qq + 1) : rr8 * (qq + 1) + (xcd - rr8) * qq) + local;
  }
  const int bx = id % nbx, by = (id / nbx) % nby, b = id / (nbx * nby);
  const int xi = GRP ? b / K : b;
  const bool lead = !GRP || b - xi * K == 0;
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  const int ox0 = bx * 4, ox = ox0 + wave;
  const bool live_col = ox < Wo;            // a dead column computes on clamped pixels and stores nothing
  // a block walks a strip of `strip` output rows (the launcher's choice): the 20 rows of vertical run-in are
  // paid once per strip, so tall strips where the grid stays large enough (64-row strips: 31 % more input rows)
  const int oy0 = by * strip;
  const int nout = min(strip, Ho - oy0);
  const int nrows = nout + kWin - 1;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  const unsigned img_bytes = (unsigned)H * (unsigned)W * (unsigned)C * (unsigned)SZ;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<T *>(fx + (size_t)xi * H * W * C), 0, img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<T *>(fy + (size_t)b * H * W * C), 0, img_bytes, 0x00020000);
  // this wave's DMA pieces: piece p = i*4 + wave covers pixels [pidx*PPP, +PPP) of image p / PPI
  unsigned voff[NPW];  // per-lane source offset of piece i at row 0 of the strip, channel block 0
  int pdst[NPW], pimg[NPW];
#pragma unroll
  for (int i = 0; i < NPW; ++i) {
    const int pc = i * 4 + wave;
    pimg[i] = pc / PPI;
    const int pidx = pc - pimg[i] * PPI;
    pdst[i] = pimg[i] * (WPX * PXB) + pidx * 1024;
    const int px = min(ox0 + pidx * PPP + lane / (64 / PPP), W - 1);
    voff[i] = (unsigned)(((oy0 * W + px) * C) * SZ + (lane % (64 / PPP)) * 16);
  }
  const unsigned row_stride = (unsigned)W * (unsigned)C * (unsigned)SZ;
  const int rd_base = wave * PXB + lane * SZ;  // this lane's tap 0 of image x inside a slot
  float acc_g = 0.f, acc_t = 0.f, acc_s = 0.f;  // lane l: output row oy0 + 64 k + l of the current 64-row group k
  // (Moving two of these accumulators to LDS for C > 64 was tried to spare registers: it takes the block's LDS past a
  // third of the CU's -- 2 blocks per CU instead of 3 -- see profiles/r03_window_ab.txt.)
  for (int cb = 0; cb < C; cb += 64) {
    const int c = cb + lane;
    // a finished group of (up to) 64 output rows leaves the lanes: stored by the first channel block, added to
    // by the later ones (same lane, same address, program order), the last one scales gamma by 1/C
    auto flush = [&](int orow) {
      const int r = (orow & ~63) + lane;
      if (live_col && r <= orow) {
        const size_t o = ((size_t)b * Ho + oy0 + r) * Wo + ox;
        const size_t og = GRP ? ((size_t)xi * Ho + oy0 + r) * Wo + ox : o;
        float fg = acc_g, ft = acc_t, fs = acc_s;
        if (cb > 0) {
          if (lead) fg += gamma[og];
          ft += tw[o];
          fs += sw[o];
        }
        if (lead) gamma[og] = cb + 64 >= C ? fg / (float)C : fg;
        tw[o] = ft;
        sw[o] = fs;
      }
      acc_g = acc_t = acc_s = 0.f;
    };
    // the channel's three constants live in LDS (re-read per output row at immediate offsets): with them in
    // registers the C > 64 instances need 172 VGPRs, four past the three-waves-per-SIMD limit
    float *const chan = reinterpret_cast<float *>(smem_w + R * ROWB) + wave * 192 + lane;
    chan[0] = q[0 * st + qo + c];
    chan[64] = q[1 * st + qo + c];
    chan[128] = wgt[(size_t)xi * ctot + coff + c];
    auto issue_row = [&](int r) {
      char *slot = smem_w + (r % R) * ROWB;
#pragma unroll
      for (int i = 0; i < NPW; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(pimg[i] ? ry : rx, (lds_void_t *)(slot + pdst[i]), 16,
                                                 voff[i] + (unsigned)(cb * SZ), (unsigned)r * row_stride, 0, 0);
    };
    // every wave has finished reading the previous channel block's last rows before their slots are refilled
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int r = 0; r < D; ++r)
      if (r < nrows) issue_row(r);
    WinRing rg;
#pragma unroll
    for (int u = 0; u < kWin; ++u) rg.s0[u] = rg.s1[u] = rg.s2[u] = rg.s3[u] = rg.s4[u] = 0.f;
    // 21 rows per trip, the row body instantiated once per ring slot: every slot index and every vertical tap
    // weight is a compile-time constant
#define NQA_WIN_ROW(SLOT)                                                                                          \
  {                                                                                                                \
    const int rr = rr0 + SLOT;                                                                                     \
    if (rr < nrows) {                                                                                              \
      /* row rr has landed (this wave's pieces: all but the D-1 younger rows'; everyone's: the barrier), and */   \
      /* every wave is done with row rr-1, whose slot row rr+D now takes */                                        \
      if (rr + D <= nrows)                                                                                         \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((D - 1) * NPW) : "memory");               \
      else                                                                                                         \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");                                   \
      if (rr + D < nrows) issue_row(rr + D);                                                                       \
      const char *slot = smem_w + (rr % R) * ROWB + rd_base;                                                       \
      float xr[kWin], yr[kWin];                                                                                    \
      _Pragma("unroll") for (int j = 0; j < kWin; ++j) {                                                           \
        xr[j] = P::to_f(*reinterpret_cast<const T *>(slot + j * PXB));                                             \
        yr[j] = P::to_f(*reinterpret_cast<const T *>(slot + WPX * PXB + j * PXB));                                 \
      }                                                                                                            \
      float gterm = 0.f, tt = 0.f, ss = 0.f;                                                                       \
      const bool full = rr >= kWin - 1;                                                                            \
      win_row<SLOT>(xr, yr, rg, full, chan[0], chan[64], chan[128], gterm, tt, ss);                                \
      if (full) {                                                                                                  \
        float gs = gterm, ts = tt, sss = ss;                                                                       \
        wave_sum3(gs, ts, sss);                                                                                    \
        const int orow = rr - (kWin - 1);                                                                          \
        if (lane == (orow & 63)) {                                                                                 \
          acc_g += gs;                                                                                             \
          acc_t += ts;                                                                                             \
          acc_s += sss;                                                                                            \
        }                                                                                                          \
        if ((orow & 63) == 63 || orow == nout - 1) flush(orow);                                                    \
      }                                                                                                            \
    }                                                                                                              \
  }
    for (int rr0 = 0; rr0 < nrows; rr0 += kWin) {
      NQA_WIN_ROW(0) NQA_WIN_ROW(1) NQA_WIN_ROW(2) NQA_WIN_ROW(3) NQA_WIN_ROW(4) NQA_WIN_ROW(5) NQA_WIN_ROW(6)
      NQA_WIN_ROW(7) NQA_WIN_ROW(8) NQA_WIN_ROW(9) NQA_WIN_ROW(10) NQA_WIN_ROW(11) NQA_WIN_ROW(12) NQA_WIN_ROW(13)
      NQA_WIN_ROW(14) NQA_WIN_ROW(15) NQA_WIN_ROW(16) NQA_WIN_ROW(17) NQA_WIN_ROW(18) NQA_WIN_ROW(19) NQA_WIN_ROW(20)
    }
#undef NQA_WIN_ROW
  }
#endif
}

template <typename P, int C>
__global__ __launch_bounds__(256, 3) void adists_window_lds_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, Gauss gw,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int nbx, int nby, int strip) {
  window_lds_body<P, C, false>(fx, fy, H, W, q, B, ctot, coff, wgt, gw, gamma, tw, sw, nbx, nby, strip, 1);
}
template <typename P, int C>
__global__ __launch_bounds__(256, 3) void adists_window_lds_group_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, Gauss gw,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int nbx, int nby, int strip, int K) {
  window_lds_body<P, C, true>(fx, fy, H, W, q, B, ctot, coff, wgt, gw, gamma, tw, sw, nbx, nby, strip, K);
}

// The windowed pass of stage 0 (the raw image: 3 float planes, NCHW) in the same shape as the lanes
// kernel above, with lanes = 64 adjacent output COLUMNS of one plane: every tap load is a coalesced
// row segment at an immediate offset from one row pointer, the ring and the packed tap arithmetic
// are identical, nothing is reduced across lanes, and the three channels are accumulated into the
// maps one after the other by the same lane (plain read-modify-write, no atomics).
template <bool GRP>  // (GRP: the group form, see adists_window_lanes_kernel)
__device__ __forceinline__ void window_planar_body(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, Gauss gw, float *__restrict__ gamma, float *__restrict__ tw,
    float *__restrict__ sw, int K) {
  (void)gw;  // taps = the compile-time constants kG
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z;
  const int xi = GRP ? b / K : b;
  const bool lead = !GRP || b - xi * K == 0;
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  const int ox0 = blockIdx.x * 256 + wave * 64;
  if (ox0 >= Wo) return;
  const int ox = ox0 + lane;
  const bool live = ox < Wo;
  const int oxc = live ? ox : Wo - 1;  // dead lanes re-read the last column and store nothing
  const int oy0 = blockIdx.y * 64;
  const int nout = min(64, Ho - oy0);
  const int nrows = nout + kWin - 1;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  const size_t o0 = ((size_t)b * Ho + oy0) * Wo + ox;
  // the group form reaches gamma through a column pointer of its own (reference xi's map); with the pairwise form's
  // `gamma[o]` it needs 185 VGPRs, with this one 168: three waves per SIMD like the pairwise kernel, and no scratch
  float *const gq = gamma + ((size_t)xi * Ho + oy0) * Wo + ox;
  for (int c = 0; c < 3; ++c) {
    const float ix = q[0 * st + qo + c], iy = q[1 * st + qo + c], wc = wgt[(size_t)xi * ctot + coff + c];
    const float *px = x + ((size_t)(xi * 3 + c) * H + oy0) * W + oxc;
    const float *py = y + ((size_t)(b * 3 + c) * H + oy0) * W + oxc;
    WinRing rg;
#pragma unroll
    for (int u = 0; u < kWin; ++u) rg.s0[u] = rg.s1[u] = rg.s2[u] = rg.s3[u] = rg.s4[u] = 0.f;
#define NQA_PLANAR_ROW(SLOT)                                                          \
  {                                                                                   \
    const int rr = rr0 + SLOT;                                                        \
    if (rr < nrows) {                                                                 \
      float xr[kWin], yr[kWin];                                                       \
      _Pragma("unroll") for (int j = 0; j < kWin; ++j) {                              \
        xr[j] = px[j];                                                                \
        yr[j] = py[j];                                                                \
      }                                                                               \
      px += W;                                                                        \
      py += W;                                                                        \
      float gterm = 0.f, tt = 0.f, ss = 0.f;                                          \
      const bool full = rr >= kWin - 1;                                               \
      win_row<SLOT>(xr, yr, rg, full, ix, iy, wc, gterm, tt, ss);                     \
      if (full && live) {                                                             \
        const size_t o = o0 + (size_t)(rr - (kWin - 1)) * Wo;                         \
        if constexpr (GRP) {                                                          \
          if (lead) {                                                                 \
            float *const gp = gq + (size_t)(rr - (kWin - 1)) * Wo;                    \
            const float gsum = c == 0 ? gterm : *gp + gterm;                          \
            *gp = c == 2 ? gsum / 3.f : gsum;                                         \
          }                                                                           \
        }                                                                             \
        if (c == 0) {                                                                 \
          if constexpr (!GRP) gamma[o] = gterm;                                       \
          tw[o] = tt;                                                                 \
          sw[o] = ss;                                                                 \
        } else {                                                                      \
          if constexpr (!GRP) {                                                       \
            const float gsum = gamma[o] + gterm;                                      \
            gamma[o] = c == 2 ? gsum / 3.f : gsum;                                    \
          }                                                                           \
          tw[o] += tt;                                                                \
          sw[o] += ss;                                                                \
        }                                                                             \
      }                                                                               \
    }                                                                                 \
  }
    for (int rr0 = 0; rr0 < nrows; rr0 += kWin) {
      NQA_PLANAR_ROW(0) NQA_PLANAR_ROW(1) NQA_PLANAR_ROW(2) NQA_PLANAR_ROW(3) NQA_PLANAR_ROW(4) NQA_PLANAR_ROW(5)
      NQA_PLANAR_ROW(6) NQA_PLANAR_ROW(7) NQA_PLANAR_ROW(8) NQA_PLANAR_ROW(9) NQA_PLANAR_ROW(10) NQA_PLANAR_ROW(11)
      NQA_PLANAR_ROW(12) NQA_PLANAR_ROW(13) NQA_PLANAR_ROW(14) NQA_PLANAR_ROW(15) NQA_PLANAR_ROW(16) NQA_PLANAR_ROW(17)
      NQA_PLANAR_ROW(18) NQA_PLANAR_ROW(19) NQA_PLANAR_ROW(20)
    }
#undef NQA_PLANAR_ROW
  }
}

__global__ __launch_bounds__(256, 2) void adists_window_planar_kernel(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, Gauss gw, float *__restrict__ gamma, float *__restrict__ tw,
    float *__restrict__ sw) {
  window_planar_body<false>(x, y, H, W, q, B, ctot, coff, wgt, gw, gamma, tw, sw, 1);
}
__global__ __launch_bounds__(256, 3) void adists_window_planar_group_kernel(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, Gauss gw, float *__restrict__ gamma, float *__restrict__ tw,
    float *__restrict__ sw, int K) {
  window_planar_body<true>(x, y, H, W, q, B, ctot, coff, wgt, gw, gamma, tw, sw, K);
}

// Global branch of one stage (maps smaller than the window; ADISTS.py:91-97,176-180): one
// block per image pair, from the per-channel global statistics.  Outputs 1x1 "maps".
template <bool GRP>  // (GRP: the group form, see adists_window_lanes_kernel)
__device__ __forceinline__ void global_body(const float *__restrict__ q, int B, int ctot, int coff, int creal,
                                            const float *__restrict__ wgt, float *__restrict__ gamma,
                                            float *__restrict__ tw, float *__restrict__ sw, int K) {
  __shared__ double red[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int xi = GRP ? b / K : b;
  const bool lead = !GRP || b - xi * K == 0;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  double g = 0, t = 0, s = 0;
  for (int c = tid; c < creal; c += 256) {
    const float ix = q[0 * st + qo + c], iy = q[1 * st + qo + c], w = wgt[(size_t)xi * ctot + coff + c];
    const float rmx = q[3 * st + qo + c], rmy = q[4 * st + qo + c];
    const float rvx = q[5 * st + qo + c], rvy = q[6 * st + qo + c], rcov = q[7 * st + qo + c];
    g += (double)(rvx / (rmx + 1e-12f));
    const float mx = ix * rmx, my = iy * rmy;
    const float vx = ix * ix * rvx, vy = iy * iy * rvy, cov = ix * iy * rcov;
    t += (double)(w * ((2.f * mx * my + 1e-6f) / (mx * mx + my * my + 1e-6f)));
    s += (double)(w * ((2.f * cov + 1e-6f) / (vx + vy + 1e-6f)));
  }
  red[0][tid] = g;
  red[1][tid] = t;
  red[2][tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off)
      for (int j = 0; j < 3; ++j) red[j][tid] += red[j][tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    if (lead) gamma[xi] = (float)(red[0][0] / creal);
    tw[b] = (float)red[1][0];
    sw[b] = (float)red[2][0];
  }
}

__global__ __launch_bounds__(256) void adists_global_kernel(const float *__restrict__ q, int B, int ctot, int coff,
                                                            int creal, const float *__restrict__ wgt,
                                                            float *__restrict__ gamma, float *__restrict__ tw,
                                                            float *__restrict__ sw) {
  global_body<false>(q, B, ctot, coff, creal, wgt, gamma, tw, sw, 1);
}
__global__ __launch_bounds__(256) void adists_global_group_kernel(const float *__restrict__ q, int B, int ctot, int coff,
                                                                  int creal, const float *__restrict__ wgt,
                                                                  float *__restrict__ gamma, float *__restrict__ tw,
                                                                  float *__restrict__ sw, int K) {
  global_body<true>(q, B, ctot, coff, creal, wgt, gamma, tw, sw, K);
}

// The same pass for a run-time window size (3..63): ring in LDS, taps from a table.  Every window but 21 runs on these.
#include "nqa_window_n.h"

// ---------------------------------------------------------------------------------
// Probability chain on the small maps (compute_prob, ADISTS.py:77-99) and the stage's D.
struct ChainAcc {       // one per (stage, image); zeroed before the chain
  double sum, sumsq;    // of gamma
  unsigned ps_min, ps_max, pp_min, pp_max;  // float bit patterns (values >= 0)
  double dsum;          // sum over the map of (1-ps) TW + ps SW
};

__device__ inline float sigmoid_ref(float z) { return 1.f / (1.f + expf(-z)); }

__device__ inline void zscore(const ChainAcc &a, int n, float &mean, float &sd) {
  const double m = a.sum / n;
  mean = (float)m;
  double v = (a.sumsq - n * m * m) / (double)(n - 1);  // unbiased; n==1 -> 0/0 = NaN as torch.std
  if (v < 0.0) v = 0.0;                                  // rounding of a constant map (NaN stays NaN)
  sd = (float)sqrt(v);
}

__global__ __launch_bounds__(256) void chain_init_kernel(ChainAcc *acc, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    acc[i].sum = acc[i].sumsq = acc[i].dsum = 0.0;
    acc[i].ps_min = acc[i].pp_min = 0x7F800000u;  // +inf
    acc[i].ps_max = acc[i].pp_max = 0u;
  }
}

// Cross-block sums of the chain (gamma moments, the stage's D) are NOT accumulated with fp64 atomics: their
// arrival order would make the last bits of a score differ from run to run.  Each block stores its partial
// in a slot of its own and chain_fold_kernel adds the slots in a fixed order (min / max stay atomic: exact).
__global__ __launch_bounds__(256) void chain_fold_kernel(const double *__restrict__ cp, int G, int nvals, int which,
                                                         ChainAcc *acc) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int v = 0; v < nvals; ++v) {
    double s = 0.0;
    for (int g = tid; g < G; g += 256) s += cp[((size_t)b * G + g) * nvals + v];
    __syncthreads();
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      if (which == 1) acc[b].dsum = red[0];
      else if (v == 0) acc[b].sum = red[0];
      else acc[b].sumsq = red[0];
    }
  }
}

__global__ __launch_bounds__(256) void chain_moments_kernel(const float *__restrict__ gamma, int n,
                                                            double *__restrict__ cp /* [B][gridDim.x][2] */) {
  __shared__ double red[2][256];
  const int b = blockIdx.y, tid = threadIdx.x;
  double s = 0, s2 = 0;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
    const double g = gamma[(size_t)b * n + i];
    s += g;
    s2 += g * g;
  }
  red[0][tid] = s;
  red[1][tid] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    cp[((size_t)b * gridDim.x + blockIdx.x) * 2 + 0] = red[0][0];
    cp[((size_t)b * gridDim.x + blockIdx.x) * 2 + 1] = red[1][0];
  }
}

__device__ inline void block_minmax(float lo, float hi, unsigned *gmin, unsigned *gmax) {
  __shared__ float rl[256], rh[256];
  const int tid = threadIdx.x;
  rl[tid] = lo;
  rh[tid] = hi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      rl[tid] = fminf(rl[tid], rl[tid + off]);
      rh[tid] = fmaxf(rh[tid], rh[tid + off]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    atomicMin(gmin, __float_as_uint(rl[0]));
    atomicMax(gmax, __float_as_uint(rh[0]));
  }
}

__global__ __launch_bounds__(256) void chain_psminmax_kernel(const float *__restrict__ gamma, int n, ChainAcc *acc) {
  const int b = blockIdx.y;
  float mean, sd;
  zscore(acc[b], n, mean, sd);
  float lo = INFINITY, hi = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float ps = sigmoid_ref((gamma[(size_t)b * n + i] - mean) / (sd + 1e-12f));
    lo = fminf(lo, ps);
    hi = fmaxf(hi, ps);
  }
  block_minmax(lo, hi, &acc[b].ps_min, &acc[b].ps_max);
}

// bilinear sample of prev (hp x wp) at output (y,x) of an (h x w) grid, align_corners=True
__device__ inline float bilinear_ac(const float *__restrict__ prev, int hp, int wp, int h, int w, int y, int x) {
  const float sy = h > 1 ? (float)(hp - 1) / (float)(h - 1) : 0.f;
  const float sx = w > 1 ? (float)(wp - 1) / (float)(w - 1) : 0.f;
  const float ry = sy * y, rx = sx * x;
  const int y0 = (int)ry, x0 = (int)rx;
  const int y1 = y0 + (y0 < hp - 1 ? 1 : 0), x1 = x0 + (x0 < wp - 1 ? 1 : 0);
  const float ly = ry - y0, lx = rx - x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  return hy * (hx * prev[y0 * wp + x0] + lx * prev[y0 * wp + x1]) +
         ly * (hx * prev[y1 * wp + x0] + lx * prev[y1 * wp + x1]);
}

__device__ inline float pp_value(const float *gamma, const ChainAcc &a, int n, const float *prev, int hp, int wp,
                                 int h, int w, int i, float mean, float sd) {
  const float ps = sigmoid_ref((gamma[i] - mean) / (sd + 1e-12f));
  const float lo = __uint_as_float(a.ps_min), hi = __uint_as_float(a.ps_max);
  const float psn = (ps - lo) / (hi - lo + 1e-12f);
  return psn * bilinear_ac(prev, hp, wp, h, w, i / w, i % w);
}

__global__ __launch_bounds__(256) void chain_ppminmax_kernel(const float *__restrict__ gamma, int h, int w,
                                                             const float *__restrict__ prev, int hp, int wp,
                                                             ChainAcc *acc) {
  const int b = blockIdx.y, n = h * w;
  float mean, sd;
  zscore(acc[b], n, mean, sd);
  float lo = INFINITY, hi = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float pp = pp_value(gamma + (size_t)b * n, acc[b], n, prev + (size_t)b * hp * wp, hp, wp, h, w, i, mean, sd);
    lo = fminf(lo, pp);
    hi = fmaxf(hi, pp);
  }
  block_minmax(lo, hi, &acc[b].pp_min, &acc[b].pp_max);
}

__global__ __launch_bounds__(256) void chain_final_kernel(const float *__restrict__ gamma, int h, int w,
                                                          const float *__restrict__ prev, int hp, int wp,
                                                          const float *__restrict__ tw, const float *__restrict__ sw,
                                                          float *__restrict__ psprod, const ChainAcc *acc,
                                                          double *__restrict__ cp /* [B][gridDim.x] */) {
  __shared__ double red[256];
  const int b = blockIdx.y, n = h * w, tid = threadIdx.x;
  float mean, sd;
  zscore(acc[b], n, mean, sd);
  const float lo = __uint_as_float(acc[b].pp_min), hi = __uint_as_float(acc[b].pp_max);
  double d = 0.0;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
    const float pp = pp_value(gamma + (size_t)b * n, acc[b], n, prev + (size_t)b * hp * wp, hp, wp, h, w, i, mean, sd);
    const float ps = (pp - lo) / (hi - lo + 1e-12f);
    psprod[(size_t)b * n + i] = ps;
    d += (double)((1.f - ps) * tw[(size_t)b * n + i] + ps * sw[(size_t)b * n + i]);
  }
  red[tid] = d;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) cp[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

// global-branch stage: ps = sigmoid(gamma); ps_prod = ps * prev[0,0]; D = (1-ps_prod) TW + ps_prod SW
__global__ void chain_global_kernel(const float *__restrict__ gamma, const float *__restrict__ prev, int hpwp,
                                    const float *__restrict__ tw, const float *__restrict__ sw,
                                    float *__restrict__ psprod, ChainAcc *acc, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float ps = sigmoid_ref(gamma[b]) * prev[(size_t)b * hpwp];
  psprod[b] = ps;
  acc[b].dsum = (double)((1.f - ps) * tw[b] + ps * sw[b]);
}

// The group forms of the two kernels above (nqa_adists_forward_group): gamma, prev, psprod and `acc` are per REFERENCE
// (blockIdx.y = r), tw / sw and the D partials per pair r * K + k.  An element's ps_prod is computed and stored once;
// the K renders' sums are then taken against the stored values, each in chain_final_kernel's grid-stride order and with
// its block reduction, so a pair's partial is the pairwise kernel's bit for bit.  For that the element's term is written
// with explicit roundings, in the form hipcc contracts the pairwise kernels' `(1 - ps) * tw + ps * sw` to (ISA read:
// chain_final_kernel tw * (1 - ps), then one fma with sw * ps; chain_global_kernel the same with 1 - ps itself
// contracted to fma(-prev, sigmoid, 1)) -- left to the compiler the group kernels took the other product first and a
// pair's D could differ in its last bit.  tests/test_gpu_adists_group_stage.py holds the two forms together.
__global__ __launch_bounds__(256) void chain_final_group_kernel(const float *__restrict__ gamma, int h, int w,
                                                                const float *__restrict__ prev, int hp, int wp,
                                                                const float *__restrict__ tw, const float *__restrict__ sw,
                                                                float *psprod, const ChainAcc *acc, int K,
                                                                double *__restrict__ cp /* [R * K][gridDim.x] */) {
  __shared__ double red[256];
  const int r = blockIdx.y, n = h * w, tid = threadIdx.x;
  float mean, sd;
  zscore(acc[r], n, mean, sd);
  const float lo = __uint_as_float(acc[r].pp_min), hi = __uint_as_float(acc[r].pp_max);
  float *ps_r = psprod + (size_t)r * n;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
    const float pp = pp_value(gamma + (size_t)r * n, acc[r], n, prev + (size_t)r * hp * wp, hp, wp, h, w, i, mean, sd);
    ps_r[i] = (pp - lo) / (hi - lo + 1e-12f);
  }
  for (int k = 0; k < K; ++k) {
    const size_t b = (size_t)r * K + k;
    double d = 0.0;
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
      const float ps = ps_r[i];  // this thread's own store above
      d += (double)fmaf(sw[b * n + i], ps, __fmul_rn(tw[b * n + i], 1.f - ps));
    }
    __syncthreads();
    red[tid] = d;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) cp[b * gridDim.x + blockIdx.x] = red[0];
  }
}

// one thread per pair; gamma, prev, psprod per reference, `acc` (the D sums) per pair
__global__ void chain_global_group_kernel(const float *__restrict__ gamma, const float *__restrict__ prev, int hpwp,
                                          const float *__restrict__ tw, const float *__restrict__ sw,
                                          float *__restrict__ psprod, ChainAcc *acc, int B, int K) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int r = b / K;
  const float sg = sigmoid_ref(gamma[r]), pv = prev[(size_t)r * hpwp];
  const float ps = __fmul_rn(pv, sg);
  if (b - r * K == 0) psprod[r] = ps;
  acc[b].dsum = (double)fmaf(ps, sw[b], __fmul_rn(tw[b], fmaf(-pv, sg, 1.f)));
}

__global__ void ones_kernel(float *p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.f;
}

// D_b = sum_k dsum_k / n_k
struct DDesc {
  int n[NQA_NUM_TAPS];
};
__global__ void adists_d_kernel(const ChainAcc *acc, DDesc d, int B, float *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int k = NQA_NUM_TAPS - 1; k >= 0; --k) s += (float)(acc[(size_t)k * B + b].dsum / d.n[k]);
  out[b] = s;
}

// as_map=True (ADISTS.py:163,188-189,193): 1 - sum over stages (coarse to fine, the reference's loop
// order) of the stage's D map bilinearly resized to (H, W), align_corners=False.  The stage map is
// rebuilt from the chain's ps_prod and the window pass' TW / SW maps.
struct MapDesc {
  const float *ps[NQA_NUM_TAPS], *tw[NQA_NUM_TAPS], *sw[NQA_NUM_TAPS];
  int mh[NQA_NUM_TAPS], mw[NQA_NUM_TAPS];
};
__device__ inline void src_index(int dst, int in, int out, int &i0, int &i1, float &l0, float &l1) {
  // torch upsample_bilinear2d, align_corners=False: src = in/out * (dst + 0.5) - 0.5, clamped at 0
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}
__global__ __launch_bounds__(256) void adists_map_kernel(MapDesc d, int H, int W, float *__restrict__ out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  float s = 0.f;
  for (int k = NQA_NUM_TAPS - 1; k >= 0; --k) {
    const int mh = d.mh[k], mw = d.mw[k];
    const size_t o = (size_t)b * mh * mw;
    const float *ps = d.ps[k] + o, *tw = d.tw[k] + o, *sw = d.sw[k] + o;
    auto dm = [&](int yy, int xx) {
      const int j = yy * mw + xx;
      const float p = ps[j];
      return (1.f - p) * tw[j] + p * sw[j];
    };
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(y, mh, H, y0, y1, ly0, ly1);
    src_index(x, mw, W, x0, x1, lx0, lx1);
    s = s + (ly0 * (lx0 * dm(y0, x0) + lx1 * dm(y0, x1)) + ly1 * (lx0 * dm(y1, x0) + lx1 * dm(y1, x1)));
  }
  out[(size_t)b * H * W + i] = 1.f - s;
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
static Gauss make_gauss() {
  // gaussian(21, 7): exp(-(x-10)^2 / (2*7^2)) in double, stored as float, normalised in float
  // (ADISTS.py:102-104 builds a float32 tensor and divides by its float32 sum)
  Gauss g;
  float s = 0.f;
  float v[kWin];
  for (int i = 0; i < kWin; ++i) v[i] = (float)exp(-(double)((i - 10) * (i - 10)) / (2.0 * 7.0 * 7.0));
  // torch.sum of 21 floats: sequential order is within 1 ulp of any other; use double then round
  double sd = 0.0;
  for (int i = 0; i < kWin; ++i) sd += (double)v[i];
  s = (float)sd;
  for (int i = 0; i < kWin; ++i) g.g[i] = v[i] / s;
  return g;
}

// gaussian(n, n / 3) for every n the generic kernels take, by make_gauss's arithmetic: the centre is n / 2 (integer),
// so an even window is not symmetric (ADISTS.py:102-104); sigma = n / 3 and 2 sigma^2 are Python's doubles.
static const GaussN &gauss_n(int n) {
  struct Table {
    GaussN t[kWinMax + 1];
    Table() {
      memset(t, 0, sizeof(t));
      for (int n = kWinMin; n <= kWinMax; ++n) {
        const double sigma = (double)n / 3.0;
        float v[kWinMax];
        double sd = 0.0;
        for (int i = 0; i < n; ++i) {
          v[i] = (float)exp(-(double)((i - n / 2) * (i - n / 2)) / (2.0 * (sigma * sigma)));
          sd += (double)v[i];
        }
        const float s = (float)sd;
        for (int i = 0; i < n; ++i) t[n].g[i] = v[i] / s;
      }
    }
  };
  static const Table table;
  return table.t[n];
}

// NQA_OK for a window the library takes, else the argument error naming the range under the caller's name.
static int window_check(const char *who, int window) {
  if (window < kWinMin || window > kWinMax) {
    set_error("%s: window %d outside [%d, %d]", who, window, kWinMin, kWinMax);
    return NQA_E_ARG;
  }
  return NQA_OK;
}

// the same table and the same check for the generic window-moments kernels (nqa_window_moments_n.hip)
const float *window_taps_n(int n) { return gauss_n(n).g; }
int window_check_n(const char *who, int window) { return window_check(who, window); }

// Every host function below describes a call by three integers: X x-side images, B pairs, and K -- 0 for B independent
// pairs (X = B, pair b reads x image b), > 0 for groups of K renders per reference (B = X * K, pair b reads x image
// b / K).  What A-DISTS takes from x alone (entropy weights, gamma, the probability chain) is sized and launched by X,
// what it takes from a pair (q, tw, sw, the D sums) by B.
static const long kAdistsGroupMaxPairs = 65535;  // pairs ride a grid's y / z dimension (adists_prep_kernel, finalize)

struct APlan {
  // byte offsets into the workspace.  hsum, acc_pair and ones are areas of their own for groups; for pairs they alias
  // q's row 2 (dead once the entropy passes have read sum_x), acc_x and bufB (the ping-pong buffers are free by then)
  size_t bufA, bufB, taps[5], img4x, part, q, ent, hsum, wgt, maps[NQA_NUM_TAPS][4], acc_x, acc_pair, chain_part, ones,
      total;
  StageDesc sd;  // statistics partials of the B pairs in finalize's layout
  EntDesc ed;    // entropy partials of the X x images
  int h[NQA_NUM_TAPS], w[NQA_NUM_TAPS], c[NQA_NUM_TAPS];  // feature dims per tap (k=0 raw image)
  int mh[NQA_NUM_TAPS], mw[NQA_NUM_TAPS];                  // map dims (1x1 for the global branch)
  bool windowed[NQA_NUM_TAPS];
  int ent_ppb[NQA_NUM_TAPS];
  int win;  // the window size the maps are sized for
};

// Feature dims of the six taps of an H x W frame (k = 0 the image, k = 1 relu1_2 at full size, then halved, rounding up),
// and the dims of a stage's gamma / TW / SW / ps_prod maps: valid win x win windows, or 1 x 1 from the global branch.
static void tap_dims(int H, int W, int h[NQA_NUM_TAPS], int w[NQA_NUM_TAPS]) {
  h[0] = h[1] = H;
  w[0] = w[1] = W;
  for (int k = 2; k < NQA_NUM_TAPS; ++k) {
    h[k] = (h[k - 1] + 1) / 2;
    w[k] = (w[k - 1] + 1) / 2;
  }
}
static void map_dims(const int h[NQA_NUM_TAPS], const int w[NQA_NUM_TAPS], int win, int mh[NQA_NUM_TAPS],
                     int mw[NQA_NUM_TAPS], bool windowed[NQA_NUM_TAPS]) {
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    windowed[k] = h[k] >= win && w[k] >= win;
    mh[k] = windowed[k] ? h[k] - (win - 1) : 1;
    mw[k] = windowed[k] ? w[k] - (win - 1) : 1;
  }
}

// The descriptors of the front part (statistics partials, entropy partials) for six taps of h[k] x w[k] x c[k]; doff and
// eoff receive the doubles the two partial arrays hold.  make_plan and nqa_adists_front both size and launch by this.
static void front_descs(int X, int B, int K, const int h[NQA_NUM_TAPS], const int w[NQA_NUM_TAPS],
                        const int c[NQA_NUM_TAPS], int prec, StageDesc &sd, EntDesc &ed, int ent_ppb[NQA_NUM_TAPS],
                        long &doff, long &eoff) {
  // statistics partials of the B pairs: stage 0 from the plane kernel; stages 1..5 from the NHWC group kernel, or
  // for pairs from the fused pool pass (taps 1..4, items = pooled pixels) and the NHWC kernel (tap 5)
  doff = 0;
  int coff = 0;
  for (int k = 0; k < 6; ++k) {
    const int hw = h[k] * w[k];
    int nblk;
    if (k == 0)
      nblk = cdiv(hw, stats_nchw_ppb(hw));
    else if (K > 0)
      nblk = cdiv(hw, group_stats_units_per_block(hw, c[k], prec, X));
    else if (k <= 4)
      nblk = pool_stats_tiles((h[k] + 1) / 2, (w[k] + 1) / 2, c[k], prec, B, nullptr, nullptr);
    else
      nblk = cdiv(hw, stats_units_per_block(hw, c[k], prec, B));
    sd.part_off[k] = doff;
    sd.nblk[k] = nblk;
    sd.hw[k] = hw;
    sd.c[k] = c[k];
    sd.coff[k] = coff;
    doff += (long)B * sd.nblk[k] * c[k] * 5;
    coff += c[k];
  }
  sd.nstage = 6;
  sd.ctot = coff;
  // entropy partials of the X x images
  eoff = 0;
  for (int k = 0; k < 6; ++k) {
    const int hw = h[k] * w[k];
    const int cpad = k == 0 ? 4 : c[k];
    const int ppb = stats_units_per_block(hw, cpad, k == 0 ? NQA_PREC_F32 : prec, X);
    ent_ppb[k] = ppb;
    ed.part_off[k] = eoff;
    ed.nblk[k] = cdiv(hw, ppb);
    ed.c[k] = cpad;
    ed.creal[k] = c[k];
    ed.coff[k] = sd.coff[k];
    eoff += (long)X * ed.nblk[k] * cpad;
  }
  ed.ctot = coff;
}

// The chain's cross-block partials: two moments per x image, then one D sum per pair, in the same area.
static size_t chain_part_bytes(int X, int B) {
  return (size_t)(2 * X > B ? 2 * X : B) * kChainBlocks * sizeof(double);
}

// One NHWC batch of n = X + B images (the x images first), all five taps kept.
static APlan make_plan(int X, int B, int K, int H, int W, int prec, int win) {
  APlan p;
  memset(&p, 0, sizeof(p));
  const size_t esz = prec_elem_bytes(prec);
  const int n = X + B;
  tap_dims(H, W, p.h, p.w);
  for (int k = 0; k < NQA_NUM_TAPS; ++k) p.c[k] = kChns[k];
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += align_up(bytes, 256);
    return o;
  };
  const size_t act = (size_t)n * max_act_elems(H, W) * esz;  // not H*W*64: tiny frames peak at a later stage
  p.bufA = take(act);
  p.bufB = take(act);
  for (int k = 0; k < 5; ++k) p.taps[k] = take((size_t)n * p.h[k + 1] * p.w[k + 1] * p.c[k + 1] * esz);
  p.img4x = take((size_t)X * H * W * 4 * 4);
  long doff, eoff;
  front_descs(X, B, K, p.h, p.w, p.c, prec, p.sd, p.ed, p.ent_ppb, doff, eoff);
  const int coff = p.sd.ctot;
  p.part = take((size_t)doff * 8);
  p.q = take((size_t)8 * B * coff * 4);
  p.ent = take((size_t)eoff * 8);
  p.hsum = K > 0 ? take((size_t)X * coff * 4) : p.q + (size_t)2 * B * coff * 4;
  p.wgt = take((size_t)X * coff * 4);
  p.win = win;
  map_dims(p.h, p.w, win, p.mh, p.mw, p.windowed);
  for (int k = 0; k < 6; ++k)
    for (int j = 0; j < 4; ++j)  // gamma and ps_prod per x image, tw and sw per pair
      p.maps[k][j] = take((size_t)(j == 0 || j == 3 ? X : B) * p.mh[k] * p.mw[k] * 4);
  p.acc_x = take((size_t)6 * X * sizeof(ChainAcc));
  p.acc_pair = K > 0 ? take((size_t)6 * B * sizeof(ChainAcc)) : p.acc_x;
  p.chain_part = take(chain_part_bytes(X, B));
  p.ones = K > 0 ? take((size_t)X * sizeof(float)) : p.bufB;
  p.total = off;
  return p;
}

template <typename P>
static int launch_entropy(const void *feat, int B, int HW, int C, int ppb, const float *invx, const float *sumx,
                          int ctot, double *part, hipStream_t st) {
  dim3 grid(cdiv(HW, ppb), B);
  TimedLaunch t(NQA_K_ADISTS, st);
  entropy_nhwc_kernel<P><<<grid, 256, 0, st>>>(reinterpret_cast<const typename P::T *>(feat), HW, C, ppb, invx, sumx,
                                               ctot, part);
  return check_launch("entropy");
}

// The window launchers below take K = 0 for B independent pairs (x and y hold B images each), or K > 0 for the group
// forms: B = R * K pairs, x holds the R references, wgt R rows, gamma R maps (adists_window_lanes_kernel).
static int launch_window_planar(const float *x, const float *y, int B, int H, int W, const float *q, int ctot, int coff,
                                const float *wgt, const Gauss &g, float *gamma, float *tw, float *sw, hipStream_t st,
                                int K = 0) {
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  dim3 grid(cdiv(Wo, 256), cdiv(Ho, 64), B);
  TimedLaunch t(NQA_K_ADISTS, st);
  if (K > 0)
    adists_window_planar_group_kernel<<<grid, 256, 0, st>>>(x, y, H, W, q, B, ctot, coff, wgt, g, gamma, tw, sw, K);
  else
    adists_window_planar_kernel<<<grid, 256, 0, st>>>(x, y, H, W, q, B, ctot, coff, wgt, g, gamma, tw, sw);
  return check_launch("adists_window_planar");
}

// Grid of the LDS form of the window pass: column groups of 4, and strips as tall as the grid allows (up to 256
// rows): the fewest strips that still give the chip ~8 rounds of blocks (3 blocks per CU), else 64-row strips.
// strip_req in [1, Ho] replaces that choice of height (nqa_adists_window_stage: tests reach the multi-group
// strips at small shapes with it); 0 is the launcher's own.
static void window_lds_grid(int Ho, int Wo, int B, int strip_req, int &nbx, int &nby, int &strip) {
  nbx = cdiv(Wo, 4);
  if (strip_req > 0) {
    strip = strip_req;
  } else {
    nby = cdiv(Ho, 256);
    while (nby < cdiv(Ho, 64) && (long)nbx * nby * B < 6144) ++nby;
    strip = cdiv(Ho, nby);
  }
  nby = cdiv(Ho, strip);
}

// Which form of the NHWC pass runs: the LDS kernel (instantiated for float taps only) unless the calling thread asked
// for the first form.  The launcher and nqa_adists_window_grid both decide by this.
static bool window_uses_lds(size_t tap_elem_bytes) { return tap_elem_bytes == 4 && !adists_window_legacy(); }

template <typename P>
static int launch_window_lanes(const void *fx, const void *fy, int B, int H, int W, int C, const float *q, int ctot,
                               int coff, const float *wgt, const Gauss &g, float *gamma, float *tw, float *sw,
                               hipStream_t st, int strip_req = 0, int K = 0) {
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  const typename P::T *px = reinterpret_cast<const typename P::T *>(fx), *py = reinterpret_cast<const typename P::T *>(fy);
  // the shipped form for float taps (f32 / f32s): taps shared through LDS, XCD-aware column order.  16-bit taps
  // (the opt-in f16 / bf16 modes) measured 20 % slower that way (2-byte LDS reads + conversions) and keep the first form
  if constexpr (sizeof(typename P::T) == 4) {  // (the LDS kernel is instantiated for float taps only)
  if (window_uses_lds(sizeof(typename P::T))) {
    // four ring slots + the waves' channel constants (3 x 64 floats each): 51 KB, three blocks per CU
    const int LDS = 4 * 2 * 24 * 64 * 4 + 4 * 768;
    int nbx, nby, strip;
    window_lds_grid(Ho, Wo, B, strip_req, nbx, nby, strip);
    const long nblk = (long)nbx * nby * B;
    if (nblk > 0x7FFFFFFFL) {
      set_error("adists_window: grid too large");
      return NQA_E_SHAPE;
    }
    TimedLaunch t(NQA_K_ADISTS, st);
#define NQA_WIN(CC)                                                                                                  \
  if (K > 0)                                                                                                         \
    adists_window_lds_group_kernel<P, CC><<<(unsigned)nblk, 256, LDS, st>>>(px, py, H, W, q, B, ctot, coff, wgt, g, \
                                                                            gamma, tw, sw, nbx, nby, strip, K);     \
  else                                                                                                               \
    adists_window_lds_kernel<P, CC><<<(unsigned)nblk, 256, LDS, st>>>(px, py, H, W, q, B, ctot, coff, wgt, g, gamma, \
                                                                      tw, sw, nbx, nby, strip)
    switch (C) {
      case 64: NQA_WIN(64); break;
      case 128: NQA_WIN(128); break;
      case 256: NQA_WIN(256); break;
      case 512: NQA_WIN(512); break;
      default: set_error("adists_window: unsupported channel count %d", C); return NQA_E_SHAPE;
    }
#undef NQA_WIN
    return check_launch("adists_window_lds");
  }
  }
  dim3 grid(cdiv(Wo, 4), cdiv(Ho, 64), B);
  TimedLaunch t(NQA_K_ADISTS, st);
#define NQA_LANES(CC)                                                                                                   \
  if (K > 0)                                                                                                            \
    adists_window_lanes_group_kernel<P, CC><<<grid, 256, 0, st>>>(px, py, H, W, q, B, ctot, coff, wgt, g, gamma, tw, sw, K); \
  else                                                                                                                  \
    adists_window_lanes_kernel<P, CC><<<grid, 256, 0, st>>>(px, py, H, W, q, B, ctot, coff, wgt, g, gamma, tw, sw)
  switch (C) {
    case 64: NQA_LANES(64); break;
    case 128: NQA_LANES(128); break;
    case 256: NQA_LANES(256); break;
    case 512: NQA_LANES(512); break;
    default: set_error("adists_window_lanes: unsupported channel count %d", C); return NQA_E_SHAPE;
  }
#undef NQA_LANES
  return check_launch("adists_window_lanes");
}

static int launch_global(const float *q, int B, int ctot, int coff, int creal, const float *wgt, float *gamma,
                         float *tw, float *sw, hipStream_t st, int K = 0) {
  TimedLaunch t(NQA_K_ADISTS, st);
  if (K > 0)
    adists_global_group_kernel<<<B, 256, 0, st>>>(q, B, ctot, coff, creal, wgt, gamma, tw, sw, K);
  else
    adists_global_kernel<<<B, 256, 0, st>>>(q, B, ctot, coff, creal, wgt, gamma, tw, sw);
  return check_launch("adists_global");
}

// The window as the host computes it, or null (error set) if it is not the kernels' compile-time taps.
static const Gauss *checked_gauss(const char *who) {
  static const Gauss gauss = make_gauss();
  for (int i = 0; i < kWin; ++i)
    if (gauss.g[i] != kG[i]) {
      set_error("%s: this host's exp() gives a different Gaussian window than the kernels' constants "
                "(tap %d: %a vs %a)", who, i, (double)gauss.g[i], (double)kG[i]);
      return nullptr;
    }
  return &gauss;
}

// Strip height of the generic kernels: a strip pays n - 1 rows of vertical run-in, so it grows with the window (64 rows
// per 16 taps, up to 256) while the grid still holds ~4096 blocks (a block is one wave: 16 per CU), else 64 rows.
// strip_req in [1, Ho] replaces that choice (tests reach the multi-group strips at small shapes with it).
static int window_n_strip(int n, int Ho, int nbx, int B, int strip_req) {
  if (strip_req > 0) return strip_req;
  int strip = 64 * cdiv(n, 16);
  while (strip > 64 && (long)nbx * cdiv(Ho, strip) * B < 4096) strip -= 64;
  return min(strip, Ho);
}

// The generic window pass (nqa_window_n.h) of one stage with a window of n, H and W at least n.  K as above.
// The dynamic-LDS limit of a kernel is raised once per device, so to what the largest window needs (78.75 KiB).
static constexpr int kWindowNMaxLds = kWinMax * 5 * 64 * (int)sizeof(float);
template <typename P>
static int launch_window_n_lanes(const void *fx, const void *fy, int B, int H, int W, int C, const float *q, int ctot,
                                 int coff, const float *wgt, int n, float *gamma, float *tw, float *sw, hipStream_t st,
                                 int strip_req, int K) {
  const int Ho = H - (n - 1), Wo = W - (n - 1);
  const typename P::T *px = reinterpret_cast<const typename P::T *>(fx), *py = reinterpret_cast<const typename P::T *>(fy);
  if (C <= 0 || C % 64) {
    set_error("adists_window_n: unsupported channel count %d", C);
    return NQA_E_SHAPE;
  }
  const int strip = window_n_strip(n, Ho, Wo, B, strip_req);
  const int lds = n * 5 * 64 * (int)sizeof(float);
  dim3 grid(Wo, cdiv(Ho, strip), B);
  if (grid.y > 65535u) {
    set_error("adists_window_n: grid too large");
    return NQA_E_SHAPE;
  }
  int rc;
  if (K > 0) {
    if ((rc = lds_limit<adists_window_n_lanes_group_kernel<P>>(kWindowNMaxLds, "adists_window_n_lanes_group"))) return rc;
    TimedLaunch t(NQA_K_ADISTS, st);
    adists_window_n_lanes_group_kernel<P><<<grid, 64, lds, st>>>(px, py, H, W, C, q, B, ctot, coff, wgt, gauss_n(n), n,
                                                                 strip, gamma, tw, sw, K);
    return check_launch("adists_window_n_lanes_group");
  }
  if ((rc = lds_limit<adists_window_n_lanes_kernel<P>>(kWindowNMaxLds, "adists_window_n_lanes"))) return rc;
  TimedLaunch t(NQA_K_ADISTS, st);
  adists_window_n_lanes_kernel<P><<<grid, 64, lds, st>>>(px, py, H, W, C, q, B, ctot, coff, wgt, gauss_n(n), n, strip,
                                                         gamma, tw, sw);
  return check_launch("adists_window_n_lanes");
}

static int launch_window_n_planar(const float *x, const float *y, int B, int H, int W, const float *q, int ctot,
                                  int coff, const float *wgt, int n, float *gamma, float *tw, float *sw, hipStream_t st,
                                  int strip_req, int K) {
  const int Ho = H - (n - 1), Wo = W - (n - 1);
  const int nbx = cdiv(Wo, 64);
  const int strip = window_n_strip(n, Ho, nbx, B, strip_req);
  const int lds = n * 5 * 64 * (int)sizeof(float);
  dim3 grid(nbx, cdiv(Ho, strip), B);
  if (grid.y > 65535u) {
    set_error("adists_window_n: grid too large");
    return NQA_E_SHAPE;
  }
  int rc;
  if (K > 0) {
    if ((rc = lds_limit<adists_window_n_planar_group_kernel>(kWindowNMaxLds, "adists_window_n_planar_group"))) return rc;
    TimedLaunch t(NQA_K_ADISTS, st);
    adists_window_n_planar_group_kernel<<<grid, 64, lds, st>>>(x, y, H, W, q, B, ctot, coff, wgt, gauss_n(n), n, strip,
                                                               gamma, tw, sw, K);
    return check_launch("adists_window_n_planar_group");
  }
  if ((rc = lds_limit<adists_window_n_planar_kernel>(kWindowNMaxLds, "adists_window_n_planar"))) return rc;
  TimedLaunch t(NQA_K_ADISTS, st);
  adists_window_n_planar_kernel<<<grid, 64, lds, st>>>(x, y, H, W, q, B, ctot, coff, wgt, gauss_n(n), n, strip, gamma, tw,
                                                       sw);
  return check_launch("adists_window_n_planar");
}

// One stage of the heavy pass: the global branch for maps smaller than the window, the planar kernel for the image,
// else the lanes pass in the taps' storage type.  fx holds the x-side maps, fy the B pairs' y maps.  The forward's
// stage loop and the single-stage entry points all dispatch here (`who` names the caller in a refusal).  A window of
// 21 runs the three specialised kernels unless the calling thread's tuning asks for the generic ones; every other
// window (kWinMin..kWinMax, checked by the caller) runs the generic ones.
static int launch_window_stage(const char *who, const void *fx, const void *fy, int B, int K, int H, int W, int win,
                               int C, int prec, const float *q, int ctot, int coff, const float *wgt, float *gamma,
                               float *tw, float *sw, hipStream_t st, int strip = 0) {
  if (H < win || W < win) return launch_global(q, B, ctot, coff, C, wgt, gamma, tw, sw, st, K);
  if (win != kWin || adists_window_generic()) {
    if (C == 3)
      return launch_window_n_planar(static_cast<const float *>(fx), static_cast<const float *>(fy), B, H, W, q, ctot,
                                    coff, wgt, win, gamma, tw, sw, st, strip, K);
    switch (storage_prec(prec)) {
      case NQA_PREC_F32: return launch_window_n_lanes<PrecF32>(fx, fy, B, H, W, C, q, ctot, coff, wgt, win, gamma, tw, sw, st, strip, K);
      case NQA_PREC_BF16: return launch_window_n_lanes<PrecBF16>(fx, fy, B, H, W, C, q, ctot, coff, wgt, win, gamma, tw, sw, st, strip, K);
      default: return launch_window_n_lanes<PrecF16>(fx, fy, B, H, W, C, q, ctot, coff, wgt, win, gamma, tw, sw, st, strip, K);
    }
  }
  const Gauss *gp = checked_gauss(who);
  if (!gp) return NQA_E_LAUNCH;
  if (C == 3)
    return launch_window_planar(static_cast<const float *>(fx), static_cast<const float *>(fy), B, H, W, q, ctot, coff,
                                wgt, *gp, gamma, tw, sw, st, K);
  switch (storage_prec(prec)) {
    case NQA_PREC_F32: return launch_window_lanes<PrecF32>(fx, fy, B, H, W, C, q, ctot, coff, wgt, *gp, gamma, tw, sw, st, strip, K);
    case NQA_PREC_BF16: return launch_window_lanes<PrecBF16>(fx, fy, B, H, W, C, q, ctot, coff, wgt, *gp, gamma, tw, sw, st, strip, K);
    default: return launch_window_lanes<PrecF16>(fx, fy, B, H, W, C, q, ctot, coff, wgt, *gp, gamma, tw, sw, st, strip, K);
  }
}

}  // namespace nqa

using namespace nqa;

extern "C" {

size_t nqa_adists_workspace_bytes_n(int B, int H, int W, int window, int prec) {
  if (window_check("adists_workspace_bytes_n", window)) return 0;
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return make_plan(B, B, 0, H, W, prec, window).total;
}

size_t nqa_adists_workspace_bytes(int B, int H, int W, int prec) {
  return nqa_adists_workspace_bytes_n(B, H, W, kWin, prec);
}

}  // extern "C"

// The back part of the forward: the probability chain from the coarsest stage to the finest, the stages' D sums, D_b and,
// with map_out (pairs only), the as_map=True resampler.  The forwards and the two chain entry points all launch it
// through this function.  The probability part (moments, fold, the two min / max passes, the global branch's sigmoid)
// runs per x image; for groups chain_final_group_kernel / chain_global_group_kernel then take the K renders' D sums
// against each reference's ps_prod.  The D fold and adists_d_kernel run over the pairs.
struct ChainMaps {
  const float *gamma[NQA_NUM_TAPS], *tw[NQA_NUM_TAPS], *sw[NQA_NUM_TAPS];  // gamma (X, mh, mw); tw, sw (B, mh, mw)
  float *ps[NQA_NUM_TAPS];                                                 // ps_prod out, (X, mh, mw)
  int mh[NQA_NUM_TAPS], mw[NQA_NUM_TAPS];
  bool windowed[NQA_NUM_TAPS];
};

static int launch_chain(const ChainMaps &m, int X, int B, int K, int H, int W, ChainAcc *acc_x /* [6][X] */,
                        ChainAcc *acc_pair /* [6][B]; acc_x itself for pairs */,
                        double *cp /* chain_part_bytes(X, B) */, float *ones /* [X] */, float *d_out, float *map_out,
                        hipStream_t st) {
  int rc;
  {
    TimedLaunch t(NQA_K_ADISTS, st);
    chain_init_kernel<<<cdiv(6 * X, 256), 256, 0, st>>>(acc_x, 6 * X);
    if (K > 0) chain_init_kernel<<<cdiv(6 * B, 256), 256, 0, st>>>(acc_pair, 6 * B);
    // initial ps_prod = ones (ADISTS.py:75): a 1x1 map of 1 upsamples to the same constant
    ones_kernel<<<cdiv(X, 256), 256, 0, st>>>(ones, X);
    const float *prev = ones;
    int hp = 1, wp = 1;
    for (int k = 5; k >= 0; --k) {
      const float *gamma = m.gamma[k], *tw = m.tw[k], *sw = m.sw[k];
      float *psprod = m.ps[k];
      ChainAcc *ax = acc_x + (size_t)k * X, *ap = acc_pair + (size_t)k * B;
      if (m.windowed[k]) {
        const int n = m.mh[k] * m.mw[k];
        dim3 grid(min(cdiv(n, 256), kChainBlocks), X);
        chain_moments_kernel<<<grid, 256, 0, st>>>(gamma, n, cp);
        chain_fold_kernel<<<X, 256, 0, st>>>(cp, grid.x, 2, 0, ax);
        chain_psminmax_kernel<<<grid, 256, 0, st>>>(gamma, n, ax);
        chain_ppminmax_kernel<<<grid, 256, 0, st>>>(gamma, m.mh[k], m.mw[k], prev, hp, wp, ax);
        if (K > 0)
          chain_final_group_kernel<<<grid, 256, 0, st>>>(gamma, m.mh[k], m.mw[k], prev, hp, wp, tw, sw, psprod, ax, K, cp);
        else
          chain_final_kernel<<<grid, 256, 0, st>>>(gamma, m.mh[k], m.mw[k], prev, hp, wp, tw, sw, psprod, ax, cp);
        chain_fold_kernel<<<B, 256, 0, st>>>(cp, grid.x, 1, 1, ap);
      } else if (K > 0) {
        chain_global_group_kernel<<<cdiv(B, 256), 256, 0, st>>>(gamma, prev, hp * wp, tw, sw, psprod, ap, B, K);
      } else {
        chain_global_kernel<<<cdiv(B, 256), 256, 0, st>>>(gamma, prev, hp * wp, tw, sw, psprod, ap, B);
      }
      prev = psprod;
      hp = m.mh[k];
      wp = m.mw[k];
    }
    DDesc dd;
    for (int k = 0; k < 6; ++k) dd.n[k] = m.mh[k] * m.mw[k];
    adists_d_kernel<<<cdiv(B, 256), 256, 0, st>>>(acc_pair, dd, B, d_out);
    if ((rc = check_launch(K > 0 ? "adists_chain_group" : "adists_chain"))) return rc;
  }
  if (map_out) {
    MapDesc md;
    for (int k = 0; k < 6; ++k) {
      md.tw[k] = m.tw[k];
      md.sw[k] = m.sw[k];
      md.ps[k] = m.ps[k];
      md.mh[k] = m.mh[k];
      md.mw[k] = m.mw[k];
    }
    TimedLaunch t(NQA_K_ADISTS, st);
    adists_map_kernel<<<dim3(cdiv(H * W, 256), B), 256, 0, st>>>(md, H, W, map_out);
    if ((rc = check_launch("adists_map"))) return rc;
  }
  return NQA_OK;
}

// The front part of the forward behind the statistics sums: from the fp64 partial sums `part` of the six taps (left by
// stats_nchw, pool_stats and stats_nhwc) to the per-channel scalars q, the entropies of the x maps and the channel
// weights.  The forwards and nqa_adists_front all launch it through this function.  h, w, c: the six taps' dims (k = 0
// the image); taps[k - 1]: tap k, X + B images (the x images first).  The scalars are per pair -- for groups from
// adists_prep_group_kernel, a wave per value --; the NHWC4 conversion, the six entropy passes, their fold and the
// weights kernel run on the X x images alone.  x image i's inv_x / sum_x are those of its first pair: the entropy kernel
// indexes its two rows by image * stride, and the stride handed over is max(K, 1) rows of q.  hsum [X][ctot] receives
// the folded per-channel entropy; for pairs it is q's row 2, which is dead once the entropy kernels have run.
static int launch_front(const float *x, void *const *taps, int X, int B, int K, const int h[NQA_NUM_TAPS],
                        const int w[NQA_NUM_TAPS], const int c[NQA_NUM_TAPS], int prec, const StageDesc &sd,
                        const EntDesc &ed, const int ent_ppb[NQA_NUM_TAPS], const double *part,
                        float *q /* [8][B][ctot] */, float *img4x, double *ent, float *hsum, float *wgt /* [X][ctot] */,
                        hipStream_t st) {
  const int ctot = sd.ctot, H = h[0], W = w[0];
  int rc;
  {
    TimedLaunch t(NQA_K_ADISTS, st);
    if (K > 0)
      adists_prep_group_kernel<<<dim3(cdiv(ctot, 4), B), 256, 0, st>>>(part, sd, q, B);
    else
      adists_prep_kernel<<<dim3(cdiv(ctot, 256), B), 256, 0, st>>>(part, sd, q, B);
    if ((rc = check_launch(K > 0 ? "adists_prep_group" : "adists_prep"))) return rc;
  }
  {
    dim3 grid(cdiv(H * W, 256), X);
    TimedLaunch t(NQA_K_ADISTS, st);
    nchw3_to_nhwc4_kernel<<<grid, 256, 0, st>>>(x, img4x, H * W);
    if ((rc = check_launch("nchw3_to_nhwc4"))) return rc;
  }
  const size_t qst = (size_t)B * ctot;
  const int stride = ctot * (K > 0 ? K : 1);  // floats of a q row between two x images' first pairs
  // stage 0's q/wgt rows are indexed with channel < 3; the NHWC4 kernels read index 3 too, which
  // is channel 0 of stage 1 in the concatenated vector -- harmless: its feature value is 0 (entropy
  // term 0) and the window kernel masks c >= creal.
  if ((rc = launch_entropy<PrecF32>(img4x, X, H * W, 4, ent_ppb[0], q + 0 * qst + sd.coff[0], q + 2 * qst + sd.coff[0],
                                    stride, ent + ed.part_off[0], st)))
    return rc;
  for (int k = 1; k < 6; ++k) {
    const int hw = h[k] * w[k];
    const float *invx = q + 0 * qst + sd.coff[k], *sumx = q + 2 * qst + sd.coff[k];
    double *ep = ent + ed.part_off[k];
    switch (storage_prec(prec)) {  // (the x images are the first X of every tap)
      case NQA_PREC_F32: rc = launch_entropy<PrecF32>(taps[k - 1], X, hw, c[k], ent_ppb[k], invx, sumx, stride, ep, st); break;
      case NQA_PREC_BF16: rc = launch_entropy<PrecBF16>(taps[k - 1], X, hw, c[k], ent_ppb[k], invx, sumx, stride, ep, st); break;
      default: rc = launch_entropy<PrecF16>(taps[k - 1], X, hw, c[k], ent_ppb[k], invx, sumx, stride, ep, st); break;
    }
    if (rc) return rc;
  }
  {
    TimedLaunch t(NQA_K_ADISTS, st);
    adists_entropy_fold_kernel<<<dim3(cdiv(ctot, 4), X), 256, 0, st>>>(ent, ed, hsum);
    adists_weights_kernel<<<X, 256, 0, st>>>(hsum, ed, wgt);
    if ((rc = check_launch("adists_weights"))) return rc;
  }
  return NQA_OK;
}

// The forward behind the pyramid and its statistics sums, for both forms: per-pair scalars, the x images as NHWC4,
// entropies and channel weights; the heavy pass (tw / sw per pair, gamma per x image); the probability chain per x
// image, D per pair and, with map_out, the as_map=True resampler.  x: the X x images, y: the B y images; the
// plan's five taps and `part` are complete on entry and nothing here writes them.
static int adists_tail(const char *who, const float *x, const float *y, int X, int B, int K, const APlan &p, int prec,
                       char *base, float *d_out, float *map_out, hipStream_t st) {
  const size_t esz = prec_elem_bytes(prec);
  const int ctot = p.sd.ctot, H = p.h[0], W = p.w[0];
  float *q = reinterpret_cast<float *>(base + p.q);
  float *wgt = reinterpret_cast<float *>(base + p.wgt);
  void *taps[5];
  for (int k = 0; k < 5; ++k) taps[k] = base + p.taps[k];
  int rc;
  if ((rc = launch_front(x, taps, X, B, K, p.h, p.w, p.c, prec, p.sd, p.ed, p.ent_ppb,
                         reinterpret_cast<const double *>(base + p.part), q, reinterpret_cast<float *>(base + p.img4x),
                         reinterpret_cast<double *>(base + p.ent), reinterpret_cast<float *>(base + p.hsum), wgt, st)))
    return rc;
  ChainMaps cm;
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    float *gamma = reinterpret_cast<float *>(base + p.maps[k][0]);
    float *tw = reinterpret_cast<float *>(base + p.maps[k][1]);
    float *sw = reinterpret_cast<float *>(base + p.maps[k][2]);
    cm.gamma[k] = gamma;
    cm.tw[k] = tw;
    cm.sw[k] = sw;
    cm.ps[k] = reinterpret_cast<float *>(base + p.maps[k][3]);
    cm.mh[k] = p.mh[k];
    cm.mw[k] = p.mw[k];
    cm.windowed[k] = p.windowed[k];
    const void *fx = k == 0 ? static_cast<const void *>(x) : taps[k - 1];
    const void *fy = k == 0 ? static_cast<const void *>(y)
                            : static_cast<const char *>(taps[k - 1]) + (size_t)X * p.h[k] * p.w[k] * p.c[k] * esz;
    if ((rc = launch_window_stage(who, fx, fy, B, K, p.h[k], p.w[k], p.win, p.c[k], prec, q, ctot, p.sd.coff[k], wgt,
                                  gamma, tw, sw, st)))
      return rc;
  }
  return launch_chain(cm, X, B, K, H, W, reinterpret_cast<ChainAcc *>(base + p.acc_x),
                      reinterpret_cast<ChainAcc *>(base + p.acc_pair), reinterpret_cast<double *>(base + p.chain_part),
                      reinterpret_cast<float *>(base + p.ones), d_out, map_out, st);
}

static int adists_run(const float *x, const float *y, int B, int H, int W, int win, const void *packed, int prec,
                      void *ws, size_t ws_bytes, float *d_out, float *map_out, void *stream, float *s1_out = nullptr,
                      float *s2_out = nullptr) {
  if (!x || !y || !packed || !ws || !d_out) {
    set_error("adists_forward: null pointer");
    return NQA_E_ARG;
  }
  if (int rc = window_check("adists_forward", win)) return rc;
  if (B <= 0 || H <= 0 || W <= 0 || !prec_valid(prec)) {
    set_error("adists_forward: bad size or prec (B=%d H=%d W=%d prec=%d)", B, H, W, prec);
    return NQA_E_ARG;
  }
  if ((long)H * W * 64 * (long)prec_elem_bytes(prec) >= (1L << 31)) {
    set_error("adists_forward: image too large for 32-bit in-image byte offsets");
    return NQA_E_ARG;
  }
  const APlan p = make_plan(B, B, 0, H, W, prec, win);
  if (ws_bytes < p.total) {
    set_error("adists_forward: workspace %zu < %zu bytes", ws_bytes, p.total);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(ws);
  double *part = reinterpret_cast<double *>(base + p.part);
  void *taps[5];
  for (int k = 0; k < 5; ++k) taps[k] = base + p.taps[k];
  int rc;

  // ---- pyramids (x images [0,B), y images [B,2B)) with the global statistics per tap ----
  if ((rc = stats_nchw(x, y, B, 3, H * W, part + p.sd.part_off[0], st))) return rc;
  // (f32s stage 1 is conv1_regw_split_kernel: frames in f32s are >= 128 x 128 pixels under the default `auto`, far from
  // the tiny-frame knife edge that made a conv1_1 rounding pattern matter, section 4.4)
  rc = run_stages(x, y, B, base + p.bufA, base + p.bufB, 2 * B, H, W, packed, prec, taps,
                  [&](int k, void *tap, int hk, int wk, int ck, void *pool_dst) {
                    double *pk = part + p.sd.part_off[k + 1];
                    if (!pool_dst) return stats_nhwc(tap, B, hk * wk, ck, prec, pk, st);
                    const int rc2 = pool_stats(tap, B, hk, wk, ck, prec, pool_dst, pk, st);
                    return rc2 ? rc2 : 1;
                  },
                  st);
  if (rc) return rc;
  // ---- DISTS' S1 / S2 from the same sums (nqa_adists_dists_forward only).  `part` is complete here and nothing
  // below writes it: adists_prep_kernel reads it, hsum reuses rows of q, the chain's `ones` lives in bufB ----
  if (s1_out && (rc = finalize(part, p.sd, B, s1_out, s2_out, st))) return rc;
  // ---- front, heavy pass, probability chain, D, the as_map=True resampler ----
  return adists_tail("adists_forward", x, y, B, B, 0, p, prec, base, d_out, map_out, st);
}

// The back part on its own (include/nqa.h).  Workspace: ChainAcc[6][X], for groups ChainAcc[6][B], the chain's
// per-block partials, the X ones.
struct ChainPlan {
  size_t acc_x, acc_pair, part, ones, total;
};
static ChainPlan chain_plan(int X, int B, int K) {
  ChainPlan c;
  c.acc_x = c.acc_pair = 0;
  c.part = align_up((size_t)6 * X * sizeof(ChainAcc), 256);
  if (K > 0) {
    c.acc_pair = c.part;
    c.part += align_up((size_t)6 * B * sizeof(ChainAcc), 256);
  }
  c.ones = c.part + align_up(chain_part_bytes(X, B), 256);
  c.total = c.ones + align_up((size_t)X * sizeof(float), 256);
  return c;
}
static int chain_frame_check(const char *who, int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) {
    set_error("%s: bad size (B=%d H=%d W=%d)", who, B, H, W);
    return NQA_E_ARG;
  }
  if ((long)H * W * 64 * 4 >= (1L << 31)) {  // nqa_adists_forward's limit, for its widest element
    set_error("%s: image too large for 32-bit in-image byte offsets", who);
    return NQA_E_ARG;
  }
  return NQA_OK;
}
// nqa_adists_chain (group false: X pairs, K ignored) and nqa_adists_chain_group (X references of K renders) behind
// their argument lists: the refusals under the caller's name, then launch_chain on the caller's maps.
static int chain_entry(const char *who, bool group, const float *const *gamma, const float *const *tw,
                       const float *const *sw, int X, int K, int H, int W, int win, void *ws, size_t ws_bytes,
                       float *const *ps_prod, float *d, float *map, void *stream) {
  if (!gamma || !tw || !sw || !ws || !ps_prod || !d) {
    set_error("%s: null pointer", who);
    return NQA_E_ARG;
  }
  for (int k = 0; k < NQA_NUM_TAPS; ++k)
    if (!gamma[k] || !tw[k] || !sw[k] || !ps_prod[k]) {
      set_error("%s: null pointer (stage %d)", who, k);
      return NQA_E_ARG;
    }
  if (group && (X <= 0 || K <= 0 || (long)X * K > kAdistsGroupMaxPairs)) {
    set_error("%s: bad group (R=%d K=%d; at most %ld pairs)", who, X, K, kAdistsGroupMaxPairs);
    return NQA_E_ARG;
  }
  if (int rc = chain_frame_check(who, X, H, W)) return rc;
  if (int rc = window_check(who, win)) return rc;
  if (!group) K = 0;
  const int B = group ? X * K : X;
  const ChainPlan c = chain_plan(X, B, K);
  if (ws_bytes < c.total) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, c.total);
    return NQA_E_WORKSPACE;
  }
  ChainMaps cm;
  int h[NQA_NUM_TAPS], w[NQA_NUM_TAPS];
  tap_dims(H, W, h, w);
  map_dims(h, w, win, cm.mh, cm.mw, cm.windowed);
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    cm.gamma[k] = gamma[k];
    cm.tw[k] = tw[k];
    cm.sw[k] = sw[k];
    cm.ps[k] = ps_prod[k];
  }
  char *base = static_cast<char *>(ws);
  return launch_chain(cm, X, B, K, H, W, reinterpret_cast<ChainAcc *>(base + c.acc_x),
                      reinterpret_cast<ChainAcc *>(base + c.acc_pair), reinterpret_cast<double *>(base + c.part),
                      reinterpret_cast<float *>(base + c.ones), d, map, static_cast<hipStream_t>(stream));
}

extern "C" {

int nqa_adists_chain_dims_n(int H, int W, int window, int *mh, int *mw) {
  if (!mh || !mw) {
    set_error("adists_chain_dims: null pointer");
    return NQA_E_ARG;
  }
  if (int rc = chain_frame_check("adists_chain_dims", 1, H, W)) return rc;
  if (int rc = window_check("adists_chain_dims", window)) return rc;
  int h[NQA_NUM_TAPS], w[NQA_NUM_TAPS];
  bool windowed[NQA_NUM_TAPS];
  tap_dims(H, W, h, w);
  map_dims(h, w, window, mh, mw, windowed);
  int nwin = 0;
  for (int k = 0; k < NQA_NUM_TAPS; ++k) nwin += windowed[k] ? 1 : 0;
  return nwin;
}

int nqa_adists_chain_dims(int H, int W, int *mh, int *mw) { return nqa_adists_chain_dims_n(H, W, kWin, mh, mw); }

size_t nqa_adists_chain_bytes_n(int B, int H, int W, int window) {
  if (window_check("adists_chain_bytes_n", window)) return 0;
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return chain_plan(B, B, 0).total;
}

size_t nqa_adists_chain_bytes(int B, int H, int W) { return nqa_adists_chain_bytes_n(B, H, W, kWin); }

int nqa_adists_chain_n(const float *const *gamma, const float *const *tw, const float *const *sw, int B, int H, int W,
                       int window, void *ws, size_t ws_bytes, float *const *ps_prod, float *d, float *map,
                       void *stream) {
  return chain_entry("adists_chain", false, gamma, tw, sw, B, 0, H, W, window, ws, ws_bytes, ps_prod, d, map, stream);
}

int nqa_adists_chain(const float *const *gamma, const float *const *tw, const float *const *sw, int B, int H, int W,
                     void *ws, size_t ws_bytes, float *const *ps_prod, float *d, float *map, void *stream) {
  return nqa_adists_chain_n(gamma, tw, sw, B, H, W, kWin, ws, ws_bytes, ps_prod, d, map, stream);
}

}  // extern "C"

// The front part on its own (include/nqa.h): the statistics launches that nqa_adists_forward interleaves with its
// pyramid (stats_nchw, pool_stats per tap 1..4, stats_nhwc on tap 5: the same launch functions with the same arguments),
// then launch_front.  The taps' sizes are the caller's.  Workspace: pool_stats' discarded pooled maps, the x images as
// NHWC4, the statistics partials, the entropy partials.
struct FrontPlan {
  size_t pooled, img4x, part, ent, total;
  StageDesc sd;
  EntDesc ed;
  int h[NQA_NUM_TAPS], w[NQA_NUM_TAPS], c[NQA_NUM_TAPS], ent_ppb[NQA_NUM_TAPS];
};
static int front_check(const char *who, int B, const int *Hk, const int *Wk, int prec) {
  if (!Hk || !Wk) {
    set_error("%s: null pointer", who);
    return NQA_E_ARG;
  }
  if (B <= 0 || !prec_valid(prec)) {
    set_error("%s: bad size or prec (B=%d prec=%d)", who, B, prec);
    return NQA_E_ARG;
  }
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    if (Hk[k] <= 0 || Wk[k] <= 0) {
      set_error("%s: bad size or prec (tap %d: %d x %d)", who, k, Hk[k], Wk[k]);
      return NQA_E_ARG;
    }
    // in-image offsets are 32-bit in places (the NHWC4 image of stage 0 counts as 4 float channels)
    const long bytes = (long)Hk[k] * Wk[k] * (k == 0 ? 4 : kChns[k]) * (long)(k == 0 ? 4 : prec_elem_bytes(prec));
    if (bytes >= (1L << 31)) {
      set_error("%s: tap %d too large for 32-bit in-image byte offsets", who, k);
      return NQA_E_ARG;
    }
  }
  return NQA_OK;
}
static FrontPlan front_plan(int B, const int *Hk, const int *Wk, int prec) {
  FrontPlan p;
  memset(&p, 0, sizeof(p));
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    p.h[k] = Hk[k];
    p.w[k] = Wk[k];
    p.c[k] = k == 0 ? 3 : kChns[k];
  }
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += align_up(bytes, 256);
    return o;
  };
  size_t pooled = 0;  // 4 bytes per element: float, split16 records, or more than a 16-bit mode needs
  for (int k = 1; k <= 4; ++k) {
    const size_t n = (size_t)2 * B * ((p.h[k] + 1) / 2) * ((p.w[k] + 1) / 2) * p.c[k] * 4;
    pooled = n > pooled ? n : pooled;
  }
  p.pooled = take(pooled);
  p.img4x = take((size_t)B * p.h[0] * p.w[0] * 4 * 4);
  long doff, eoff;
  front_descs(B, B, 0, p.h, p.w, p.c, prec, p.sd, p.ed, p.ent_ppb, doff, eoff);
  p.part = take((size_t)doff * 8);
  p.ent = take((size_t)eoff * 8);
  p.total = off;
  return p;
}

extern "C" {

size_t nqa_adists_front_bytes(int B, const int *Hk, const int *Wk, int prec) {
  if (front_check("adists_front_bytes", B, Hk, Wk, prec)) return 0;
  return front_plan(B, Hk, Wk, prec).total;
}

int nqa_adists_front_grid(int B, const int *Hk, const int *Wk, int prec, int *grid) {
  if (!grid) {
    set_error("adists_front_grid: null pointer");
    return NQA_E_ARG;
  }
  if (int rc = front_check("adists_front_grid", B, Hk, Wk, prec)) return rc;
  const FrontPlan p = front_plan(B, Hk, Wk, prec);
  for (int k = 0; k < NQA_NUM_TAPS; ++k) {
    int tr = 0, tc = 0;
    if (k >= 1 && k <= 4) pool_stats_tiles((p.h[k] + 1) / 2, (p.w[k] + 1) / 2, p.c[k], prec, B, &tr, &tc);
    grid[4 * k + 0] = p.sd.nblk[k];
    grid[4 * k + 1] = tr;
    grid[4 * k + 2] = tc;
    grid[4 * k + 3] = p.ed.nblk[k];
  }
  return NQA_OK;
}

int nqa_adists_front(const float *x, const float *y, const void *const *taps, int B, const int *Hk, const int *Wk,
                     int prec, void *ws, size_t ws_bytes, float *q, float *wgt, void *stream) {
  if (!x || !y || !taps || !Hk || !Wk || !ws || !q || !wgt) {
    set_error("adists_front: null pointer");
    return NQA_E_ARG;
  }
  for (int k = 0; k < 5; ++k)
    if (!taps[k]) {
      set_error("adists_front: null pointer (tap %d)", k + 1);
      return NQA_E_ARG;
    }
  if (int rc = front_check("adists_front", B, Hk, Wk, prec)) return rc;
  const FrontPlan p = front_plan(B, Hk, Wk, prec);
  if (ws_bytes < p.total) {
    set_error("adists_front: workspace %zu < %zu bytes", ws_bytes, p.total);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(ws);
  double *part = reinterpret_cast<double *>(base + p.part);
  void *tp[5];
  for (int k = 0; k < 5; ++k) tp[k] = const_cast<void *>(taps[k]);
  int rc;
  if ((rc = stats_nchw(x, y, B, 3, p.h[0] * p.w[0], part + p.sd.part_off[0], st))) return rc;
  for (int k = 1; k <= 4; ++k)
    if ((rc = pool_stats(tp[k - 1], B, p.h[k], p.w[k], p.c[k], prec, base + p.pooled, part + p.sd.part_off[k], st)))
      return rc;
  if ((rc = stats_nhwc(tp[4], B, p.h[5] * p.w[5], p.c[5], prec, part + p.sd.part_off[5], st))) return rc;
  return launch_front(x, tp, B, B, 0, p.h, p.w, p.c, prec, p.sd, p.ed, p.ent_ppb, part, q,
                      reinterpret_cast<float *>(base + p.img4x), reinterpret_cast<double *>(base + p.ent),
                      q + (size_t)2 * B * p.sd.ctot, wgt, st);
}

}  // extern "C"

// One stage of the heavy pass on its own, dispatched as the loop above dispatches it (ctot = C, coff = 0).
static int window_stage_check(const char *who, int B, int H, int W, int win, int C, int prec, int strip) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || !prec_valid(prec)) {
    set_error("%s: bad size or prec (B=%d H=%d W=%d C=%d prec=%d)", who, B, H, W, C, prec);
    return NQA_E_ARG;
  }
  if (int rc = window_check(who, win)) return rc;
  const bool windowed = H >= win && W >= win;
  if (strip < 0 || (windowed && strip > H - (win - 1))) {
    set_error("%s: strip %d outside [0, %d]", who, strip, windowed ? H - (win - 1) : 0);
    return NQA_E_ARG;
  }
  if (C != 3 && C != 64 && C != 128 && C != 256 && C != 512) {
    set_error("%s: unsupported channel count %d (3, 64, 128, 256 or 512)", who, C);
    return NQA_E_SHAPE;
  }
  if ((long)H * W * C * (long)(C == 3 ? 4 : prec_elem_bytes(prec)) >= (1L << 31)) {
    set_error("%s: map too large for 32-bit in-image byte offsets", who);
    return NQA_E_SHAPE;
  }
  return NQA_OK;
}

extern "C" {

int nqa_adists_window_grid(int B, int H, int W, int C, int prec, int strip, int *grid) {
  if (!grid) {
    set_error("adists_window_grid: null pointer");
    return NQA_E_ARG;
  }
  if (int rc = window_stage_check("adists_window_grid", B, H, W, kWin, C, prec, strip)) return rc;
  grid[0] = grid[1] = grid[2] = 0;
  if (H >= kWin && W >= kWin && C != 3 && !adists_window_generic() && window_uses_lds(prec_elem_bytes(prec)))
    window_lds_grid(H - (kWin - 1), W - (kWin - 1), B, strip, grid[0], grid[1], grid[2]);
  return NQA_OK;
}

int nqa_adists_window_stage_n(const void *fx, const void *fy, int B, int H, int W, int window, int C, int prec,
                              const float *q, const float *wgt, int strip, float *gamma, float *tw, float *sw,
                              void *stream) {
  if (!fx || !fy || !q || !wgt || !gamma || !tw || !sw) {
    set_error("adists_window_stage: null pointer");
    return NQA_E_ARG;
  }
  if (int rc = window_stage_check("adists_window_stage", B, H, W, window, C, prec, strip)) return rc;
  return launch_window_stage("adists_window_stage", fx, fy, B, 0, H, W, window, C, prec, q, C, 0, wgt, gamma, tw, sw,
                             static_cast<hipStream_t>(stream), strip);
}

int nqa_adists_window_stage(const void *fx, const void *fy, int B, int H, int W, int C, int prec, const float *q,
                            const float *wgt, int strip, float *gamma, float *tw, float *sw, void *stream) {
  return nqa_adists_window_stage_n(fx, fy, B, H, W, kWin, C, prec, q, wgt, strip, gamma, tw, sw, stream);
}

int nqa_adists_forward_n(const float *x, const float *y, int B, int H, int W, int window, const void *packed, int prec,
                         void *ws, size_t ws_bytes, float *d_out, void *stream) {
  return adists_run(x, y, B, H, W, window, packed, prec, ws, ws_bytes, d_out, nullptr, stream);
}

int nqa_adists_forward(const float *x, const float *y, int B, int H, int W, const void *packed, int prec, void *ws,
                       size_t ws_bytes, float *d_out, void *stream) {
  return nqa_adists_forward_n(x, y, B, H, W, kWin, packed, prec, ws, ws_bytes, d_out, stream);
}

int nqa_adists_forward_map_n(const float *x, const float *y, int B, int H, int W, int window, const void *packed,
                             int prec, void *ws, size_t ws_bytes, float *d_out, float *map_out, void *stream) {
  if (!map_out) {
    set_error("adists_forward_map: null map pointer");
    return NQA_E_ARG;
  }
  return adists_run(x, y, B, H, W, window, packed, prec, ws, ws_bytes, d_out, map_out, stream);
}

int nqa_adists_forward_map(const float *x, const float *y, int B, int H, int W, const void *packed, int prec,
                           void *ws, size_t ws_bytes, float *d_out, float *map_out, void *stream) {
  return nqa_adists_forward_map_n(x, y, B, H, W, kWin, packed, prec, ws, ws_bytes, d_out, map_out, stream);
}

int nqa_adists_dists_forward_n(const float *x, const float *y, int B, int H, int W, int window, const void *packed,
                               int prec, void *ws, size_t ws_bytes, float *d_out, float *s1, float *s2, float *map_out,
                               void *stream) {
  if (!s1 || !s2) {
    set_error("adists_dists_forward: null similarity pointer");
    return NQA_E_ARG;
  }
  return adists_run(x, y, B, H, W, window, packed, prec, ws, ws_bytes, d_out, map_out, stream, s1, s2);
}

int nqa_adists_dists_forward(const float *x, const float *y, int B, int H, int W, const void *packed, int prec,
                             void *ws, size_t ws_bytes, float *d_out, float *s1, float *s2, float *map_out,
                             void *stream) {
  return nqa_adists_dists_forward_n(x, y, B, H, W, kWin, packed, prec, ws, ws_bytes, d_out, s1, s2, map_out, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// K renders against ONE reference, for R such groups (include/nqa.h, nqa_adists_forward_group).  Everything A-DISTS takes
// from x alone -- the reference's pyramid, its entropy weights, gamma and the probability chain -- runs once per
// reference; the window pass and the D sums run per pair r * K + k against it.
// ---------------------------------------------------------------------------------

// NQA_OK if the group forward takes these arguments, else NQA_E_ARG with the error set under the caller's name
static int group_args_check(const char *who, int R, int K, int H, int W, int prec) {
  if (R <= 0 || K <= 0 || H <= 0 || W <= 0) {
    set_error("%s: non-positive size (R=%d K=%d H=%d W=%d)", who, R, K, H, W);
    return NQA_E_ARG;
  }
  if ((long)R * K > kAdistsGroupMaxPairs) {
    set_error("%s: R*K = %ld pairs, more than %ld in one call (slice over R)", who, (long)R * K, kAdistsGroupMaxPairs);
    return NQA_E_ARG;
  }
  if (!prec_valid(prec)) {
    set_error(is_mixed(prec) ? "%s: the mixed modes are DISTS modes (prec %d): A-DISTS needs float precision in every layer"
                             : "%s: unknown prec %d", who, prec);
    return NQA_E_ARG;
  }
  if ((long)H * W * 64 * (long)prec_elem_bytes(prec) >= (1L << 31)) {
    set_error("%s: image too large for 32-bit in-image byte offsets", who);
    return NQA_E_ARG;
  }
  return NQA_OK;
}

extern "C" {

size_t nqa_adists_group_workspace_bytes_n(int R, int K, int H, int W, int window, int prec) {
  if (window_check("adists_group_workspace_bytes_n", window)) return 0;
  if (R <= 0 || K <= 0 || H <= 0 || W <= 0 || (long)R * K > kAdistsGroupMaxPairs || !prec_valid(prec)) return 0;
  if ((long)H * W * 64 * (long)prec_elem_bytes(prec) >= (1L << 31)) return 0;
  return make_plan(R, R * K, K, H, W, prec, window).total;
}

size_t nqa_adists_group_workspace_bytes(int R, int K, int H, int W, int prec) {
  return nqa_adists_group_workspace_bytes_n(R, K, H, W, kWin, prec);
}

int nqa_adists_forward_group(const float *ref, const float *renders, int R, int K, int H, int W, const void *packed,
                             int prec, void *ws, size_t ws_bytes, float *d_out, float *s1, float *s2, void *stream) {
  return nqa_adists_forward_group_n(ref, renders, R, K, H, W, kWin, packed, prec, ws, ws_bytes, d_out, s1, s2, stream);
}

int nqa_adists_forward_group_n(const float *ref, const float *renders, int R, int K, int H, int W, int window,
                               const void *packed, int prec, void *ws, size_t ws_bytes, float *d_out, float *s1,
                               float *s2, void *stream) {
  if (!ref || !renders || !packed || !ws || !d_out) {
    set_error("adists_forward_group: null pointer");
    return NQA_E_ARG;
  }
  if ((s1 == nullptr) != (s2 == nullptr)) {
    set_error("adists_forward_group: s1 and s2 must both be given or both be null");
    return NQA_E_ARG;
  }
  if (int rc = group_args_check("adists_forward_group", R, K, H, W, prec)) return rc;
  if (int rc = window_check("adists_forward_group", window)) return rc;
  const int B = R * K, n = R + B;
  const APlan p = make_plan(R, B, K, H, W, prec, window);
  if (ws_bytes < p.total) {
    set_error("adists_forward_group: workspace %zu < %zu bytes", ws_bytes, p.total);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(ws);
  const size_t esz = prec_elem_bytes(prec);
  double *part = reinterpret_cast<double *>(base + p.part);
  void *taps[5];
  for (int k = 0; k < 5; ++k) taps[k] = base + p.taps[k];
  int rc;

  // ---- one pyramid of R + R * K images (the references first, render (r, k) at image R + r * K + k), all five taps
  // kept; the group statistics kernels leave the pairs' sums in finalize's layout; the plain L2-pools follow ----
  if ((rc = group_stats_nchw(ref, renders, R, K, 3, H * W, part + p.sd.part_off[0], st))) return rc;
  rc = run_stages(ref, renders, R, base + p.bufA, base + p.bufB, n, H, W, packed, prec, taps,
                  [&](int k, void *tap, int hk, int wk, int ck, void *) {
                    const char *rn = static_cast<const char *>(tap) + (size_t)R * hk * wk * ck * esz;
                    return group_stats_nhwc(tap, rn, R, K, hk * wk, ck, prec, part + p.sd.part_off[k + 1], st);
                  },
                  st);
  if (rc) return rc;
  // ---- DISTS' S1 / S2 of the pairs from the same sums ----
  if (s1 && (rc = finalize(part, p.sd, B, s1, s2, st))) return rc;
  // ---- front on the references, heavy pass per pair, probability chain per reference, D per pair ----
  return adists_tail("adists_forward_group", ref, renders, R, B, K, p, prec, base, d_out, nullptr, st);
}

int nqa_adists_window_stage_group(const void *fx, const void *fy, int R, int K, int H, int W, int C, int prec,
                                  const float *q, const float *wgt, int strip, float *gamma, float *tw, float *sw,
                                  void *stream) {
  return nqa_adists_window_stage_group_n(fx, fy, R, K, H, W, kWin, C, prec, q, wgt, strip, gamma, tw, sw, stream);
}

int nqa_adists_window_stage_group_n(const void *fx, const void *fy, int R, int K, int H, int W, int window, int C,
                                    int prec, const float *q, const float *wgt, int strip, float *gamma, float *tw,
                                    float *sw, void *stream) {
  if (!fx || !fy || !q || !wgt || !gamma || !tw || !sw) {
    set_error("adists_window_stage_group: null pointer");
    return NQA_E_ARG;
  }
  if (R <= 0 || K <= 0 || (long)R * K > kAdistsGroupMaxPairs) {
    set_error("adists_window_stage_group: bad group (R=%d K=%d; at most %ld pairs)", R, K, kAdistsGroupMaxPairs);
    return NQA_E_ARG;
  }
  if (int rc = window_stage_check("adists_window_stage_group", R * K, H, W, window, C, prec, strip)) return rc;
  return launch_window_stage("adists_window_stage_group", fx, fy, R * K, K, H, W, window, C, prec, q, C, 0, wgt, gamma, tw, sw,
                             static_cast<hipStream_t>(stream), strip);
}

size_t nqa_adists_chain_group_bytes_n(int R, int K, int H, int W, int window) {
  if (window_check("adists_chain_group_bytes_n", window)) return 0;
  if (R <= 0 || K <= 0 || H <= 0 || W <= 0 || (long)R * K > kAdistsGroupMaxPairs) return 0;
  return chain_plan(R, R * K, K).total;
}

size_t nqa_adists_chain_group_bytes(int R, int K, int H, int W) {
  return nqa_adists_chain_group_bytes_n(R, K, H, W, kWin);
}

int nqa_adists_chain_group_n(const float *const *gamma, const float *const *tw, const float *const *sw, int R, int K,
                             int H, int W, int window, void *ws, size_t ws_bytes, float *const *ps_prod, float *d,
                             void *stream) {
  return chain_entry("adists_chain_group", true, gamma, tw, sw, R, K, H, W, window, ws, ws_bytes, ps_prod, d, nullptr,
                     stream);
}

int nqa_adists_chain_group(const float *const *gamma, const float *const *tw, const float *const *sw, int R, int K, int H,
                           int W, void *ws, size_t ws_bytes, float *const *ps_prod, float *d, void *stream) {
  return nqa_adists_chain_group_n(gamma, tw, sw, R, K, H, W, kWin, ws, ws_bytes, ps_prod, d, stream);
}

}  // extern "C"
