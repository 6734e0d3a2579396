// Shared device/host helpers for libnqa_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/nqa.h"

namespace nqa {

// ---- error plumbing ------------------------------------------------------------
void set_error(const char *fmt, ...);
int check_launch(const char *what);

// ---- timing ring (bench.py roofline leg) -----------------------------------------
struct TimedLaunch {
  TimedLaunch(int kclass, hipStream_t s);
  ~TimedLaunch();
  int kclass;
  hipStream_t stream;
  int slot;
};

// ---- precision traits ------------------------------------------------------------
// One 16-byte "k-chunk" is the unit every tile is staged and read in: 8 sixteen-bit
// channels or 4 floats.  A 64-byte pixel record (4 chunks) is one LDS row.
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// T: element type of the maps a kernel READS (and, normally, writes); TO: element type of what the pooling
// kernels WRITE (differs from T only at the mixed mode's f16 -> split16 boundary, PrecF16X).
struct PrecF32 {
  typedef float T;
  typedef float TO;
  static constexpr bool OUT_SPLIT16 = false;
  static constexpr int ID = NQA_PREC_F32;
  static constexpr int CPC = 4;   // channels per 16-byte chunk
  static constexpr int KC = 16;   // channels per 64-byte LDS row
  static constexpr bool SPLIT = false;
  __device__ static inline float to_f(T v) { return v; }
  __device__ static inline T from_f(float v) { return v; }
  // one chunk pair -> K=8 of the contraction as four exact-f32 MFMAs (K=2 each)
  __device__ static inline f32x16 mma(u32x4 a, u32x4 b, f32x16 c) {
    f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bf[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bf[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bf[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bf[3], c, 0, 0, 0);
    return c;
  }
};
// NQA_PREC_F32S: float precision carried as f16 (hi, lo) pairs so the convolutions run on the f16
// MFMA: a*b ~= ah*bh + ah*bl + al*bh (the dropped al*bl is ~2^-22 relative).  Weights are split
// at pack time.  Activations BETWEEN conv layers live in the "split16" format, written by the
// producing kernel's epilogue: 16 channels = 64 bytes [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15],
// hi = f16(v), lo = f16(v - hi) -- 4 bytes per element like float, same row layout as the packed
// weights, so both MFMA operands are plain 16-byte LDS reads.  The tapped maps (relu1_2 ... relu5_3,
// read by the statistics / pooling / A-DISTS kernels) are plain float.
struct PrecF32S : PrecF32 {
  static constexpr int ID = NQA_PREC_F32S;
  static constexpr bool SPLIT = true;
};
struct PrecBF16 {
  typedef __bf16 T;
  typedef __bf16 TO;
  static constexpr bool OUT_SPLIT16 = false;
  static constexpr int ID = NQA_PREC_BF16;
  static constexpr int CPC = 8;
  static constexpr int KC = 32;
  static constexpr bool SPLIT = false;
  __device__ static inline float to_f(T v) { return (float)v; }
  __device__ static inline T from_f(float v) { return (T)v; }
  __device__ static inline f32x16 mma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
  }
  // the 16x16x32 shape (one chunk pair -> K = 32 of a 16 x 16 tile)
  __device__ static inline f32x4 mma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
  }
};
struct PrecF16 {
  typedef _Float16 T;
  typedef _Float16 TO;
  static constexpr bool OUT_SPLIT16 = false;
  static constexpr int ID = NQA_PREC_F16;
  static constexpr int CPC = 8;
  static constexpr int KC = 32;
  static constexpr bool SPLIT = false;
  __device__ static inline float to_f(T v) { return (float)v; }
  __device__ static inline T from_f(float v) { return (T)v; }
  __device__ static inline f32x16 mma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
  }
  __device__ static inline f32x4 mma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
  }
};

// NQA_PREC_F32M, the L2-pool behind its last two-term stage: half taps in, split16 records out (they feed an
// f32s conv layer)
struct PrecF16X : PrecF16 {
  typedef float TO;  // 4 bytes per element
  static constexpr bool OUT_SPLIT16 = true;
};

// split16 store of the 4 consecutive channels c..c+3 (c % 4 == 0) of the pixel record at `pixel`
__device__ static inline void store_split4(char *pixel, int c, float v0, float v1, float v2, float v3) {
  typedef __attribute__((ext_vector_type(4))) _Float16 h4;
  const h4 hi = {(_Float16)v0, (_Float16)v1, (_Float16)v2, (_Float16)v3};
  const h4 lo = {(_Float16)(v0 - (float)hi[0]), (_Float16)(v1 - (float)hi[1]), (_Float16)(v2 - (float)hi[2]),
                 (_Float16)(v3 - (float)hi[3])};
  char *p = pixel + (c >> 4) * 64 + ((c >> 3) & 1) * 16 + (c & 7) * 2;
  *reinterpret_cast<h4 *>(p) = hi;
  *reinterpret_cast<h4 *>(p + 32) = lo;
}
// store one P::CPC-channel group (channels c..) of a pixel in the activation format `P` writes
template <typename P>
__device__ static inline void store_group(typename P::T *pixel, int c, const float (&v)[P::CPC]) {
  if constexpr (P::SPLIT) {
    store_split4(reinterpret_cast<char *>(pixel), c, v[0], v[1], v[2], v[3]);
  } else {
    typedef __attribute__((ext_vector_type(P::CPC))) typename P::T tvec;
    tvec o;
#pragma unroll
    for (int e = 0; e < P::CPC; ++e) o[e] = P::from_f(v[e]);
    *reinterpret_cast<tvec *>(pixel + c) = o;
  }
}

// what the pooling kernels write: P's own format, or split16 records at the mixed mode's boundary
template <typename P>
__device__ static inline void store_pooled(typename P::TO *pixel, int c, const float (&v)[P::CPC]) {
  if constexpr (P::OUT_SPLIT16 && sizeof(typename P::T) == 2) {
    store_split4(reinterpret_cast<char *>(pixel), c, v[0], v[1], v[2], v[3]);
    store_split4(reinterpret_cast<char *>(pixel), c + 4, v[4], v[5], v[6], v[7]);
  } else {
    store_group<P>(reinterpret_cast<typename P::T *>(pixel), c, v);
  }
}

// (NQA_PREC_F32M is a pyramid-level mode: its stages run as F16 / F32S kernels, see stage_prec; the packed blob
// holds 4 bytes per weight in it -- f16 hi + lo, or the f32s rows)
__host__ __device__ static inline size_t prec_elem_bytes(int prec) {
  return prec == NQA_PREC_F32 || prec == NQA_PREC_F32S ? 4 : 2;
}
static inline bool prec_valid(int prec) { return prec >= NQA_PREC_F32 && prec <= NQA_PREC_F32S; }  // kernel-level modes
static inline bool is_mixed(int prec) { return NQA_MIXED_STAGES(prec) > 0; }
static inline bool prec_valid_pyramid(int prec) { return prec_valid(prec) || is_mixed(prec); }
// the kernel precision of pyramid stage `stage` (0-based) in mode `prec`
static inline int stage_prec(int prec, int stage) {
  if (!is_mixed(prec)) return prec;
  return stage < NQA_MIXED_STAGES(prec) ? NQA_PREC_F16 : NQA_PREC_F32S;
}
// weight terms per product of conv layer `layer` in mode `prec` (2: f16 hi + lo against f16 activations)
static inline int layer_terms(int prec, int layer);
// the precision the kernels that READ tapped maps see: in f32s those are plain float
static inline int storage_prec(int prec) { return prec == NQA_PREC_F32S ? NQA_PREC_F32 : prec; }

// ---- VGG plan --------------------------------------------------------------------
struct ConvSpec {
  int cin, cout, stage;  // stage 0..4 (after which tap k=stage+1 is taken when last==1)
  int last;
};
static const ConvSpec kConvs[NQA_NUM_CONVS] = {
    {3, 64, 0, 0},    {64, 64, 0, 1},   {64, 128, 1, 0},  {128, 128, 1, 1}, {128, 256, 2, 0},
    {256, 256, 2, 0}, {256, 256, 2, 1}, {256, 512, 3, 0}, {512, 512, 3, 0}, {512, 512, 3, 1},
    {512, 512, 4, 0}, {512, 512, 4, 0}, {512, 512, 4, 1}};
static inline int layer_terms(int prec, int layer) {
  return kConvs[layer].stage < NQA_MIXED_STAGES(prec) ? 2 : 1;
}
static const int kChns[NQA_NUM_TAPS] = {3, 64, 128, 256, 512, 512};
static const int kChnOff[NQA_NUM_TAPS] = {0, 3, 67, 195, 451, 963};

// ---- Packed weight blob -------------------------------------------------------------------------------------------------
// What nqa_pack_vgg_weights writes for mode `prec` and every kernel reads (nqa_weights.hip: one walk over the sections
// below per mode fills a table, the accessors here read it).  Sections in blob order; sections 1..4 and each part of 4
// start on a multiple of 256 bytes, the fragment sections 5..6 follow one another without padding.
//   "16-bit modes" = bf16, f16 (elements in the mode's format); "two-term modes" = f32s and the mixed modes f32m, f32m2,
//   f32m4, f16w.  (hi, lo) of a weight w: hi = f16(w * s), lo = f16(w * s - hi), s the power of two that puts the
//   layer's largest |w| in [512, 1024) (so that lo is a normal half; 2^-8 <= s <= 2^24, s = 1 for an all-zero layer).
//
// 1. Zero page, 256 bytes: the source of out-of-image halo pixels.
// 2. Layer 0 (conv1_1) for the float kernels: float w[27][64], k = (ky*3+kx)*3 + c, then float bias[64].
// 3. conv1_1 as 32x32x16 MFMA A fragments, 6144 bytes: [ky][cout][h][8 elements], element j of half h is the weight of
//    (kx = 2h + j/4, c = j%4), i.e. k = ky*16 + kx*4 + c, zero for kx = 3 or c = 3.  16-bit modes only (conv1_fused_kernel,
//    conv1_tile_kernel).  f32: zeros.  Two-term modes: the first float is 1/s of section 6, the rest zeros.
// 4. Layers 1..12, each: its rows, then float bias[cout] followed by ONE float 1/s (1 where the rows are unscaled).
//    Rows are tiles [cout/64][cin/KC] of [9 taps][64 rows][4 positions of 16 bytes]; chunk c of row n lies at position
//    c ^ ((n>>2)&3), or c ^ 2*((n>>2)&1) in the 16-bit and two-term-row layers 2..12 (read by the 16x16x32 MFMA).  The
//    64-channel granularity lets any block tile that is a multiple of 64 channels stream whole sub-slabs.  By the kernel
//    precision that reads the layer (stage_prec, layer_terms):
//      f32            KC = 16; chunk c = 4 floats, input channels 4c.. of the tile
//      bf16, f16      KC = 32; chunk c = 8 elements, channels 8c..
//      f32s           KC = 16; chunk c = 8 halfs, channels 8(c&1)..: hi for c < 2, lo for c >= 2 (4 bytes per weight)
//      two-term rows  (a mixed mode's layers up to its boundary) KC = 32; the tile is [ky][hi, lo][kx][64 rows][4
//                     positions] (18 slabs); chunk c = 8 halfs, channels 8c.. (4 bytes per weight)
// 5. Layers 1..4 (conv1_2, conv2_1: Cin 64; conv2_2, conv3_1: Cin 128) whole as 16x16x32 MFMA A fragments for the
//    register-weights kernels: [cout/16 tiles][terms][Cin/32 * 9 k-steps][64 lanes][8 halfs], k-step = chunk * 9 + tap,
//    element j of lane (row l15 = lane & 15, k-group c4 = lane >> 4) = w[16*tile + l15][32*chunk + 8*c4 + j][tap].
//    16-bit modes: one term (a kernel's 32-channel group = two consecutive tiles).  Two-term modes: the tile's hi, then
//    its lo, with the s of the layer's rows; f32s carries layers 1..2 only.  f32: none.
// 6. conv1_1 as 16x16x32 A fragments: [4 tiles of 16 channels][2 MFMAs][terms][64 lanes][8 halfs]; MFMA m contracts
//    kernel rows 2m and 2m+1: k = 8*c4 + j = 16*(ky - 2m) + 4*kx + c (kx, c padded to 4; zero for ky = 3).  Terms and
//    modes as in 5 (8192 bytes per term); the two-term s is conv1_1's own, its 1/s heads section 3.
static constexpr size_t kZeroPage = 256;
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t layer_offset(int layer, int prec);       // sections 2 / 4: the layer's weights (layer 0..12)
size_t layer_bias_offset(int layer, int prec);  // its bias (layers 1..12: and 1/s)
size_t layer0_mfma_offset(int prec);            // section 3
size_t regw_offset(int layer, int prec);        // section 5, layer 1..4
size_t layer0_m16_offset(int prec);             // section 6
// a layer packed alone by nqa_pack_conv_split: f32s rows, then (at this offset) a zero bias[cout] and 1/s
size_t conv_split_bias_off(int cout, int cin);
// a layer packed alone by nqa_pack_conv_half: f16 rows (kRows16), then (at this offset) a zero bias[cout]
size_t conv_half_bias_off(int cout, int cin);

// Where each stage's partial sums live and how to fold them (finalize_kernel).
struct StageDesc {
  long part_off[NQA_NUM_TAPS];  // offset (in doubles) of each stage's partial block
  int nblk[NQA_NUM_TAPS];
  int hw[NQA_NUM_TAPS];
  int c[NQA_NUM_TAPS];
  int coff[NQA_NUM_TAPS];  // channel offset of the stage inside the concatenated vector
  int nstage;
  int ctot;
};

// Moments of one (pair b, global channel gc) from a stage's per-block partial sums, folded by one wave (lane = 0..63:
// lanes stride over the blocks, then a shuffle tree; the total is valid in lane 0): mx, my, vx, vy, cov in fp64.
// Returns the stage k and its channel c.  (finalize_kernel and the statistics' backward share it, so the backward
// differentiates exactly the numbers the forward formed.)
struct PlaneMoments {
  int k, c;
  double mx, my, vx, vy, cov, inv;
};
__device__ inline PlaneMoments plane_moments(const double *__restrict__ part, const StageDesc &d, int b, int gc, int lane) {
  PlaneMoments m;
  int k = 0;
  while (k + 1 < d.nstage && gc >= d.coff[k + 1]) ++k;
  const int c = gc - d.coff[k];
  const double *p = part + d.part_off[k] + ((size_t)b * d.nblk[k] * d.c[k] + c) * 5;
  double s[5] = {0, 0, 0, 0, 0};
  for (int blk = lane; blk < d.nblk[k]; blk += 64) {
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] += p[(size_t)blk * d.c[k] * 5 + q];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q)
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off, 64);
  m.k = k;
  m.c = c;
  m.inv = 1.0 / (double)d.hw[k];
  m.mx = s[0] * m.inv;
  m.my = s[1] * m.inv;
  m.vx = s[2] * m.inv - m.mx * m.mx;
  m.vy = s[3] * m.inv - m.my * m.my;
  m.cov = s[4] * m.inv - m.mx * m.my;
  return m;
}

size_t max_act_elems(int H, int W);  // largest activation map of the pyramid, elements per image (nqa_api.hip)

// ---- launch preparation (nqa_api.hip) ----------------------------------------------------
int current_device();  // a failing hipGetDevice reads as device 0
// compute units of the current device, cached per device (a process may drive several); 0 if the device cannot be
// queried, with "<who>: cannot query the device" as the error when `who` is given
int num_cus(const char *who);
int raise_lds_limit(const void *kernel, std::atomic<bool> *done_dev, int bytes, const char *who);
// Raises the dynamic-LDS limit of kernel K to `bytes`, once per device (the attribute is per device) and per
// instantiation: the flags belong to K.  NQA_OK, or NQA_E_LAUNCH with the error set under the kernel's name `who`.
template <auto K>
static int lds_limit(int bytes, const char *who) {
  static std::atomic<bool> done_dev[64];
  return raise_lds_limit(reinterpret_cast<const void *>(K), done_dev, bytes, who);
}

// ---- tuning state: what nqa_set_conv_variant decodes (include/nqa.h), A/B switches for the tools and tests ----
// One object per thread (nqa_api.hip): a choice made by one thread never changes what another thread's calls launch.
struct Tuning {
  int conv_variant = 1;        // bits 0-1.  0: 4-wave tiles everywhere; 1: + 8-wave 256x256 tiles; 2: + 8-wave 128x512 tiles
  int stage1_variant = 0;      // bit 2.  0: persistent kernels (conv1_regw_kernel / conv1_fused_kernel); 1: conv1_tile_kernel
  bool window_legacy = false;  // bit 3: the first form of the A-DISTS window pass (no sharing through LDS)
  bool first_forms = false;    // bit 4: the round-1 forms of stage 1 (two-phase kernel) and conv2_1 (implicit GEMM)
  bool no_regw128 = false;     // bit 5: conv2_2 / conv3_1 on the implicit GEMM instead of the register-weights kernel
  bool fuse_taps = true;       // bit 6 clear: conv2_2 + L2-pool + statistics in one kernel (nqa_conv_pool.hip)
  bool fuse_stage1 = true;     // bit 7 clear: stage 1 + L2-pool + statistics in one kernel (nqa_conv1_pool.hip)
  // bits 8-9, the grid of the implicit GEMM on maps with 1 <= W % 32 <= 16: 0 = mixed (16-wide tiles on the right
  // edge) where it saves a round of blocks, 1 = plain grids only, 2 = mixed on every such map (tests, at small sizes)
  int edge_grid = 0;
  bool window_generic = false;  // bit 11: a window of 21 runs the generic window kernels (nqa_window_n.h) as well
  // bit 12: a window of 21 under MomentsKernels::Tuned (the _n window-moments / stage-backward entry points) runs the
  // generic kernels (nqa_window_moments_n.hip) as well
  bool moments_generic = false;
  int mixed_launches = 0;  // mixed grids this thread has launched since it last asked (variant 1024)
};
Tuning &tuning();

// ---- host launchers shared between translation units ---------------------------------
// The conv entry points take the BLOB's mode `prec`, plain or mixed, and run the layer with the kernels of its own
// stage (stage_prec / layer_terms: in a mixed mode F16 on two-term weights up to the boundary, F32S behind it).
int conv1_1(const float *x, int n, int H, int W, const void *packed, int prec, void *out, hipStream_t st);
// stage 1 (conv1_1 + conv1_2) of images [x(0..B), y(0..n-B)) in one kernel; every mode but NQA_PREC_F32 has one
int conv1_fused(const float *x, const float *y, int B, int n, int H, int W, const void *packed, int prec, void *out,
                hipStream_t st);
// whether the pyramid runs stage 1 of W-wide frames as conv1_fused (else conv1_1 followed by layer 1)
bool stage1_is_fused(int prec, int W);
// an F32S layer leaves plain float where it is tapped, split16 records otherwise
int conv3x3(const void *in, int n, int H, int W, int layer, const void *packed, int prec, void *out, hipStream_t st);
int relu_mask_split16(const float *g, const void *act, int act_split, long npix, int C, void *out, hipStream_t st);
int l2pool_backward(const float *x, const void *y_split16, const float *gy, int n, int H, int W, int C, float *gx,
                    hipStream_t st);
int conv1_1_backward(const float *gm, const float *w_oihw, int n, int H, int W, float *gimg, hipStream_t st);
// the same three with the chain's power-of-two renormalisation read from device memory (per image: kexp the exponent
// of the step, ktot the running total), nqa_backward.hip
int relu_mask_split16_scaled(const float *g, const void *act, int act_split, int n, long pix_per_image, int C,
                             const int *kexp, void *out, hipStream_t st);
int l2pool_backward_scaled(const float *x, const float *gy, const float *g_tap, const int *ktot, int n, int H, int W,
                           int C, float *out, hipStream_t st);
int conv1_1_backward_scaled(const float *g, const void *act0_split16, const float *w_oihw, const int *kexp,
                            const int *ktot, int n, int H, int W, float *gimg, hipStream_t st);
// the half gradient chain (grad_precision "f16"): plain half NHWC gradient maps, per-image exponents with max|g| 2^k in
// [8, 16); g_half: whether g is a half map (else float)
int relu_mask_f16_scaled(const void *g, int g_half, const void *act, int act_split, int n, long pix_per_image, int C,
                         const int *kexp, void *out, hipStream_t st);
int l2pool_backward_scaled_half(const float *x, const void *gy_f16, const float *g_tap, const int *ktot, int n, int H, int W,
                                int C, float *out, hipStream_t st);
int conv1_1_backward_scaled_half(const void *g_f16, const void *act0_split16, const float *w_oihw, const int *kexp,
                                 const int *ktot, int n, int H, int W, float *gimg, hipStream_t st);
int grad_exponent_half(const void *g, int g_half, int n, long per_image, unsigned *ws, int *kexp, int *ktot, hipStream_t st);
int conv3x3_half_generic(const void *in, int n, int H, int W, int cin, int cout, const void *blob, size_t bias_off, void *out,
                         hipStream_t st);
// ---- the loss path (nqa_loss_backward.hip): statistics' gradient on NHWC taps, renormalisation exponents ----
size_t loss_stats_backward_doubles(int B, int HW, int C);
int loss_stats_backward(const float *tx, const float *ty, int B, int HW, int C, const float *g_s1, const float *g_s2,
                        long g_stride, double *ws, float *gx, float *gy, hipStream_t st);
// its two halves for a loss against a prepared target: the forward leaves the sums' partials ([B][nblk][C][5] doubles)
// and S1 / S2 (pair b's C values at s + b * s_stride); the backward starts from them (coef: [B][C][6] doubles)
size_t loss_stats_partials_doubles(int B, int HW, int C);
size_t loss_stats_coef_doubles(int B, int C);
int loss_stats_target(const float *tx, const float *ty, int B, int HW, int C, double *part, float *s1, float *s2,
                      long s_stride, hipStream_t st);
int loss_stats_backward_from(const float *tx, const float *ty, int B, int HW, int C, const double *part, const float *g_s1,
                             const float *g_s2, long g_stride, double *coef, float *gx, float *gy, hipStream_t st);
// loss_stats_backward_from for the y side alone, added into the gradient gy already holds (gy += u, one float add)
int loss_stats_grad_y_add(const float *tx, const float *ty, int B, int HW, int C, const double *part, const float *g_s1,
                          const float *g_s2, long g_stride, double *coef, float *gy, hipStream_t st);
int grad_exponent_nblk(long per_image);
int grad_exponent(const float *g, int n, long per_image, unsigned *ws, int *kexp, int *ktot, hipStream_t st);
// ---- windowed moments of the A-DISTS head and their backward (nqa_window_moments_n.hip, nqa_window_moments.hip) ----
// Which kernels a window of 21 runs (every other window has the generic ones alone).  Tuned: the 21-tap kernels unless
// Tuning::moments_generic is set, what the _n entry points pass; Taps21: the 21-tap kernels whatever the tuning state
// says, what the entry points without a window pass.
enum class MomentsKernels { Tuned, Taps21 };
// a window of n taps, 3 <= n <= 63: h = H - n + 1, w = W - n + 1.  out: moment m of plane p at (m * P + p) * h * w (five
// moments with y, two without); g[q] null = zero
int window_moments_forward(const float *x, const float *y, int P, int H, int W, int n, MomentsKernels kernels, float *out,
                           hipStream_t st);
int window_moments_backward(const float *x, const float *y, int P, int H, int W, int n, MomentsKernels kernels,
                            const float *const g[5], float *gx, float *gy, hipStream_t st);
// window_taps_n: gaussian(n, n / 3), the generic scoring kernels' table (nqa_adists.hip); window_check_n: NQA_E_ARG
// naming the range for a window outside it.
const float *window_taps_n(int n);
int window_check_n(const char *who, int window);
// ---- one stage of the A-DISTS head's backward towards y (nqa_adists_backward.hip) ----
// planar float maps (B, C, H, W); a window of `window` taps (3 .. 63) on the window moments above; q [8][B][ctot] and
// wgt [B][ctot] with the stage's channels at coff; ps (B, mh, mw); u (B) = dL/dD; gy planar, or NHWC (B, H, W, C) with
// out_nhwc (C % 32 == 0 on a windowed stage)
bool adists_ts_backward_fits(int B, int C, int H, int W, int window);
size_t adists_ts_backward_bytes(int B, int C, int H, int W, int window);
int adists_ts_backward(const float *x, const float *y, int B, int C, int H, int W, int window, MomentsKernels kernels,
                       const float *q, const float *wgt, int ctot, int coff, const float *ps, const float *u, int mask,
                       int out_nhwc, void *ws, float *gy, hipStream_t st);
int conv3x3_split_generic(const void *in, int n, int H, int W, int cin, int cout, const void *blob, size_t bias_off,
                          int relu, void *out, hipStream_t st);
int l2pool_to_split16(const void *in_f16, int n, int H, int W, int C, void *out_split16, hipStream_t st);
int pool_stats_to_split16(const void *feat_f16, int B, int H, int W, int C, void *pooled_split16, double *part,
                          hipStream_t st);
int l2pool(const void *in, int n, int H, int W, int C, int prec, void *out, hipStream_t st);
int stats_units_per_block(int units, int C, int prec, int B);
int stats_nchw_ppb(int HW);
int pool_stats_tiles(int Ho, int Wo, int C, int prec, int B, int *tr, int *tc);
int pool_stats(const void *feat, int B, int H, int W, int C, int prec, void *pooled, double *part, hipStream_t st);
int stats_nhwc(const void *feat, int B, int HW, int C, int prec, double *part, hipStream_t st);
int stats_nchw(const float *fx, const float *fy, int B, int C, int HW, double *part, hipStream_t st);
int finalize(const double *part, const StageDesc &d, int B, float *s1, float *s2, hipStream_t st);
// ---- one reference against its K renders (nqa_group_stats.hip): R reference maps, then render (r, k) at r * K + k;
// partial sums in finalize's layout with B := R * K, pair p = r * K + k ----
int group_stats_units_per_block(int units, int C, int prec, int R);
bool group_stats_nhwc_ok(int C, int prec);
int group_stats_nhwc(const void *ref, const void *ren, int R, int K, int HW, int C, int prec, double *part, hipStream_t st);
int group_stats_nchw(const float *ref, const float *ren, int R, int K, int C, int HW, double *part, hipStream_t st);
// ---- backward of the NCHW statistics (nqa_stats_backward.hip; forward_from_feats under autograd) ----
// per-plane fp64 coefficients {mx, my, a, b, ox, oy} from the forward's partials and dL/dS1, dL/dS2 (B, ctot);
// tap k's planes (b, c) at record B * coff[k] + b * C[k] + c
int stats_coef(const double *part, const StageDesc &d, int B, const float *g_s1, const float *g_s2, double *coef,
               hipStream_t st);
// gx[k] / gy[k] (either may be null) from the maps and those coefficients, all six taps in one launch
int stats_grad(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B, const int C[NQA_NUM_TAPS],
               const int HW[NQA_NUM_TAPS], const double *coef, float *const gx[NQA_NUM_TAPS], float *const gy[NQA_NUM_TAPS],
               hipStream_t st);
int score(const float *s1, const float *s2, const float *alpha, const float *beta, int B, float *out, hipStream_t st);
int nhwc_to_nchw(const void *in, int n, int HW, int C, int prec, float *out, hipStream_t st);
// ---- conv + L2-pool + statistics in one kernel (nqa_conv_pool.hip; the DISTS path's tap 2) ----
// rows of statistics partials a fused tap reserves per pair (= the largest grid the fused kernel runs; unwritten rows are zero)
#define NQA_FUSED_PART_BLOCKS 256
#define NQA_FUSED_PART_BLOCKS_S1 512  // (the fused stage 1 leaves two rows per block)
int pool_seam_finish(const float *seam, void *pooled, int nimg, int strips, int Ho, int Wo, int C, hipStream_t st);
bool conv1_pool_fusable(int B, int H, int W, int blob_prec);
int conv1_pool_stats_fused(const float *x, const float *y, int B, int H, int W, const void *packed, void *pooled, float *seam,
                           double *part, hipStream_t st);
bool conv_pool_fusable(int layer, int B, int H, int W, int blob_prec, int kprec);
size_t conv_pool_seam_bytes(int B, int H, int W, int C);
int conv_pool_stats_fused(const void *in, int B, int H, int W, int layer, const void *packed, int blob_prec, void *pooled,
                          float *seam, double *part, hipStream_t st);

}  // namespace nqa
