// Statistics of ONE reference against its K renders (nerf_qa/DISTS_pytorch/DISTS_pt.py:131-139 for the R * K pairs of R
// groups): the reference's scoring tables (test2_prep.py:89,201,304,404) hold several rows per reference_folder, and the
// pairwise kernels of nqa_pool_stats.hip would read -- and the pyramid would compute -- the reference once per row.
//
//   group_stats_nhwc_kernel   taps 1..5: a block owns a pixel strip of reference r, holds it in registers and walks the
//                             K renders of the group against it; (1 + K) maps are read per tap, not 2 K
//   group_stats_nchw_kernel   the same on float32 planes (tap 0 = the raw images), fp64 throughout like stats_nchw_kernel
//
// Batch layout: n = R + R * K images, the references first, render (r, k) at image R + r * K + k; pair p = r * K + k.
// Partial sums: part[((p * nblk + blk) * C + c) * 5 + s], the layout finalize_kernel folds with B := R * K.  Every
// element has one writer, nothing is atomic: two runs are bit-identical, and a pair's sums do not depend on which other
// renders share its group or in which order.
#include "nqa_common.h"
#include "nqa_moments.h"

namespace nqa {

// strip items a thread keeps of the reference: 16 x 16 bytes = 64 VGPRs; the launchers never plan longer strips
#define NQA_GROUP_ITEMS 16

// (the strip stays live across reduce_store's fp64 conversions: 170 VGPRs in the float instance, two blocks per CU; 282
// with the AGPRs in the 16-bit ones, one block per CU -- asking for two or three spills 108 or 12 bytes per lane)
template <typename P>
__global__ __launch_bounds__(256) void group_stats_nhwc_kernel(const typename P::T *__restrict__ ref,
                                                               const typename P::T *__restrict__ ren, int K, int HW, int C,
                                                               int pix_per_block, int nblk, double *__restrict__ part) {
  typedef typename P::T T;
  typedef __attribute__((ext_vector_type(P::CPC))) T tvec;
  __shared__ double red[256 * P::CPC];
  const int tid = threadIdx.x;
  const int r = blockIdx.x / nblk, blk = blockIdx.x - r * nblk;
  const int G = C / P::CPC;   // 16-byte channel groups per pixel (<= 128)
  const int PL = 256 / G;     // pixels handled side by side
  const int g = tid % G, pl = tid / G;
  const int p_begin = blk * pix_per_block + pl;
  const int p_end = min(HW, blk * pix_per_block + pix_per_block);
  const T *fx = ref + (size_t)r * HW * C + g * P::CPC;
  // the thread's part of the reference strip, loaded once
  tvec X[NQA_GROUP_ITEMS];
  int n = 0;
#pragma unroll
  for (int i = 0; i < NQA_GROUP_ITEMS; ++i) {
    const int p = p_begin + i * PL;
    if (p < p_end) {
      X[i] = *reinterpret_cast<const tvec *>(fx + (size_t)p * C);
      n = i + 1;
    } else {
      X[i] = (tvec)(T)0;
    }
  }
  for (int k = 0; k < K; ++k) {
    const size_t pair = (size_t)r * K + k;
    const T *fy = ren + pair * HW * C + g * P::CPC;
    ShiftedMoments<P::CPC> m;
    m.init();
    if (n) {
      unpack2<P>(X[0], m.px);
      unpack2<P>(*reinterpret_cast<const tvec *>(fy + (size_t)p_begin * C), m.py);
    }
#pragma unroll
    for (int i = 0; i < NQA_GROUP_ITEMS; ++i) {
      if (i < n) {
        const tvec vy = *reinterpret_cast<const tvec *>(fy + (size_t)(p_begin + i * PL) * C);
        f32x2 A[P::CPC / 2], B[P::CPC / 2];
        unpack2<P>(X[i], A);
        unpack2<P>(vy, B);
#pragma unroll
        for (int e = 0; e < P::CPC / 2; ++e) m.add2(e, A[e], B[e]);
      }
    }
    m.n = n;
    reduce_store<P::CPC>(m, red, tid, G, PL, C, part + (pair * nblk + blk) * C * 5);
  }
}

// float32 planes: grid (R * C, nblk).  ref: (R, C, HW), ren: (R * K, C, HW).
__global__ __launch_bounds__(256) void group_stats_nchw_kernel(const float *__restrict__ ref, const float *__restrict__ ren,
                                                               int K, int C, int HW, int pix_per_block,
                                                               double *__restrict__ part) {
  __shared__ double red[5][256];
  const int tid = threadIdx.x;
  const int rc = blockIdx.x, blk = blockIdx.y, nblk = gridDim.y;
  const int r = rc / C, c = rc - r * C;
  const float *px = ref + (size_t)rc * HW;
  const int p_begin = blk * pix_per_block + tid;
  const int p_end = min(HW, blk * pix_per_block + pix_per_block);
  float X[NQA_GROUP_ITEMS];
#pragma unroll
  for (int i = 0; i < NQA_GROUP_ITEMS; ++i) {
    const int p = p_begin + i * 256;
    X[i] = p < p_end ? px[p] : 0.f;
  }
  for (int k = 0; k < K; ++k) {
    const size_t pair = (size_t)r * K + k;
    const float *py = ren + (pair * C + c) * HW;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
    for (int i = 0; i < NQA_GROUP_ITEMS; ++i) {
      const int p = p_begin + i * 256;
      if (p < p_end) {
        const double x = (double)X[i], y = (double)py[p];
        a0 += x;
        a1 += y;
        a2 = fma(x, x, a2);
        a3 = fma(y, y, a3);
        a4 = fma(x, y, a4);
      }
    }
    __syncthreads();  // (the previous render's totals have been read)
    red[0][tid] = a0;
    red[1][tid] = a1;
    red[2][tid] = a2;
    red[3][tid] = a3;
    red[4][tid] = a4;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) {
#pragma unroll
        for (int s = 0; s < 5; ++s) red[s][tid] += red[s][tid + off];
      }
      __syncthreads();
    }
    if (tid < 5) part[((pair * nblk + blk) * C + c) * 5 + tid] = red[tid][0];
  }
}

// ---------------------------------------------------------------------------------
// Pixels per block of the NHWC kernel: the split of stats_units_per_block (4..16 items per thread, ~1024 blocks over the
// R references, fewer for wide taps), without its cap on the block count -- a strip has to fit the registers, so a large
// map takes more blocks instead of longer strips.  A block reads (1 + K) * 64 KB at 16 items and leaves K * C * 40 bytes
// of partial sums: 4 % of what it read at C = 64, 30 % at C = 512, where the maps are small.
int group_stats_units_per_block(int units, int C, int prec, int R) {
  prec = storage_prec(prec);
  const int cpc = prec == NQA_PREC_F32 ? 4 : 8;
  const int PL = 256 / (C / cpc);
  if (R < 1) R = 1;
  const long target_blocks = C >= 512 ? 384 : (C >= 256 ? 768 : 1024);
  long per_thread = (long)units * R / ((long)PL * target_blocks);
  per_thread = per_thread < 4 ? 4 : (per_thread > NQA_GROUP_ITEMS ? NQA_GROUP_ITEMS : per_thread);
  return (int)per_thread * PL;
}
// whether the NHWC kernel takes C channels of `prec`'s storage type: whole 16-byte groups, a power-of-two number of them
bool group_stats_nhwc_ok(int C, int prec) {
  const int cpc = storage_prec(prec) == NQA_PREC_F32 ? 4 : 8;
  return C >= cpc && C % cpc == 0 && C / cpc <= 256 && 256 % (C / cpc) == 0;
}

template <typename P>
static int launch_group_stats_nhwc(const void *ref, const void *ren, int R, int K, int HW, int C, double *part,
                                   hipStream_t st) {
  const int ppb = group_stats_units_per_block(HW, C, P::ID, R);
  const int nblk = cdiv(HW, ppb);
  TimedLaunch t(NQA_K_STATS, st);
  group_stats_nhwc_kernel<P><<<R * nblk, 256, 0, st>>>(reinterpret_cast<const typename P::T *>(ref),
                                                      reinterpret_cast<const typename P::T *>(ren), K, HW, C, ppb, nblk,
                                                      part);
  return check_launch("group_stats_nhwc");
}

// ref: R maps (HW, C), ren: R * K maps, render (r, k) at r * K + k, both NHWC in prec's storage type
int group_stats_nhwc(const void *ref, const void *ren, int R, int K, int HW, int C, int prec, double *part,
                     hipStream_t st) {
  prec = storage_prec(prec);
  if (!group_stats_nhwc_ok(C, prec) || (long)R * cdiv(HW, group_stats_units_per_block(HW, C, prec, R)) > 0x7fffffffL) {
    set_error("group_stats: no kernel for C=%d (R=%d, HW=%d)", C, R, HW);
    return NQA_E_SHAPE;
  }
  switch (prec) {
    case NQA_PREC_F32: return launch_group_stats_nhwc<PrecF32>(ref, ren, R, K, HW, C, part, st);
    case NQA_PREC_BF16: return launch_group_stats_nhwc<PrecBF16>(ref, ren, R, K, HW, C, part, st);
    case NQA_PREC_F16: return launch_group_stats_nhwc<PrecF16>(ref, ren, R, K, HW, C, part, st);
  }
  set_error("group_stats: unknown prec %d", prec);
  return NQA_E_ARG;
}

int group_stats_nchw(const float *ref, const float *ren, int R, int K, int C, int HW, double *part, hipStream_t st) {
  const int ppb = stats_nchw_ppb(HW);  // at most 4096 = NQA_GROUP_ITEMS * 256
  dim3 grid(R * C, cdiv(HW, ppb));
  TimedLaunch t(NQA_K_STATS, st);
  group_stats_nchw_kernel<<<grid, 256, 0, st>>>(ref, ren, K, C, HW, ppb, part);
  return check_launch("group_stats_nchw");
}

}  // namespace nqa
