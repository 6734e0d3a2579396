// The VGG pyramid as one chain of launches, shared by the DISTS drivers (nqa_api.hip) and the A-DISTS forward
// (nqa_adists.hip).  Host code only.
#pragma once
#include "nqa_common.h"

namespace nqa {

struct PyrDims {
  int h[5], w[5];
};
static PyrDims pyr_dims(int H, int W) {
  PyrDims d;
  d.h[0] = H;
  d.w[0] = W;
  for (int k = 1; k < 5; ++k) {
    d.h[k] = (d.h[k - 1] + 1) / 2;
    d.w[k] = (d.w[k - 1] + 1) / 2;
  }
  return d;
}

// Runs the 13 convs and the four L2-pools on `n` images: images [0,nx) come from x, the rest from
// y (fp32 NCHW).  `prec` is the blob's mode, plain or mixed; every stage runs in its own kernel precision
// stage_prec(prec, k) (mixed: F16 on two-term weights, then F32S behind a pool that writes split16 records), and that
// is the precision on_tap sees its tap in.  Stage 1 is one fused kernel where stage1_is_fused says so, conv1_1 and
// layer 1 otherwise.  Stage k's last conv writes into taps[k] when taps is given, else into the ping-pong pair.
// on_tap(k, tap, Hk, Wk, Ck, pool_dst) is called once that conv is enqueued; pool_dst is where
// the stage's L2-pool output must go (null after stage 5).  It returns 1 if it pooled the tap
// itself (the fused pool+statistics pass), 0 to have the plain L2-pool run, <0 on error.
// fuse_tap(k, in, Hk, Wk, layer, pool_dst): the DISTS path's offer to run stage k's LAST conv, its L2-pool and its
// statistics as one kernel (nqa_conv_pool.hip); it returns 1 if it did, 0 to decline (then the conv, on_tap and the
// pool run as usual), < 0 on error.  Only asked when the batch is x | y pairs (n == 2 * nx) and no taps are wanted.
struct NoFuse {
  int operator()(int, const void *, int, int, int, void *) const { return 0; }
};
// fuse_stage1(pool_dst): the same offer for the whole of stage 1 (nqa_conv1_pool.hip: normalisation, conv1_1, conv1_2,
// L2-pool and the statistics of tap 1 from the raw images); 1 = done, `pool_dst` holds the pooled relu1_2.
struct NoFuse1 {
  int operator()(void *) const { return 0; }
};
template <typename F, typename FU = NoFuse, typename FS = NoFuse1>
static int run_stages(const float *x, const float *y, int nx, void *bufA, void *bufB, int n, int H, int W,
                      const void *packed, int prec, void *const *taps, F on_tap, hipStream_t st, FU fuse_tap = FU(),
                      FS fuse_stage1 = FS()) {
  const PyrDims d = pyr_dims(H, W);
  const bool fused1 = stage1_is_fused(prec, W);
  void *cur = bufA;
  int rc, first_layer = 1;
  if (!taps && n == 2 * nx) {  // stage 1 with its pool and statistics in one kernel: the layer loop starts at conv2_1
    if ((rc = fuse_stage1(bufA)) < 0) return rc;
    if (rc == 1) first_layer = 2;
  }
  if (!fused1 && first_layer == 1) {
    const size_t ybytes = (size_t)nx * H * W * 64 * prec_elem_bytes(stage_prec(prec, 0));
    if ((rc = conv1_1(x, nx, H, W, packed, prec, bufA, st))) return rc;
    if (n > nx && (rc = conv1_1(y, n - nx, H, W, packed, prec, static_cast<char *>(bufA) + ybytes, st))) return rc;
  }
  for (int layer = first_layer; layer < NQA_NUM_CONVS; ++layer) {
    const ConvSpec &cs = kConvs[layer];
    const int k = cs.stage, kp = stage_prec(prec, k);
    void *dst = (cs.last && taps) ? taps[k] : (cur == bufA ? bufB : bufA);
    if (cs.last && k < 4 && !taps && n == 2 * nx && layer > 1) {
      if ((rc = fuse_tap(k, cur, d.h[k], d.w[k], layer, dst)) < 0) return rc;
      if (rc == 1) {  // conv + pool + statistics done: `dst` holds the POOLED map
        cur = dst;
        continue;
      }
    }
    if (layer == 1 && fused1) {
      if ((rc = conv1_fused(x, y, nx, n, H, W, packed, prec, dst, st))) return rc;
    } else if ((rc = conv3x3(cur, n, d.h[k], d.w[k], layer, packed, prec, dst, st))) {
      return rc;
    }
    cur = dst;
    if (cs.last) {
      void *pdst = k < 4 ? ((cur == bufA) ? bufB : bufA) : nullptr;
      if ((rc = on_tap(k, cur, d.h[k], d.w[k], cs.cout, pdst)) < 0) return rc;
      if (k < 4) {
        if (rc == 0) {  // (a 16-bit stage in front of an F32S one: the boundary pool of the mixed modes)
          const bool boundary = kp == NQA_PREC_F16 && stage_prec(prec, k + 1) == NQA_PREC_F32S;
          rc = boundary ? l2pool_to_split16(cur, n, d.h[k], d.w[k], cs.cout, pdst, st)
                        : l2pool(cur, n, d.h[k], d.w[k], cs.cout, kp, pdst, st);
          if (rc) return rc;
        }
        cur = pdst;
      }
    }
  }
  return NQA_OK;
}

}  // namespace nqa
