/*
 * nqa.h -- C ABI of libnqa_hip.so: the DISTS / A-DISTS hot path of kobejean/nerf-qa
 * as hand-written HIP kernels for MI355X (gfx950).
 *
 * The reference has no FFI: its boundary for this path is the Python callable
 * surface of two nn.Modules.  Each entry point below names
 * the reference lines whose arithmetic it replaces; nerf_qa_amd/ (the Python
 * shell that mirrors those modules) is the only intended caller and binds these
 * symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; every pointer marked "dev" is a device pointer owned by
 *     the caller (e.g. a torch tensor's data_ptr()); "host" pointers are host memory;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Kernels
 *     are enqueued on it and the call returns without synchronising;
 *   - return value: 0 on success, a negative NQA_E_* code on failure, with a
 *     message available from nqa_last_error() (thread-local);
 *   - the only mutable state is THREAD-LOCAL (the error string, the timing ring of nqa_timing_*
 *     and the tuning choice of nqa_set_conv_variant) plus idempotent per-device caches (kernel
 *     attributes, CU count), so calls are re-entrant per (thread, stream): one thread's tuning
 *     or timing never changes or observes another thread's launches.
 *   - the Python shell PARSES this file for its signatures and constants (nerf_qa_amd/_lib.py), so declarations stay
 *     plain C: int / long / size_t / double / float and pointers, every parameter named, no structs, no function
 *     pointers, no varargs, no conditional blocks; what the parser does not understand it refuses at import.
 *
 * Layouts
 *   - images enter as the reference's tensors: float32 NCHW, values in [0,1];
 *   - activations inside the pyramid are NHWC in the element type of the chosen
 *     precision (`prec`): NQA_PREC_F32 / NQA_PREC_F32S float, NQA_PREC_BF16 bfloat16,
 *     NQA_PREC_F16 IEEE half.  All accumulation and all statistics are float32/float64;
 *   - in NQA_PREC_F32S the maps BETWEEN conv layers (the outputs of nqa_conv1_1, of the
 *     non-tapped conv layers and of nqa_l2pool) are "split16": per pixel and per group of 16
 *     channels 64 bytes [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15], hi = half(v), lo = half(v - hi),
 *     4 bytes per element like float; the tapped maps (conv layers 1, 3, 6, 9, 12 = relu1_2 ..
 *     relu5_3) are plain float.  nqa_split16_encode / _decode convert;
 *   - VGG weights are handed over once as a packed blob (nqa_pack_vgg_weights).
 *
 * Gradients: the score's dependence on its inputs has two backward families below -- the pyramid backward
 * (DISTS.forward(require_grad=True), nqa_conv3x3_split ... nqa_conv1_1_backward) and the statistics backward onto
 * caller-provided feature maps (forward_from_feats under autograd, nqa_dists_stats_nchw_backward).
 */
#ifndef NQA_H
#define NQA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NQA_VERSION 1

/* NQA_PREC_F32S: float32 activations like NQA_PREC_F32, but conv layers 2..13 multiply on the f16
 * matrix cores with both operands split into (hi, lo) half pairs (3 MFMAs per product block,
 * ~2^-21 relative error per product) -- near-f32 results at a fraction of the f32-MFMA cost.
 *
 * NQA_PREC_F32M ("mixed", a mode of the DISTS pyramid: nqa_pack_vgg_weights, nqa_workspace_bytes, nqa_vgg_pyramid,
 * nqa_dists_forward, and the single operators that run one of its layers on a mixed blob -- nqa_conv1_1, nqa_conv1_fused,
 * nqa_conv3x3_relu, nqa_l2pool, nqa_l2pool_f16_to_split16; the A-DISTS entry points and nqa_nhwc_to_nchw_f32 refuse it):
 * stages 1..3 (conv layers 0..6) keep f16 NHWC activations and multiply them
 * with weights held as f16 (hi, lo) pairs -- TWO MFMAs per product, the weights' 11-bit rounding removed -- and
 * stages 4..5 (layers 7..12) run as NQA_PREC_F32S; the L2-pool after stage 3 turns the f16 tap into split16
 * records.  Taps 1..3 are half, taps 4..5 float.  What is left of the 16-bit error is the activation rounding of the
 * first seven layers, whose contribution to a DISTS score is the smallest of all (tools/cpu_prec_layers.py).
 *
 * NQA_PREC_F32M2: the same with only stages 1..2 (conv layers 0..3) on two-term weights and stages 3..5 as
 * NQA_PREC_F32S (taps 1..2 half, 3..5 float): 2.6 times less of that residual error for ~10 % of the speed.
 * NQA_PREC_F32M4: stages 1..4 (layers 0..9) on two-term weights, stage 5 as NQA_PREC_F32S.  NQA_PREC_F16W: ALL five stages
 * -- f16 activations x two-term weights throughout, no float stage, every tap half: f16 without its weight rounding. */
enum { NQA_PREC_F32 = 0, NQA_PREC_BF16 = 1, NQA_PREC_F16 = 2, NQA_PREC_F32S = 3, NQA_PREC_F32M = 4, NQA_PREC_F32M2 = 5,
       NQA_PREC_F32M4 = 6, NQA_PREC_F16W = 7 };
/* pyramid stages (1-based count) that run with f16 activations + two-term weights in a mixed mode, 0 otherwise */
#define NQA_MIXED_STAGES(prec) \
  ((prec) == NQA_PREC_F32M ? 3 : (prec) == NQA_PREC_F32M2 ? 2 : (prec) == NQA_PREC_F32M4 ? 4 : (prec) == NQA_PREC_F16W ? 5 : 0)

enum {
  NQA_OK = 0,
  NQA_E_ARG = -1,       /* bad argument (null pointer, non-positive size, unknown prec) */
  NQA_E_SHAPE = -2,     /* shape the kernels do not support */
  NQA_E_WORKSPACE = -3, /* workspace too small */
  NQA_E_LAUNCH = -4     /* HIP reported an error when enqueuing */
};

#define NQA_NUM_CONVS 13
#define NQA_NUM_TAPS 6
#define NQA_TOTAL_CHNS 1475 /* 3+64+128+256+512+512, DISTS_pt.py:57 */

int nqa_version(void);
const char *nqa_last_error(void);

/* ---- VGG-16 weights -------------------------------------------------------- */

/* Bytes of the packed weight blob for `prec`. */
size_t nqa_packed_weights_bytes(int prec);

/* Pack the 13 conv3x3 layers (torchvision features[0,2,5,7,10,12,14,17,19,21,24,26,28],
 * sliced into stages at DISTS_pt.py:36-49) from float32 OIHW host arrays into the
 * kernel-native blob (host memory, nqa_packed_weights_bytes(prec) bytes).  The caller
 * then copies the blob to the device once. */
int nqa_pack_vgg_weights(const float *const w_host[NQA_NUM_CONVS], const float *const b_host[NQA_NUM_CONVS],
                         int prec, void *packed_host);

/* ---- single operators (used by forward_once and by the parity tests) ------- */

/* conv1_1 with the input normalisation folded in front: h=(x-mean)/std (DISTS_pt.py:92),
 * zero padding applied to h, conv3x3(3->64)+bias+ReLU (features[0,1]).  x: dev float32
 * NCHW (n,3,H,W); out: dev NHWC (n,H,W,64) in prec's element type (split16 in NQA_PREC_F32S).
 * A mixed mode: the exact float convolution stored as half, the form the pyramid runs where it does not fuse stage 1. */
int nqa_conv1_1(const float *x_nchw, int n, int H, int W, const void *packed_w, int prec, void *out_nhwc,
                void *stream);

/* Stage 1 in one kernel (16-bit modes and NQA_PREC_F32S): conv1_1 as above followed by conv1_2+ReLU
 * (features[0..3], DISTS_pt.py:36-37), the 64-channel intermediate staying in LDS.
 * x: dev float32 NCHW (n,3,H,W); out: dev NHWC (n,H,W,64) = relu1_2 in prec's element type (float in NQA_PREC_F32S, whose
 * products are three-term (hi, lo) splits in both convolutions).  NQA_PREC_F32 has no fused form.
 * A mixed mode: both convolutions on two-term weights, half out (the normalised pixels and relu1_1 are rounded to half);
 * the pyramid takes this form only for W >= 16 with the first-forms bit of nqa_set_conv_variant clear, and so does this
 * call: NQA_E_SHAPE otherwise (run nqa_conv1_1 and nqa_conv3x3_relu(layer 1) then, as the pyramid does). */
int nqa_conv1_fused(const float *x_nchw, int n, int H, int W, const void *packed_w, int prec, void *out_nhwc,
                    void *stream);

/* conv3x3 stride 1 pad 1 + bias + ReLU for VGG layer `layer` (1..12), NHWC in/out
 * (torchvision Conv2d+ReLU pairs, DISTS_pt.py:36-49).  NQA_PREC_F32S: split16 in; float out for
 * the tapped layers (1, 3, 6, 9, 12), split16 out otherwise.  A mixed mode: the layer as the pyramid runs it on the
 * mixed blob -- half in and out on two-term weights where the layer's stage is a 16-bit one (NQA_MIXED_STAGES), the
 * formats and kernels of NQA_PREC_F32S behind it. */
int nqa_conv3x3_relu(const void *in_nhwc, int n, int H, int W, int layer, const void *packed_w, int prec,
                     void *out_nhwc, void *stream);

/* L2pooling.forward, DISTS_pt.py:22-25 (= Downsample, ADISTS.py:28-31):
 * sqrt(depthwise 3x3 Hanning, stride 2, pad 1, of x^2, + 1e-12).  NHWC (n,H,W,C) ->
 * (n,ceil(H/2),ceil(W/2),C).  NQA_PREC_F32S: float in (a tapped map), split16 out.  A mixed mode: the pool between two
 * of its 16-bit stages, i.e. NQA_PREC_F16 (the call has no stage argument; the boundary pool is the next function). */
int nqa_l2pool(const void *in_nhwc, int n, int H, int W, int C, int prec, void *out_nhwc, void *stream);

/* The L2-pool at a mixed mode's boundary, behind its last 16-bit stage: half NHWC (n,H,W,C) in, split16 records
 * (n,ceil(H/2),ceil(W/2),C) out, C a multiple of 16.  The pooled value is formed in float from the half inputs and split
 * as everywhere: hi = half(v), lo = half(v - hi).  Below 2^-14 hi is a subnormal half and lo adds nothing, so such a value
 * is kept to an absolute 2^-25, not to float precision. */
int nqa_l2pool_f16_to_split16(const void *in_nhwc_f16, int n, int H, int W, int C, void *out_split16, void *stream);

/* NHWC (prec element type) -> float32 NCHW, so forward_once can return the
 * reference's tensor format (DISTS_pt.py:103). */
int nqa_nhwc_to_nchw_f32(const void *in_nhwc, int n, int H, int W, int C, int prec, float *out_nchw, void *stream);

/* float32 NHWC (pixels, C) <-> split16 (see Layouts), C a multiple of 16.  Used by the
 * single-operator parity tests in NQA_PREC_F32S; the fused paths never call them. */
int nqa_split16_encode(const float *in_nhwc, long pixels, int C, void *out, void *stream);
int nqa_split16_decode(const void *in, long pixels, int C, float *out_nhwc, void *stream);

/* ---- the fused paths --------------------------------------------------------- */

/* Workspace bytes needed by nqa_vgg_pyramid / nqa_dists_forward for `n_images`
 * images (2*B for a batch of B pairs) of H x W. */
size_t nqa_workspace_bytes(int n_images, int H, int W, int prec);

/* forward_once, DISTS_pt.py:91-103, for n images: runs the 13 convs and 4 L2-pools.
 * taps[k] (k=0..4, dev, may not be null) receives relu{1_2,2_2,3_3,4_3,5_3} as NHWC
 * in prec's element type with shape (n, Hk, Wk, Ck), Hk = ceil(H / 2^k). */
int nqa_vgg_pyramid(const float *x_nchw, int n, int H, int W, const void *packed_w, int prec, void *workspace,
                    size_t workspace_bytes, void *const taps[5], void *stream);

/* DISTS.forward up to the per-channel similarities, DISTS_pt.py:105-141:
 * both pyramids (x and y, B images each, float32 NCHW (B,3,H,W)), then for every
 * (b, stage, channel) S1 = (2 mx my + 1e-6)/(mx^2 + my^2 + 1e-6) and
 * S2 = (2 cov + 1e-6)/(vx + vy + 1e-6).  s1, s2: dev float32 (B, 1475). */
int nqa_dists_forward(const float *x_nchw, const float *y_nchw, int B, int H, int W, const void *packed_w, int prec,
                      void *workspace, size_t workspace_bytes, float *s1, float *s2, void *stream);

/* DISTS of K renders against ONE reference, for R such groups (DISTS_pt.py:105-141 for the R * K pairs; the reference's
 * scoring tables hold several rows per reference_folder, test2_prep.py:89,201,304,404, and score each row with a
 * forward of its own): the reference frames go through the pyramid once per group, not once per render -- R + R * K
 * images where nqa_dists_forward runs 2 * R * K.
 *   ref      dev float32 NCHW (R,3,H,W); renders  dev float32 NCHW (R,K,3,H,W) contiguous, render k of group r at r * K + k.
 *   s1, s2   dev float32 (R * K, 1475), pair p = r * K + k: what nqa_dists_forward writes for (ref[r], renders[r][k]) in
 *            `prec`, up to the order of the fp64 partial sums (another split of the pixels into blocks).
 * Inside, one NHWC batch of n = R + R * K images: the references first, render (r, k) at image R + r * K + k.  Every
 * `prec` of nqa_dists_forward, the mixed modes included.  The statistics are nqa_group_stats.hip's kernels: a block
 * keeps a strip of the reference's tap and walks the group's renders against it, so a tap is read (1 + K) / (2 K) times
 * as often as by the pairwise kernels; one writer per partial sum, no atomics, bitwise repeatable.  The L2-pools run as
 * launches of their own: this path has no fused pool + statistics pass and no fused stage-closing kernel.
 * Workspace: nqa_dists_group_workspace_bytes (0 for arguments the forward refuses).
 * Refused on the host, before any launch: NQA_E_ARG null pointer, non-positive size, more than 65535 pairs in one call
 * (slice over R), unknown prec, a frame of H * W * 64 elements reaching 2^31 bytes (nqa_dists_forward's limit);
 * NQA_E_WORKSPACE a short workspace. */
size_t nqa_dists_group_workspace_bytes(int R, int K, int H, int W, int prec);
int nqa_dists_forward_group(const float *ref, const float *renders, int R, int K, int H, int W, const void *packed_w,
                            int prec, void *workspace, size_t workspace_bytes, float *s1, float *s2, void *stream);

/* ONE map's group statistics and their finalisation on their own, for tests and tools: the launch functions
 * nqa_dists_forward_group enqueues for a tap (DISTS_pt.py:131-141), with the map's channels as the whole vector.
 *   feat     dev, n = R + R * K maps of HW pixels, the R references first, render (r, k) at map R + r * K + k.
 *            nchw = 1: float32 planes (n, C, HW), whatever prec is (the plane kernel, fp64 throughout).
 *            nchw = 0: NHWC (n, HW, C) in prec's storage type (float for NQA_PREC_F32 / NQA_PREC_F32S), 16-byte aligned,
 *            C a power-of-two number of 16-byte channel groups (C = 4 .. 1024 floats, 8 .. 2048 halves).
 *   s1, s2   dev float32 (R * K, C).   scratch: dev, nqa_dists_group_stats_bytes bytes (0 for arguments the call refuses).
 * Refused on the host, before any launch: NQA_E_ARG null pointer, non-positive size, more than 65535 pairs, prec
 * outside the four kernel-level modes, a map of HW * C elements reaching 2^31 bytes; NQA_E_SHAPE an NHWC map whose C the
 * kernel does not take; NQA_E_WORKSPACE a short scratch. */
size_t nqa_dists_group_stats_bytes(int R, int K, int HW, int C, int prec, int nchw);
int nqa_dists_group_stats(const void *feat, int R, int K, int HW, int C, int prec, int nchw, void *scratch,
                          size_t scratch_bytes, float *s1, float *s2, void *stream);

/* The group statistics' five sums and their launch plan, for tests and tools: nqa_dists_group_stats' launch, unchanged
 * (the same arguments, the same scratch, the same refusals under the name dists_group_sums, plus a null sums), and one
 * fold of its per-block fp64 partials in place of the finalisation.
 *   sums     dev double (R * K, C, 5) = {sum x, sum y, sum x^2, sum y^2, sum xy} over the HW stored values of pair
 *            p = r * K + k, per channel; x is reference r, y its render k.
 * nqa_dists_group_stats_grid: out[0..3] = pixels per block, blocks per map, pixels a block takes side by side (256 for
 * planes), the largest number of strip items a thread holds (at most 16), from the launcher's own planning functions.
 * Host-only, touches no device; refuses (NQA_E_ARG / NQA_E_SHAPE) what nqa_dists_group_stats_bytes answers with 0, and a
 * null out. */
int nqa_dists_group_sums(const void *feat, int R, int K, int HW, int C, int prec, int nchw, void *scratch,
                         size_t scratch_bytes, double *sums, void *stream);
int nqa_dists_group_stats_grid(int R, int K, int HW, int C, int prec, int nchw, int out[4]);

/* The PAIR path's two statistics passes on their own, for tests and tools: the launch functions nqa_dists_forward and
 * nqa_adists_forward enqueue for a tapped map, unchanged, and one fold of their per-block fp64 partials.
 *   nqa_pool_stats   L2pooling.forward (DISTS_pt.py:22-25) and the five sums behind DISTS_pt.py:131-139 of ONE tap in one
 *           pass (pool_stats_kernel): what the forwards run on taps 1..4 wherever no conv kernel closes the tap itself.
 *   nqa_pool_stats_f16_to_split16   the same pass behind a mixed mode's last 16-bit stage: half in, split16 records out
 *           (as nqa_l2pool_f16_to_split16), C a multiple of 16.
 *   nqa_stats_nhwc   the sums alone (stats_nhwc_kernel): what the forwards run on the last tap, relu5_3.
 *   feat     dev NHWC, 2B maps (2B, H, W, C) or (2B, HW, C): the B x maps, then the B y maps, in prec's storage type (float
 *            for NQA_PREC_F32 / NQA_PREC_F32S), 16-byte aligned; C a power-of-two number of 16-byte channel groups, at most
 *            256 of them (C = 4 .. 1024 floats, 8 .. 2048 halves; NQA_PREC_F32S writes split16 and needs C % 16 == 0).
 *   pooled   dev (2B, ceil(H/2), ceil(W/2), C) as nqa_l2pool writes it for `prec` (split16 in NQA_PREC_F32S), bit for bit.
 *   sums     dev double (B, C, 5) = {sum x, sum y, sum x^2, sum y^2, sum xy} over the H * W stored values of pair b's maps,
 *            per channel: per-thread shifted float moments, fp64 from the block reduction on (nqa_moments.h).
 *   ws       dev, nqa_pool_stats_workspace_bytes / nqa_stats_nhwc_workspace_bytes bytes (the per-block partials, B * blocks
 *            * C * 5 doubles; 0 for arguments the call refuses; the split16 form takes NQA_PREC_F16's).
 * nqa_pool_stats_grid: out[0..4] = tile rows TR, tile columns TC, tiles across the pooled map, tiles per pair, blocks of
 * the launch, from the launcher's own planning function.  nqa_stats_nhwc_grid: out[0..2] = pixels per block, blocks per
 * pair, pixels a block takes side by side.  Both are host-only and touch no device.
 * Refused on the host, before any launch, with a message naming the function: NQA_E_ARG null pointer, non-positive size,
 * a mixed or unknown prec, more than 65535 pairs, a map of H * W * C elements reaching 2^31 bytes; NQA_E_SHAPE a C the
 * kernels do not take; NQA_E_WORKSPACE a short workspace. */
size_t nqa_pool_stats_workspace_bytes(int B, int H, int W, int C, int prec);
size_t nqa_stats_nhwc_workspace_bytes(int B, int HW, int C, int prec);
int nqa_pool_stats_grid(int B, int H, int W, int C, int prec, int out[5]);
int nqa_stats_nhwc_grid(int B, int HW, int C, int prec, int out[3]);
int nqa_pool_stats(const void *feat, int B, int H, int W, int C, int prec, void *pooled, double *sums, void *ws,
                   size_t ws_bytes, void *stream);
int nqa_pool_stats_f16_to_split16(const void *feat_f16, int B, int H, int W, int C, void *pooled_split16, double *sums,
                                  void *ws, size_t ws_bytes, void *stream);
int nqa_stats_nhwc(const void *feat, int B, int HW, int C, int prec, double *sums, void *ws, size_t ws_bytes,
                   void *stream);

/* The statistics alone on caller-provided float32 NCHW feature lists
 * (forward_from_feats, DISTS_pt.py:181-202).  fx[k], fy[k]: dev (B, C[k], Hk[k], Wk[k]).
 * scratch: dev, nqa_stats_scratch_bytes(B, total pixels...) bytes. */
size_t nqa_stats_scratch_bytes(int B, const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS], const int Wk[NQA_NUM_TAPS]);
int nqa_dists_stats_nchw(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B,
                         const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS], const int Wk[NQA_NUM_TAPS],
                         void *scratch, size_t scratch_bytes, float *s1, float *s2, void *stream);

/* Backward of nqa_dists_stats_nchw: forward_from_feats under autograd (the training loss of the reference's
 * no-reference models, nerf_qa/model_nr_v8.py:258-265).  Given g_s1 = dL/dS1 and g_s2 = dL/dS2 (dev float32 (B, ctot),
 * ctot = sum C[k]), writes gx[k] = dL/dfx[k] and gy[k] = dL/dfy[k] (dev float32 NCHW, the shapes of fx[k]); either of
 * gx[k], gy[k] may be null, and nothing is computed or written for that map.  Per (pair, channel) plane of N pixels:
 *   gx = g1 dS1/dmx / N + 2 g2 dS2/dv / N (x - mx) + g2 dS2/dcov / N (y - my), gy the same with x and y swapped,
 * the coefficients from the forward's fp64 sums and the affine map evaluated in fp64, rounded to float once.
 * fwd_scratch / fwd_bytes: the scratch that the MATCHING nqa_dists_stats_nchw call (same maps, B, C, Hk, Wk) filled,
 * left unchanged since; coef: dev, nqa_stats_backward_bytes(B, C) bytes of per-plane coefficients (overwritten).
 * Two launches, both counted as NQA_K_STATS by the timing ring; no atomics (bitwise repeatable). */
size_t nqa_stats_backward_bytes(int B, const int C[NQA_NUM_TAPS]);
int nqa_dists_stats_nchw_backward(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B,
                                  const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS], const int Wk[NQA_NUM_TAPS],
                                  const void *fwd_scratch, size_t fwd_bytes, const float *g_s1, const float *g_s2,
                                  void *coef, size_t coef_bytes, float *const gx[NQA_NUM_TAPS],
                                  float *const gy[NQA_NUM_TAPS], void *stream);

/* alpha/beta weighted sum -> score, DISTS_pt.py:127-129,135,142,144:
 * w = sum(alpha)+sum(beta); score_b = 1 - sum_c alpha_c/w S1_bc - sum_c beta_c/w S2_bc.
 * alpha, beta: dev float32 (1475).  score: dev float32 (B). */
int nqa_dists_score(const float *s1, const float *s2, const float *alpha, const float *beta, int B, float *score,
                    void *stream);

/* ---- A-DISTS (ADISTS.forward, ADISTS.py:137-197, as_map=False) ------------------ */

size_t nqa_adists_workspace_bytes(int B, int H, int W, int prec);

/* Both pyramids, texture-probability maps from x (compute_prob, ADISTS.py:71-100),
 * entropy channel weights from x (ADISTS.py:127-135,150-161), Gaussian-windowed (21x21,
 * sigma 7, valid) or global T/S statistics per stage (ADISTS.py:165-183) and the
 * weighted combine (ADISTS.py:185-191).  d: dev float32 (B) receives D (the caller
 * returns 1-D or 1-mean(D), ADISTS.py:194-197). */
int nqa_adists_forward(const float *x_nchw, const float *y_nchw, int B, int H, int W, const void *packed_w, int prec,
                       void *workspace, size_t workspace_bytes, float *d, void *stream);

/* The same pass with as_map=True (ADISTS.py:163,188-189,193): additionally map[b] (dev float32
 * (B,H,W)) = 1 - sum over stages of the stage's distortion map resized bilinearly
 * (align_corners=False) to H x W.  The reference's return value broadcasts this to (B,B,H,W)
 * with out[i][j] = map[i] for every j (its (B,H,W) + (B,1,H,W) addition); the Python shell
 * reproduces that shape. */
int nqa_adists_forward_map(const float *x_nchw, const float *y_nchw, int B, int H, int W, const void *packed_w,
                           int prec, void *workspace, size_t workspace_bytes, float *d, float *map, void *stream);

/* A-DISTS and DISTS of the same pairs from ONE pyramid.  nqa_adists_forward already fills, for its channel norms and
 * global-branch moments, the fp64 per-(pair, channel) sums of all six taps -- the very sums nqa_dists_forward folds into
 * S1 / S2, from the same statistics kernels.  This call runs nqa_adists_forward's launches unchanged (d, and map when
 * non-null, are bit-identical to nqa_adists_forward / nqa_adists_forward_map) plus one finalisation launch on those sums
 * (counted as NQA_K_STATS): s1, s2 dev float32 (B,1475) receive what nqa_dists_forward writes for (x, y) in `prec`, up
 * to the order of the fp64 partial sums of taps 1-2 where nqa_dists_forward fuses them into a conv kernel.  Workspace
 * nqa_adists_workspace_bytes(B, H, W, prec); map may be null.  Arguments are checked as in nqa_adists_forward, and s1 /
 * s2 must not be null. */
int nqa_adists_dists_forward(const float *x_nchw, const float *y_nchw, int B, int H, int W, const void *packed_w,
                             int prec, void *workspace, size_t workspace_bytes, float *d, float *s1, float *s2,
                             float *map, void *stream);

/* A-DISTS of K renders against ONE reference, for R such groups (ADISTS.forward, ADISTS.py:137-197, for the R * K pairs;
 * the reference's scoring loops pass x = ref, prep.py:186, and its tables hold several rows per reference_folder,
 * test2_prep.py:89,201,304,404).  A-DISTS is asymmetric: the texture-probability chain (compute_prob, ADISTS.py:71-100),
 * the entropy channel weights (:127-135,150-161) and gamma come from x alone, so here they are computed once per
 * reference, not once per render, and the reference frames go through the pyramid once per group -- R + R * K images
 * where nqa_adists_forward runs 2 * R * K.
 *   ref      dev float32 NCHW (R,3,H,W); renders  dev float32 NCHW (R,K,3,H,W) contiguous, render k of group r at r * K + k
 *            (the layout and pair index p = r * K + k of nqa_dists_forward_group).
 *   d        dev float32 (R * K): what nqa_adists_forward writes for (ref[r], renders[r][k]) in `prec`, up to the order
 *            of the fp64 partial sums of the statistics (the group statistics kernels split the pixels into other blocks)
 *            and of the entropy sums.
 *   s1, s2   both null, or both dev float32 (R * K, 1475): what nqa_adists_dists_forward writes, by the same
 *            finalisation launch on the same partial sums.
 * Inside, one NHWC batch of n = R + R * K images: the references first, render (r, k) at image R + r * K + k, all five
 * taps kept.  The statistics are nqa_group_stats.hip's kernels and the L2-pools run as launches of their own, as in
 * nqa_dists_forward_group; the NHWC4 conversion, the six entropy passes, their fold and the weights kernel run on the R
 * references; the window pass runs per pair in the group instances of its kernels (pair p reads x and the channel
 * weights of reference p / K, writes tw / sw of its own, and the k = 0 pair writes the reference's gamma; a pair's
 * arithmetic is the pairwise kernel's); the probability chain runs per reference, and chain_final_group_kernel takes
 * the K renders' sums against each reference's ps_prod.  No atomics on any sum: bitwise repeatable.
 * Every `prec` nqa_adists_forward takes; the mixed modes are refused as there.  There is no as_map form.
 * Workspace: nqa_adists_group_workspace_bytes (0 for arguments the forward refuses).
 * Refused on the host, before any launch: NQA_E_ARG null pointer (s1 / s2 excepted), only one of s1 / s2 given,
 * non-positive size, more than 65535 pairs in one call (slice over R), unknown or mixed prec, a frame of H * W * 64
 * elements reaching 2^31 bytes (nqa_adists_forward's limit); NQA_E_WORKSPACE a short workspace. */
size_t nqa_adists_group_workspace_bytes(int R, int K, int H, int W, int prec);
int nqa_adists_forward_group(const float *ref, const float *renders, int R, int K, int H, int W,
                             const void *packed_w, int prec, void *workspace, size_t workspace_bytes,
                             float *d, float *s1, float *s2, void *stream);

/* The window pass and the back part of nqa_adists_forward_group on their own, for tests and tools, through the launch
 * functions the group forward uses (the pairwise forward's own, told the group size).
 *   nqa_adists_window_stage_group   nqa_adists_window_stage for R * K pairs: fx the R references' maps, fy the R * K
 *           renders' (pair r * K + k), q [8][R*K][C] per pair, wgt [R][C] per reference; gamma (R, H-20, W-20) per
 *           reference, tw / sw (R*K, H-20, W-20) per pair (the global branch: R and R * K values).  Dispatch, strip and
 *           refusals as nqa_adists_window_stage, with R <= 0, K <= 0 or more than 65535 pairs NQA_E_ARG.
 *   nqa_adists_chain_group          nqa_adists_chain for R * K pairs: gamma[k] and ps_prod[k] (R, mh[k], mw[k]), tw[k] and
 *           sw[k] (R*K, mh[k], mw[k]), d (R*K).  No map.  Workspace nqa_adists_chain_group_bytes(R, K, H, W) (0 for
 *           sizes it refuses); refusals as nqa_adists_chain plus the group's. */
int nqa_adists_window_stage_group(const void *fx, const void *fy, int R, int K, int H, int W, int C, int prec,
                                  const float *q, const float *wgt, int strip, float *gamma, float *tw, float *sw,
                                  void *stream);
size_t nqa_adists_chain_group_bytes(int R, int K, int H, int W);
int nqa_adists_chain_group(const float *const *gamma, const float *const *tw, const float *const *sw, int R, int K, int H,
                           int W, void *workspace, size_t workspace_bytes, float *const *ps_prod, float *d, void *stream);

/* ONE stage of nqa_adists_forward's heavy pass on its own, for tests and tools: the launch that turns a tap pair into
 * the stage's three channel-reduced maps, exactly as nqa_adists_forward enqueues it (the same launch functions, with the
 * stage's channels as the whole channel vector: ctot = C, offset 0).  No workspace.
 *   fx, fy  C == 3: dev float32 NCHW planes (B,3,H,W), whatever prec is.  C in {64,128,256,512}: dev NHWC taps
 *           (B,H,W,C) in prec's storage type (float for NQA_PREC_F32 / NQA_PREC_F32S).
 *   q       dev float32 [8][B][C], rows as the forward's preparation kernel writes them: 0 inv_x, 1 inv_y
 *           (1 / max(||f||_2, 1e-12) of the raw maps), 2 unused here, 3..7 mean_x mean_y var_x var_y cov of the raw maps
 *           (population), read by the global branch only.
 *   wgt     dev float32 [B][C] channel weights.
 *   gamma, tw, sw   dev float32 (B, H-20, W-20): gamma = mean_c (E[x^2] - E[x]^2) / (E[x] + 1e-12) of the RAW x maps
 *           under the 21 x 21 window (ADISTS.py:84-86), tw = sum_c w_c T_c, sw = sum_c w_c S_c of the normalised maps
 *           (ADISTS.py:165-183).  H < 21 or W < 21: the global branch (ADISTS.py:91-97,176-180) from q rows 3..7, B values
 *           per map.
 * Dispatch: C == 3 the planar kernel; float taps the LDS kernel, or the first form when the calling thread's
 * nqa_set_conv_variant bit 3 is set; 16-bit taps the first form.
 *   strip   0: the launcher's own strip height.  1 <= strip <= H-20: that many output rows per block of the LDS kernel
 *           (more than 64 makes a block flush its rows in groups of 64); ignored where no LDS kernel runs.  The launcher
 *           itself never goes past 256 rows; taller forced strips are allowed (nothing in the kernel is sized by the
 *           strip) but the tests force at most 150.
 * Refused on the host, before any launch: NQA_E_ARG null pointer, non-positive size, prec outside the four kernel-level
 * modes, strip < 0 or > H-20; NQA_E_SHAPE any other C, or H * W * C elements of the tap's type reaching 2^31 bytes (the
 * kernels' in-image byte offsets are 32-bit; nqa_adists_forward refuses its own form of this limit, on the frame, with
 * NQA_E_ARG -- the two codes differ).
 * nqa_adists_window_grid: the LDS kernel's grid for the same arguments and the calling thread's variant, grid[0..2] =
 * column groups, row strips, strip height (from the launcher's own function); zeros where no LDS kernel would run.
 * The same refusals. */
int nqa_adists_window_stage(const void *fx, const void *fy, int B, int H, int W, int C, int prec, const float *q,
                            const float *wgt, int strip, float *gamma, float *tw, float *sw, void *stream);
int nqa_adists_window_grid(int B, int H, int W, int C, int prec, int strip, int *grid);

/* The BACK part of nqa_adists_forward on its own, for tests and tools: from the six stages' gamma / tw / sw maps (what
 * the window pass leaves) to the texture-probability chain (compute_prob, ADISTS.py:77-99, coarse to fine), the stages'
 * D sums, D_b (ADISTS.py:185-191) and, with a map pointer, the as_map=True resampler (ADISTS.py:163,188-189,193).  It is
 * the launch function nqa_adists_forward itself ends with: the same kernels on the same grids in the same order.
 *   nqa_adists_chain_dims   mh[k] x mw[k], k = 0..5, of stage k's maps for an H x W frame: the tap is H x W for k = 0
 *           and 1 and halves (rounding up) from k = 2 on; a tap of at least 21 x 21 gives a (h-20) x (w-20) map of valid
 *           windows, a smaller one the global branch's 1 x 1.  Returns the number of windowed stages (they are stages
 *           0 .. n-1; a 21-wide tap is windowed with a 1 x 1 map), or a negative code.
 *   nqa_adists_chain_bytes  workspace of nqa_adists_chain: the chain's accumulators (6 B), its per-block partial sums and
 *           the B ones the coarsest stage is multiplied with.  0 for a non-positive size.
 *   gamma, tw, sw   host arrays of six dev float32 pointers, map k (B, mh[k], mw[k]) contiguous.
 *   ps_prod         host array of six dev float32 pointers, (B, mh[k], mw[k]): receives stage k's probability map.
 *   d               dev float32 (B): D_b = sum_k mean_hw((1 - ps_prod_k) tw_k + ps_prod_k sw_k).
 *   map             null, or dev float32 (B,H,W) as nqa_adists_forward_map writes it.
 * A windowed stage of ONE element has no unbiased standard deviation: its ps_prod, every finer stage's, d and the map
 * are NaN, as the reference's torch.std makes them.
 * Refused on the host, before any launch: NQA_E_ARG null pointer (map excepted; the six pointers of every array
 * included), non-positive size, a frame of H * W * 64 floats reaching 2^31 bytes (nqa_adists_forward's limit);
 * NQA_E_WORKSPACE a workspace under nqa_adists_chain_bytes(B, H, W). */
int nqa_adists_chain_dims(int H, int W, int *mh, int *mw);
size_t nqa_adists_chain_bytes(int B, int H, int W);
int nqa_adists_chain(const float *const *gamma, const float *const *tw, const float *const *sw, int B, int H, int W,
                     void *workspace, size_t workspace_bytes, float *const *ps_prod, float *d, float *map, void *stream);

/* ---- A-DISTS with a window size other than 21 (ADISTS(window_size=n), ADISTS.py:36,66-69) ----
 * Every A-DISTS entry point above whose result depends on the window has a form with an explicit `int window` behind
 * `W`; there is no hidden state.  The old names are the window-21 calls of these.  window: 3 .. 63, odd or even; the
 * taps are those of the reference's gaussian(window, window / 3) -- float32 of exp, a float32-rounded sum, float32
 * quotients, centre window / 2, so an even window is not symmetric -- built on the host and handed to the kernels as a
 * table.  A stage whose tap is at least window x window gives (h-window+1) x (w-window+1) maps of valid windows, a
 * smaller one the global branch's 1 x 1, unchanged.
 * Dispatch of the window pass: window == 21 runs the three specialised kernels exactly as the old names do; every other
 * window runs the generic kernels (nqa_window_n.h: ring of horizontal sums in LDS, one wave per block), NHWC taps with C
 * a multiple of 64 in float / f16 / bf16 storage, planes for C == 3, pair and group forms.  nqa_set_conv_variant + 2048
 * makes window 21 run the generic kernels too (tests and tools compare the two with it).
 *   strip   of the generic kernels: 0 the launcher's own height, 1 <= strip <= H-window+1 that many output rows per
 *           block (more than 64 are flushed in groups of 64), for planes as well.
 * The upper end is the ring's: 1280 * window bytes of LDS per wave, two waves per 160-KiB CU.
 * Refusals are those of the old names, plus NQA_E_ARG "window <n> outside [3, 63]"; the functions that return a size
 * return 0 and set the same message.  The front part (nqa_adists_front) does not depend on the window. */
size_t nqa_adists_workspace_bytes_n(int B, int H, int W, int window, int prec);
int nqa_adists_forward_n(const float *x_nchw, const float *y_nchw, int B, int H, int W, int window, const void *packed_w,
                         int prec, void *workspace, size_t workspace_bytes, float *d, void *stream);
int nqa_adists_forward_map_n(const float *x_nchw, const float *y_nchw, int B, int H, int W, int window,
                             const void *packed_w, int prec, void *workspace, size_t workspace_bytes, float *d,
                             float *map, void *stream);
int nqa_adists_dists_forward_n(const float *x_nchw, const float *y_nchw, int B, int H, int W, int window,
                               const void *packed_w, int prec, void *workspace, size_t workspace_bytes, float *d,
                               float *s1, float *s2, float *map, void *stream);
size_t nqa_adists_group_workspace_bytes_n(int R, int K, int H, int W, int window, int prec);
int nqa_adists_forward_group_n(const float *ref, const float *renders, int R, int K, int H, int W, int window,
                               const void *packed_w, int prec, void *workspace, size_t workspace_bytes, float *d,
                               float *s1, float *s2, void *stream);
int nqa_adists_window_stage_n(const void *fx, const void *fy, int B, int H, int W, int window, int C, int prec,
                              const float *q, const float *wgt, int strip, float *gamma, float *tw, float *sw,
                              void *stream);
int nqa_adists_window_stage_group_n(const void *fx, const void *fy, int R, int K, int H, int W, int window, int C,
                                    int prec, const float *q, const float *wgt, int strip, float *gamma, float *tw,
                                    float *sw, void *stream);
int nqa_adists_chain_dims_n(int H, int W, int window, int *mh, int *mw);
size_t nqa_adists_chain_bytes_n(int B, int H, int W, int window);
int nqa_adists_chain_n(const float *const *gamma, const float *const *tw, const float *const *sw, int B, int H, int W,
                       int window, void *workspace, size_t workspace_bytes, float *const *ps_prod, float *d, float *map,
                       void *stream);
size_t nqa_adists_chain_group_bytes_n(int R, int K, int H, int W, int window);
int nqa_adists_chain_group_n(const float *const *gamma, const float *const *tw, const float *const *sw, int R, int K,
                             int H, int W, int window, void *workspace, size_t workspace_bytes, float *const *ps_prod,
                             float *d, void *stream);

/* The FRONT part of nqa_adists_forward on its own, for tests and tools: from the two images and the five tapped maps to
 * the per-channel scalars q and the channel weights wgt that the window pass and the global branch read.  It runs what
 * nqa_adists_forward runs for them, through the same launch functions, on the same grids, in the same order: the
 * statistics sums (the plane kernel on the images, the fused pool + statistics pass on taps 1..4 -- its pooled maps go to
 * the workspace and are discarded -- and the NHWC kernel on tap 5; the forward enqueues these between the layers of its
 * pyramid), then the preparation kernel, the x images as NHWC4, the six entropy passes, their fold and the weights kernel
 * (ADISTS.py:127-135,150-161,166-167,176-180); the last five steps are one launch function shared with the forward.
 *   x, y    dev float32 NCHW (B,3,Hk[0],Wk[0]).
 *   taps    host array of five dev pointers, tap k = 1..5 at taps[k-1]: NHWC (2B,Hk[k],Wk[k],C_k), images x then y, in
 *           prec's storage type (float for NQA_PREC_F32 / NQA_PREC_F32S); C_k = 64, 128, 256, 512, 512.
 *   Hk, Wk  host int[6]: the sizes of the image (k = 0) and of every tap, free as in nqa_dists_stats_nchw: nothing here
 *           needs one tap to be half the previous one.
 *   q       dev float32 [8][B][1475] as the forward leaves it before the window pass: rows 0, 1 inv_x, inv_y =
 *           1 / max(||f||_2, 1e-12) of the raw maps; rows 3..7 mean_x mean_y var_x var_y cov of the raw maps (population);
 *           row 2 is NOT sum_x any more but hsum, the folded per-channel entropy of the x maps: the forward reuses the
 *           sum_x row for it once the entropy passes have read it.
 *   wgt     dev float32 [B][1475], the channel weights.
 * Contract: the maps are taken as NON-NEGATIVE (images in [0,1], taps behind a ReLU).  The entropy normalises relu(f)
 * with 1 / ||f|| and sum(f) of the raw map, where the reference takes both of relu(f); the two agree on such maps only.
 * nqa_adists_front_bytes: the workspace (0 for arguments nqa_adists_front refuses).  nqa_adists_front_grid: grid[4 k ..
 * 4 k + 3] for k = 0..5 = blocks per image pair of tap k's statistics pass, the pool pass' tile rows TR and columns TC
 * (0, 0 for k = 0 and 5), blocks per image of its entropy pass -- from the planning functions the launches use.
 * Refused on the host, before any launch: NQA_E_ARG null pointer (each of the five tap pointers included), non-positive
 * size, prec outside the four kernel-level modes, a tap of H * W * C elements (the image: H * W * 4 floats) reaching 2^31
 * bytes; NQA_E_WORKSPACE a workspace under nqa_adists_front_bytes. */
size_t nqa_adists_front_bytes(int B, const int *Hk, const int *Wk, int prec);
int nqa_adists_front_grid(int B, const int *Hk, const int *Wk, int prec, int *grid);
int nqa_adists_front(const float *x_nchw, const float *y_nchw, const void *const *taps, int B, const int *Hk,
                     const int *Wk, int prec, void *workspace, size_t workspace_bytes, float *q, float *wgt, void *stream);

/* ---- input preparation on the device (decoded uint8 frame -> metric input) ------------ */

/* transforms.ToTensor / `torch.from_numpy(frame).permute(2,0,1).float() / 255.0` (prep.py:89,
 * data.py:80): in dev uint8 (n,H,W,3) -> out dev float32 (n,3,H,W).  pil_roundtrip != 0 also
 * applies prep.py:90-91's ToPILImage -> ToTensor round trip (mul(255).byte() truncates). */
int nqa_u8hwc_to_f32nchw(const uint8_t *in, int n, int H, int W, int pil_roundtrip, float *out, void *stream);

/* F.interpolate(x, size=(Hout,Wout), mode='bilinear', align_corners=False) (prep.py:93-95,
 * data.py:81-82, test2_prep.py:437) on `planes` = n*C float32 planes of Hin x Win. */
int nqa_resize_bilinear_f32(const float *in, int planes, int Hin, int Win, int Hout, int Wout, float *out,
                            void *stream);

/* The two steps above fused (uint8 (n,Hin,Win,3) -> float32 (n,3,Hout,Wout)), bit-identical to
 * running them back to back; reads only the taps it needs. */
int nqa_u8_resize_bilinear_f32(const uint8_t *in, int n, int Hin, int Win, int Hout, int Wout, float *out,
                               void *stream);

/* transforms.functional.resize on a PIL image (DISTS_pt.py:213-215, test2_prep.py:112,225) =
 * PIL Image.resize((Wout,Hout), BILINEAR): Pillow's antialiased two-pass 8-bit resampler,
 * bit-exact.  in dev uint8 (n,Hin,Win,3) -> out dev uint8 (n,Hout,Wout,3). */
size_t nqa_resize_pil_workspace_bytes(int n, int Hin, int Win, int Hout, int Wout);
int nqa_resize_pil_bilinear_u8(const uint8_t *in, int n, int Hin, int Win, int Hout, int Wout, void *workspace,
                               size_t workspace_bytes, uint8_t *out, void *stream);

/* ---- score-map targets of the no-reference dataset prep (nerf_nr_qa_prep_4.py:71-133) -- */

/* From the K A-DISTS distortion maps of a frame's K renders to the K score-map images and the 2K + 4 logged extrema,
 * for F frames: v = double(max(map, 1e-10f)) (NaN stays NaN); per pixel mean = (sum_k v) / K, k ascending, and the
 * unbiased std = sqrt(sum_k (v - mean)^2 / (K - 1)) (K = 1: NaN, as torch.std); min and max per map and of the std and
 * mean maps, NaN propagating as amin / amax; byte = trunc(255 * (log_max - (-log10 q)) / (log_max - log_min)) where
 * the spread is > 0, else 0, and 0 for a quotient that is not finite.  The per-pixel -log10 and the one that forms
 * log_max / log_min are one device function.
 *   maps  dev float32 (F, K, H, W): frame f's K maps as nqa_adists_forward_map writes them for K pairs.
 *   rgb   dev uint8 (F, K, H, W, 3): HWC, channels (mean, map k, std).
 *   logs  dev double (F, 2K + 4): K x log_max_k = -log10(min of map k), K x log_min_k = -log10(max of map k), then
 *         std_max, std_min, mean_max, mean_min, formed the same way from the std and mean maps.
 * Three launches (NQA_K_PREP), no atomics, fixed fold order: bitwise repeatable.  The workspace
 * (nqa_score_maps_workspace_bytes; 0 for sizes the call refuses) holds the fp64 mean and std maps and the per-block
 * partials; nothing in it is read before it is written.
 * Refused on the host, before any launch: NQA_E_ARG null pointer, non-positive size, K > 256, F * K > 65535,
 * F * K * H * W * 3 reaching 2^31; NQA_E_WORKSPACE a short workspace. */
size_t nqa_score_maps_workspace_bytes(int F, int K, int H, int W);
int nqa_score_maps(const float *maps, int F, int K, int H, int W, void *workspace, size_t workspace_bytes,
                   uint8_t *rgb, double *logs, void *stream);

/* ---- tuning hook ------------------------------------------------------------------ */

/* The stage-closing conv of the DISTS path fused with what consumes its tap (nqa_conv_pool.hip; replaces
 * nerf_qa/DISTS_pytorch/DISTS_pt.py:94 `stage2` conv2_2 + ReLU, :22-25 the L2pooling in front of stage 3, and the
 * sums behind :130-142 for tap relu2_2): the tap is never written.  `in`: dev NHWC batch of 2B images of `layer`'s input
 * (x images [0,B), y images [B,2B)), 16-bit activations of `prec`'s stage; pooled: dev (2B, ceil(H/2), ceil(W/2), Cout)
 * in the next stage's input format; sums: dev double (B, Cout, 5) = {sum x, sum y, sum x^2, sum y^2, sum xy} over the
 * H*W pixels of the (rounded) tap, per pair and channel.  Only layer 3 (conv2_2) in NQA_PREC_F16 and the mixed modes
 * whose stage 3 stays 16-bit has a fused form so far: anything else returns NQA_E_SHAPE.  nqa_dists_forward takes this
 * path by itself (nqa_set_conv_variant + 64 turns it off); these two entry points exist for tests and tools. */
size_t nqa_conv_pool_workspace_bytes(int B, int H, int W, int layer);

/* Which tapped maps nqa_dists_forward(B, H, W, prec) closes inside their conv kernel (pool + statistics fused, the
 * full-resolution map never written): fused[k] = 1 for tap k (1..5; fused[0] is the image, always 0).  Depends on the
 * shape, the mode and the calling thread's nqa_set_conv_variant bits 64 / 128.  bench.py prices its HBM roofline
 * (the pool_stats passes that remain) with it. */
int nqa_dists_fused_taps(int B, int H, int W, int prec, int fused[6]);
/* The same for the WHOLE of stage 1 (nqa_conv1_pool.hip; DISTS_pt.py:92-94 normalisation + conv1_1 + conv1_2, the L2pooling
 * in front of stage 2 and tap relu1_2's sums) from the raw frames: x, y dev float32 NCHW (B,3,H,W); pooled: dev NHWC f16
 * (2B, ceil(H/2), ceil(W/2), 64), x images first; sums: dev double (B, 64, 5); workspace nqa_conv_pool_workspace_bytes(B, H,
 * W, 1).  NQA_PREC_F16 only so far (NQA_E_SHAPE otherwise).  The sums and the pool take relu1_2 rounded to f16, the values
 * the unfused kernels store and read back. */
int nqa_conv1_pool_stats(const float *x, const float *y, int B, int H, int W, const void *packed, int prec, void *pooled,
                         double *sums, void *ws, size_t ws_bytes, void *stream);
int nqa_conv_pool_stats(const void *in, int B, int H, int W, int layer, const void *packed, int prec, void *pooled,
                        double *sums, void *ws, size_t ws_bytes, void *stream);

/* Block-tile choice of the implicit-GEMM conv: 0 = 4-wave tiles (128 ch x 128 px) on every
 * layer, 1 (default) = + 8-wave 256 ch x 256 px tiles on layers with >= 256 output channels, 2 =
 * + 8-wave 128 ch x 512 px tiles wherever the map is large enough (measured equal to 1).
 * Adding 4 selects the tile form of the fused stage-1 kernel; adding 16 selects the round-1 forms of stage 1 (the
 * persistent two-phase kernel) and of conv2_1 (the implicit GEMM) instead of the register-resident-weights kernels, and
 * in NQA_PREC_F32S the round-2 pair of stage-1 kernels (VALU conv1_1 + implicit-GEMM conv1_2) instead of the fused one,
 * adding 32 the implicit GEMM for conv2_2 / conv3_1; adding 64 runs the DISTS path's tap 2 UNFUSED (conv2_2, then the
 * pool + statistics pass over the tap it wrote) instead of conv + L2-pool + statistics in one kernel (nqa_conv_pool.hip);
 * adding 128 does the same for stage 1 (conv1_regw_kernel + pool_stats_kernel instead of nqa_conv1_pool.hip's kernel);
 * adding 8 selects the first form of the A-DISTS window pass (every wave loads its own taps instead of sharing them
 * through LDS); adding 2048 runs a 21-tap A-DISTS window on the generic window kernels (nqa_window_n.h) instead of the
 * specialised ones; adding 4096 does the same for a window of 21 on the _n window-moments and stage-backward entry points
 * (nqa_window_moments_forward_n ...; nqa_window_moments_n.hip; the bit counts on top of a non-zero variant, e.g. 1 + 4096:
 * 4096 on its own is refused as it always was).  Bits 8-9 choose the implicit GEMM's grid on maps whose last 32-wide tile column is at most half full
 * (1 <= W % 32 <= 16): by default such a layer takes ONE launch of 32-wide tiles plus 16-wide tiles down the right edge
 * (conv3x3_igemm_mixed_kernel) wherever that needs fewer rounds of blocks over the chip than the plain grid of 32-wide
 * tiles; adding 256 keeps the plain grid everywhere (A/B runs), adding 512 takes the mixed grid on every such map
 * whatever the block count (so tests reach it at small sizes); 256 + 512 is refused.  The two grids are bit-identical.
 * nqa_set_conv_variant(1024) is a query: it changes nothing and returns how many mixed grids the calling thread has
 * launched since it last asked (>= 0).  Results agree in every variant to the rounding of a different summation order inside a layer (the
 * tile variants are bit-identical); this only exists so they can be timed against each other in one process.
 * The choice is thread-local (it applies to the calling thread's later calls only). */
int nqa_set_conv_variant(int variant);

/* ---- per-kernel timing (bench.py's roofline leg) -------------------------------- */

/* When enabled, every launch of the conv / pool / stats kernels is bracketed by a
 * pair of hipEvents recorded on the launch stream.  nqa_timing_collect synchronises
 * those events and returns, per kernel class, the number of launches and the summed
 * device time in milliseconds, then clears the ring.  Thread-local: only the enabling thread's
 * launches are bracketed, and it collects only its own. */
enum { NQA_K_CONV1 = 0, NQA_K_CONV = 1, NQA_K_POOL = 2, NQA_K_STATS = 3, NQA_K_ADISTS = 4, NQA_K_PREP = 5, NQA_K_SEAM = 6,
       NQA_K_COUNT = 7 };  /* NQA_K_CONV holds the fused conv + pool + statistics kernels too; NQA_K_SEAM their seam pass */
int nqa_timing_enable(int on);
int nqa_timing_collect(int launches[NQA_K_COUNT], double ms[NQA_K_COUNT]);

/* ---- backward pass of the DISTS pyramid: DISTS.forward(x, y, require_grad=True), nerf_qa/DISTS_pytorch/DISTS_pt.py:105-108
 * (the reference runs forward_once WITH autograd there).  nerf_qa_amd/autograd.py drives these per layer; float
 * precision throughout (three-term split products).  Not on the scoring hot path.
 *   nqa_pack_conv_split      one 3x3 layer (float32 OIHW host array; cout % 64 == 0, cin % 16 == 0) in the NQA_PREC_F32S row
 *                            format, zero bias -- e.g. a layer's flipped, transposed weights for its data gradient;
 *   nqa_conv3x3_split        that layer: split16 NHWC in, FLOAT NHWC out, ReLU optional;
 *   nqa_relu_mask_split16    g * (act > 0) as split16 records (act: a float tapped map, or split16);
 *   nqa_l2pool_backward      g_tap += d(L2-pool)/d(tap) applied to g_pooled (DISTS_pt.py:22-25); pooled_split16 is accepted and NOT read -- the
 *                            pooled value is formed from the tap in float (split16 loses it below 2^-14);
 *   nqa_conv1_1_backward     g * (relu1_1 > 0) (float NHWC, 64 channels) -> gradient of the RAW image, float NCHW (n,3,H,W),
 *                            the (x - mean) / std of DISTS_pt.py:92 included; w = conv1_1's float32 OIHW weights on the device. */
size_t nqa_packed_conv_split_bytes(int cout, int cin);
int nqa_pack_conv_split(const float *w_oihw, int cout, int cin, void *packed_host);
int nqa_conv3x3_split(const void *in_split16, int n, int H, int W, int cin, int cout, const void *packed_conv, int relu,
                      float *out_nhwc, void *stream);
int nqa_relu_mask_split16(const float *g_nhwc, const void *act_nhwc, int act_is_split16, long pixels, int C,
                          void *out_split16, void *stream);
int nqa_l2pool_backward(const float *tap_nhwc, const void *pooled_split16, const float *g_pooled_nhwc, int n, int H, int W,
                        int C, float *g_tap_nhwc, void *stream);
int nqa_conv1_1_backward(const float *gm_nhwc, const float *w_oihw_dev, int n, int H, int W, float *g_image_nchw,
                         void *stream);

/* ---- DISTS as a loss: the same backward enqueued without one device -> host read (nerf_qa_amd/autograd.py,
 * pyramid_backward_device / dists_backward).  The chain above is linear in the gradient, and its split16 operands have a
 * half's range, so the gradient is renormalised by an exact power of two before every layer; here the exponents live
 * in device memory, PER IMAGE, so the images of a batch never influence one another.
 *
 *   nqa_dists_stats_nhwc_backward   the statistics' gradient on the pyramid's own layout: tx, ty dev float NHWC
 *       (B, H, W, C) taps of the two images, g_s1 / g_s2 dev float, pair b's C values at g + b * g_stride (e.g. the
 *       tap's columns of the (B, 1475) upstream: g_stride 1475).  Writes gx = dL/dtx and gy = dL/dty (either may be null:
 *       nothing is computed for it), each times the tap's own ReLU mask (t > 0).  The arithmetic contract of
 *       nqa_dists_stats_nchw_backward: fp64 sums and coefficients, the affine map centred and combined in fp64, rounded to
 *       float once, one writer per element, no atomics.  C a power of two in 16..1024, maps 16-byte aligned, H * W <= 2^30.
 *       Three launches, counted as NQA_K_STATS.
 *   nqa_grad_exponent               k[i] = the exponent with max|g_i| * 2^k[i] in [128, 256) for image i of g (n images of
 *       per_image floats each, per_image % 4 == 0), 0 where that maximum is 0 or not finite; k_total[i] += k[i] when
 *       k_total is not null.  Two launches (NQA_K_POOL).
 *   nqa_relu_mask_split16_scaled    nqa_relu_mask_split16 of g * 2^k[image];
 *   nqa_l2pool_backward_scaled      out = g_tap * 2^k_total[image] + d(L2-pool)/d(tap) applied to g_pooled (g_tap: the tap's
 *       own gradient, brought into the chain's running scale; out may be g_tap);
 *   nqa_conv1_1_backward_scaled     nqa_conv1_1_backward of g * 2^k[image] * (relu1_1 > 0), times 2^-k_total[image];
 *       relu1_1_split16: nqa_conv1_1's NQA_PREC_F32S output, or null for no mask.
 * Power-of-two scaling is exact: each scaled form equals its plain form on operands scaled beforehand, bit for bit. */
size_t nqa_dists_stats_nhwc_backward_bytes(int B, int H, int W, int C);
int nqa_dists_stats_nhwc_backward(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C, const float *g_s1,
                                  const float *g_s2, long g_stride, void *workspace, size_t workspace_bytes, float *gx_nhwc,
                                  float *gy_nhwc, void *stream);
size_t nqa_grad_exponent_bytes(int n, long per_image);
int nqa_grad_exponent(const float *g, int n, long per_image, void *workspace, size_t workspace_bytes, int *k, int *k_total,
                      void *stream);
int nqa_relu_mask_split16_scaled(const float *g_nhwc, const void *act_nhwc, int act_is_split16, int n,
                                 long pixels_per_image, int C, const int *k, void *out_split16, void *stream);
int nqa_l2pool_backward_scaled(const float *tap_nhwc, const float *g_pooled_nhwc, const float *g_tap_nhwc, const int *k_total,
                               int n, int H, int W, int C, float *out_nhwc, void *stream);
int nqa_conv1_1_backward_scaled(const float *g_nhwc, const void *relu1_1_split16, const float *w_oihw_dev, const int *k,
                                const int *k_total, int n, int H, int W, float *g_image_nchw, void *stream);

/* ---- The same chain on HALF gradient maps: the loss path's second rung (grad_precision="f16" of DISTS / ADISTS,
 * nerf_qa_amd/autograd.py, pyramid_backward_device).  The forward of a step, its values and its ReLU masks are untouched;
 * the gradient between layers is a plain f16 NHWC map (2 bytes per element) instead of split16 records, the weights are
 * halves, and a data-gradient convolution is ONE f16 MFMA per product with a float32 accumulator.  The per-image
 * exponents put max|g| * 2^k in [8, 16), four octaves below the split16 chain's window, because a convolution's OUTPUT
 * is a half here: |out| <= 16 * (largest L1 norm of a data-gradient filter) has to stay below 65504.
 *
 *   nqa_pack_conv_half               one 3x3 layer (float32 OIHW host array; cout % 64 == 0, cin % 32 == 0) as f16 rows,
 *       each weight rounded to nearest even, zero bias: nqa_packed_conv_half_bytes = the rows (cout * cin * 9 * 2 bytes,
 *       rounded up to 256) + the bias section ((cout + 1) * 4 bytes, rounded up to 256); 0 for a shape it refuses.  Rows
 *       as in the packed blob's 16-bit layers: tiles [cout/64][cin/32] of [9 taps][64 rows][4 positions of 16 bytes],
 *       chunk c (input channels 8c .. 8c+7 of the tile) of row n at position c ^ 2*((n>>2)&1) where cout % 128 == 0 (the
 *       16x16x32 MFMA's swizzle), else c ^ ((n>>2)&3) (the 32x32x16 one's).
 *   nqa_conv3x3_half                 that layer without bias or ReLU: f16 NHWC (n, H, W, cin) in, f16 NHWC (n, H, W, cout)
 *       out (float32 accumulation, rounded to half once).  The implicit GEMM's f16 instances: 128-channel tiles where
 *       cout % 128 == 0, else 64-channel tiles; 16-wide pixel tiles for W <= 16.  Maps and layer 16-byte aligned,
 *       H * W * max(cin, cout) * 2 < 2^31.  Counted as NQA_K_CONV.
 *   nqa_relu_mask_f16_scaled         out = (half)(g * 2^k[image]) where act > 0, else 0: g float or half NHWC
 *       (g_is_half), act a float tapped map or split16 records, out a plain half NHWC map; the scaling is exact, the
 *       conversion rounds to nearest even once.  C % 16 == 0, maps 16-byte aligned.  One launch (NQA_K_POOL).
 *   nqa_grad_exponent_half           nqa_grad_exponent for this chain: k[i] with max|g_i| * 2^k[i] in [8, 16) (that
 *       function's k minus 4), g float (per_image % 4 == 0) or half (per_image % 8 == 0), 16-byte aligned; the workspace
 *       is nqa_grad_exponent_bytes(n, per_image).
 *   nqa_l2pool_backward_scaled_half  nqa_l2pool_backward_scaled with a half g_pooled (8-byte aligned): taps, the tap's own
 *       gradient and the output stay float; the result is that function's on the halves converted to float, bit for bit.
 *   nqa_conv1_1_backward_scaled_half nqa_conv1_1_backward_scaled with a half g, likewise bit for bit.
 * NQA_E_ARG for null pointers, non-positive sizes and misaligned maps, NQA_E_SHAPE for channel counts (or per_image) the
 * kernels do not take, NQA_E_WORKSPACE for a short workspace. */
size_t nqa_packed_conv_half_bytes(int cout, int cin);
int nqa_pack_conv_half(const float *w_oihw, int cout, int cin, void *packed_host);
int nqa_conv3x3_half(const void *in_f16_nhwc, int n, int H, int W, int cin, int cout, const void *packed_conv,
                     void *out_f16_nhwc, void *stream);
int nqa_relu_mask_f16_scaled(const void *g_nhwc, int g_is_half, const void *act_nhwc, int act_is_split16, int n,
                             long pixels_per_image, int C, const int *k, void *out_f16, void *stream);
int nqa_grad_exponent_half(const void *g, int g_is_half, int n, long per_image, void *workspace, size_t workspace_bytes,
                           int *k, int *k_total, void *stream);
int nqa_l2pool_backward_scaled_half(const float *tap_nhwc, const void *g_pooled_f16, const float *g_tap_nhwc,
                                    const int *k_total, int n, int H, int W, int C, float *out_nhwc, void *stream);
int nqa_conv1_1_backward_scaled_half(const void *g_f16_nhwc, const void *relu1_1_split16, const float *w_oihw_dev,
                                     const int *k, const int *k_total, int n, int H, int W, float *g_image_nchw,
                                     void *stream);

/* ---- DISTS as a loss against a PREPARED TARGET (nerf_qa_amd/autograd.py, DistsTargetSimilarities): the statistics of
 * one tap pair split where the forward ends.  nqa_dists_stats_nhwc_backward is "sums, coefficients, gradient"; here the
 * forward runs the sums, keeps their per-block fp64 partials and forms S1 / S2 from them, and the backward starts from
 * the kept partials -- the same sums kernel on the same grid, so they are bit for bit what the backward would have formed.
 *
 *   nqa_dists_stats_target               tx, ty as above.  Writes the partials ([B][nblk][C][5] doubles: sum x, sum y,
 *       sum x^2, sum y^2, sum xy per block of pixels; nqa_dists_stats_target_bytes of them, 8-byte aligned) and
 *       S1 = (2 mx my + c) / (mx^2 + my^2 + c), S2 = (2 cov + c) / (vx + vy + c), c = 1e-6 (DISTS_pt.py:131-139),
 *       evaluated in fp64 and rounded to float once, pair b's C values at s1 / s2 + b * s_stride (s_stride >= C).  One
 *       writer per output, no atomics.  Two launches (sums, fold).
 *   nqa_dists_stats_nhwc_backward_from   nqa_dists_stats_nhwc_backward without its sums pass: `partials` as
 *       nqa_dists_stats_target left them for the same maps and shape (read only), `coef` the [B][C][6] fp64 coefficient
 *       records (nqa_dists_stats_nhwc_backward_from_bytes, 8-byte aligned, scratch).  gx, gy, g_s1, g_s2, g_stride as
 *       there, and the result equals that call's bit for bit.  Two launches (coefficients, gradient).
 * The argument rules of nqa_dists_stats_nhwc_backward: C a power of two in 16..1024 and H * W <= 2^30 (else NQA_E_SHAPE),
 * maps 16-byte aligned, no null pointer (gx or gy may be, not both), B in 1..65535, H, W > 0, stride >= C (else
 * NQA_E_ARG); a short partials or coefficient buffer is NQA_E_WORKSPACE.  All refused on the host before any launch; the
 * _bytes functions return 0 for a shape the kernels do not take.  Every launch is counted as NQA_K_STATS.  For C a
 * multiple of 32 (every tap) the two sizes add up to nqa_dists_stats_nhwc_backward_bytes. */
size_t nqa_dists_stats_target_bytes(int B, int H, int W, int C);
int nqa_dists_stats_target(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C, void *partials,
                           size_t partials_bytes, float *s1, float *s2, long s_stride, void *stream);
size_t nqa_dists_stats_nhwc_backward_from_bytes(int B, int C);
int nqa_dists_stats_nhwc_backward_from(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C,
                                       const void *partials, size_t partials_bytes, const float *g_s1, const float *g_s2,
                                       long g_stride, void *coef, size_t coef_bytes, float *gx_nhwc, float *gy_nhwc,
                                       void *stream);

/* ---- DISTS and A-DISTS as ONE loss against a prepared target (nerf_qa_amd/pair.py forward_target,
 * autograd.PairTargetLoss): the backward chain is linear in the tap gradients, so the two metrics' tap gradients are
 * summed and walked down once.  A-DISTS writes its NHWC tap gradient first (nqa_adists_ts_backward, out_nhwc = 1); the
 * DISTS term is then added IN PLACE, instead of being written to a map of its own and added by a third pass.
 *
 *   nqa_dists_stats_nhwc_grad_y_add   the y side of nqa_dists_stats_nhwc_backward_from, accumulated: tx, ty, partials,
 *       g_s1, g_s2, g_stride, coef as there; gy_inout dev float NHWC (B, H, W, C), read and written.
 *       gy_inout[e] = gy_inout[e] + u[e] in float, u[e] exactly the float nqa_dists_stats_nhwc_backward_from writes to
 *       gy_nhwc[e] (the fp64 fma chain rounded to float once, 0 where ty[e] <= 0): the result equals that call followed
 *       by one float add, bit for bit.  One reader-writer per element, no atomics, bitwise repeatable; no pair reads
 *       another pair's numbers; nothing is read back to the host.  Two launches (the coefficients as there, the
 *       accumulating gradient), counted as NQA_K_STATS.
 * The argument rules of nqa_dists_stats_nhwc_backward_from, refused on the host before any launch: C a power of two in
 * 16..1024 and H * W <= 2^30 (else NQA_E_SHAPE); no null pointer, gy_inout included, B in 1..65535, H, W > 0,
 * g_stride >= C, maps 16-byte and fp64 buffers 8-byte aligned (else NQA_E_ARG); a short partials or coefficient buffer is
 * NQA_E_WORKSPACE (sizes: nqa_dists_stats_target_bytes, nqa_dists_stats_nhwc_backward_from_bytes). */
int nqa_dists_stats_nhwc_grad_y_add(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C,
                                    const void *partials, size_t partials_bytes, const float *g_s1, const float *g_s2,
                                    long g_stride, void *coef, size_t coef_bytes, float *gy_inout, void *stream);

/* ---- the prepared-target loss step of DISTS as TWO calls (nqa_loss_step.hip; DISTS(target_step="c"),
 * nerf_qa_amd/autograd.py DistsTargetStep): everything autograd.dists_target_forward and dists_target_backward enqueue
 * launch by launch -- the single operators and loss-path entry points above, about a hundred of them a step -- driven by
 * host code in the library on ONE caller-owned state block.  The same launches on the same operands, in the same order
 * and on the same grids: s1, s2 and gy are that path's bit for bit on both gradient rungs, and every launch keeps its
 * timing class (the few element-wise kernels that stand where that path has a torch expression count as NQA_K_PREP).
 * Neither call allocates, synchronises or reads anything back to the host; a caller without Python has the whole loss
 * with nqa_dists_score and nqa_dists_score_backward around them (INTEGRATION.md section 2 shows the sequence).
 *
 *   grad_prec  the rung of the gradient chain: NQA_PREC_F32S (split16 operands, float results, nqa_pack_conv_split
 *              layers) or NQA_PREC_F16 (half maps, nqa_pack_conv_half layers).  The forward is the same on both; the state
 *              is sized by the rung, so both calls and nqa_dists_target_step_bytes take the same value.
 *   x_nchw     dev float32 NCHW (B,3,H,W), the target's frames;  x_taps: host array of five dev pointers, the target's
 *              float NHWC taps relu1_2 .. relu5_3, tap k + 1 (B, Hk, Wk, Ck) with Hk = ceil(H / 2^k): what the forward
 *              below leaves as y's taps, or nqa_vgg_pyramid in NQA_PREC_F32S, computed once for a whole optimisation.
 *   y_nchw     dev float32 NCHW (B,3,H,W), the frames the gradient is taken of.
 *   packed_w   the NQA_PREC_F32S blob of nqa_pack_vgg_weights, on the device.
 *   s1, s2     dev float32 (B, 1475), written by the forward;  g_s1, g_s2: dev float32 (B, 1475), dL/dS1 and dL/dS2.
 *   grad_layers  host array of twelve dev pointers: entry l - 1 is conv layer l's data-gradient layer, W'[ci][co][ky][kx]
 *              = W[co][ci][2-ky][2-kx] (a 3x3 layer of cout = the layer's cin, cin = the layer's cout), packed by the
 *              rung's packer.   w0_oihw_dev: conv1_1's float32 OIHW weights (64,3,3,3) on the device.
 *   gy_nchw    dev float32 NCHW (B,3,H,W): dL/dy.
 *   state      dev, nqa_dists_target_step_bytes(B, H, W, grad_prec) bytes, 256-byte aligned.  Laid out in regions on
 *              multiples of 256 bytes, in this order.  KEPT -- written by the forward, only READ by the backward, so a
 *              second backward on the same state gives the same bits: the thirteen activations of y (layer 0..12, NHWC,
 *              4 bytes per element; the tapped layers 1, 3, 6, 9, 12 are y's float taps, the others split16), the five
 *              taps' fp64 partials (nqa_dists_stats_target_bytes each), tap 0's fp64 sums (nqa_stats_scratch_bytes of the
 *              image beside five one-pixel maps) and those maps' B zero floats.  SCRATCH behind it, one area the two
 *              calls lay out each in its own way: the forward's four L2-pooled maps and the (B, 8) similarities of tap
 *              0, dead when it returns; the backward's five tap gradients, tap 0's image term and (B, 8) upstream, the
 *              fp64 coefficient records, the chain's exponents and their reduction partials, and three chain buffers of
 *              the largest layer map.  Every byte a call reads it or the forward has written before: no result depends
 *              on what the state held.  The backward must follow a forward with the same x, x_taps, y, B, H, W and
 *              grad_prec on the same state (it cannot check that without reading the device), on the same stream or
 *              ordered behind it; forward and backward may run on different host threads.
 * nqa_dists_target_step_forward   conv1_1, conv layers 1..12 and the four L2-pools of y in NQA_PREC_F32S, every
 *              activation kept; per tap 1..5 nqa_dists_stats_target (sums, fold) against x_taps; tap 0 through
 *              nqa_dists_stats_nchw with the five one-pixel zero maps, its three columns copied into s1 / s2.
 * nqa_dists_target_step_backward  per tap 1..5 nqa_dists_stats_nhwc_backward_from (coefficients, gradient, y side) from
 *              the kept partials; tap 0's nqa_dists_stats_nchw_backward from its kept sums; then the chain: the exponent
 *              of the top tap gradient, and per layer 12..1 mask, data-gradient convolution, the pool seam where the layer
 *              read an L2-pool, exponent (nqa_grad_exponent / nqa_relu_mask_split16_scaled / nqa_conv3x3_split /
 *              nqa_l2pool_backward_scaled, or their _half / f16 forms); nqa_conv1_1_backward_scaled with relu1_1's mask
 *              and 2^-k_total folded in; one float add of tap 0's image term into gy.
 * All arguments are checked on the host before the first launch, in this order, and a refused call enqueues nothing:
 *   NQA_E_ARG        a null pointer (each of the five taps and twelve layers included); B, H or W <= 0 or B > 65535; a
 *                    grad_prec that is neither rung;
 *   NQA_E_SHAPE      a frame whose map at some layer reaches 2^31 bytes (H * W * 64 floats at stage 1: the layers' 32-bit
 *                    in-image offsets), or B * H * W * 64 > 2^36 elements (slice the batch);
 *   NQA_E_ARG        a misaligned buffer: the state on 256 bytes, the five taps, packed_w and the twelve layers on 16,
 *                    every float array (x, y, s1, s2, g_s1, g_s2, w0, gy) on 4;
 *   NQA_E_WORKSPACE  a state under nqa_dists_target_step_bytes.
 * nqa_dists_target_step_bytes returns 0 for what the first two rules refuse.
 *
 * nqa_dists_score_backward   the derivative of nqa_dists_score (DISTS_pt.py:123-148) towards S1 and S2: g_s1[b][c] =
 *              -g_score[b] * alpha[c] / w, g_s2[b][c] = -g_score[b] * beta[c] / w, w = sum(alpha) + sum(beta) summed in
 *              fp64 as nqa_dists_score sums it and rounded to float; one float quotient, one float product.  alpha, beta
 *              dev float32 (1475), g_score dev float32 (B), g_s1 / g_s2 dev float32 (B, 1475).  NQA_E_ARG for a null
 *              pointer, B <= 0 or an array that is not 4-byte aligned.  One launch (NQA_K_PREP). */
size_t nqa_dists_target_step_bytes(int B, int H, int W, int grad_prec);
int nqa_dists_target_step_forward(const float *x_nchw, const void *const *x_taps, const float *y_nchw, int B, int H, int W,
                                  const void *packed_w, int grad_prec, void *state, size_t state_bytes, float *s1, float *s2,
                                  void *stream);
int nqa_dists_target_step_backward(const float *x_nchw, const void *const *x_taps, const float *y_nchw, int B, int H, int W,
                                   const float *g_s1, const float *g_s2, const void *const *grad_layers,
                                   const float *w0_oihw_dev, int grad_prec, void *state, size_t state_bytes, float *gy_nchw,
                                   void *stream);
int nqa_dists_score_backward(const float *alpha, const float *beta, const float *g_score, int B, float *g_s1, float *g_s2,
                             void *stream);

/* ---- windowed moments of the A-DISTS head under autograd (nerf_qa_amd/ADISTS/head.py, autograd.WindowMoments;
 * nqa_window_moments.hip).  x, y: dev float NCHW maps taken as P = B * C independent planes of H x W; the window is the
 * normalised 21-tap Gaussian of sigma 7 as an outer product, valid correlation: h = H - 20, w = W - 20.
 *
 *   nqa_window_moments_forward    out (n, P, h, w) dev float: with y the n = 5 window means E[x], E[y], E[x^2], E[y^2],
 *       E[xy], with y null the n = 2 means E[x], E[x^2].  One launch; the products never reach memory.
 *   nqa_window_moments_backward   g0 .. g4: upstream gradients of those five maps, each (P, h, w) dev float, null = zero.
 *       gx = W^T g0 + 2 x W^T g2 + y W^T g4 and gy = W^T g1 + 2 y W^T g3 + x W^T g4 (P, H, W), W^T the transposed
 *       correlation as a gather: a pixel sums over the windows that contain it, so no term of any other window can reach
 *       it.  gx or gy null: that side is skipped, the other is bit-identical to the two-sided call.  With y null (the
 *       moments of x alone) g1, g3, g4 and gy must be null.  One launch, one writer per element, no atomics.
 * Both need no workspace, read nothing back to the host and are counted as NQA_K_ADISTS.  Where W % 4 == 0 rows move
 * as 16-byte accesses and every pointer must be 16-byte aligned (a contiguous batch or channel slice of an aligned
 * tensor always is); for any other W nothing beyond a float's alignment is asked.  NQA_E_ARG: null pointer, P <= 0,
 * misaligned with W % 4 == 0; NQA_E_SHAPE: H or
 * W below 21 (no window fits: the head's global branch), H > 2^20, or more than 2^30 pixels per plane. */
int nqa_window_moments_forward(const float *x, const float *y, int P, int H, int W, float *out, void *stream);
int nqa_window_moments_backward(const float *x, const float *y, int P, int H, int W, const float *g0, const float *g1,
                                const float *g2, const float *g3, const float *g4, float *gx, float *gy, void *stream);

/* ---- A-DISTS as a loss with the gradient on y alone (nerf_qa_amd/autograd.py, adists_backward_y;
 * nqa_adists_backward.hip): ONE stage of the head's backward.  With x fixed, the texture probabilities and the channel
 * weights are constants, and only the T / S terms (ADISTS.py:165-183) and F.normalize of y (:167) are differentiated.
 *   x, y    dev float32 planar maps (B, C, H, W): the image pair (C = 3) or a tap pair converted to NCHW.
 *   q, wgt  dev float32 [8][B][ctot] and [B][ctot] as nqa_adists_front leaves them; the stage's C channels start at
 *           column coff (ctot = C, coff = 0 for a slice made for nqa_adists_window_stage).  Rows 0, 1: a_x, a_y =
 *           1 / max(||.||_2, 1e-12) of the raw maps; rows 3..7 (global branch only): mean_x mean_y var_x var_y cov.
 *   ps      dev float32 (B, mh, mw): ps_prod of the stage as nqa_adists_chain writes it, mh x mw = (H-20) x (W-20), or
 *           1 x 1 for the global branch.
 *   u       dev float32 (B): u_b = dL/dD_b (for 1 - mean(D): -upstream / B).
 *   mask    != 0: gy is multiplied by the map's own ReLU mask (y > 0), so a dead channel gets exactly 0 (taps); 0: not
 *           (the image).
 *   gy      dev float32, dL/dy: planar (B, C, H, W), or with out_nhwc != 0 NHWC (B, H, W, C).
 * Arithmetic, with N = mh * mw and eps = 1e-6.  Windowed stage (H, W >= 21): from the raw window means m_x, m_y, m_xx,
 * m_yy, m_xy of nqa_window_moments_forward,
 *     xm = a_x m_x, ym = a_y m_y, xv = a_x^2 m_xx - xm^2, yv = a_y^2 m_yy - ym^2, cov = a_x a_y m_xy - xm ym,
 *     T = (2 xm ym + eps) / (xm^2 + ym^2 + eps), S = (2 cov + eps) / (xv + yv + eps),
 *     A = u_b w_c (1 - p) / N, Bc = u_b w_c p / N,
 *     dT/dym = (2 xm - 2 ym T) / (xm^2 + ym^2 + eps), dS/dcov = 2 / (xv + yv + eps), dS/dyv = -S / (xv + yv + eps),
 *     G_ym = A dT/dym - Bc (xm dS/dcov + 2 ym dS/dyv), G_yy = Bc dS/dyv, G_xy = Bc dS/dcov,
 *     g1 = a_y G_ym, g3 = a_y^2 G_yy, g4 = a_x a_y G_xy   (fp64 on the float moments, rounded to float once),
 *     P = W^T g1 + 2 y W^T g3 + x W^T g4                    (nqa_window_moments_backward's gy with gx null),
 *     gy = P - y a_y^2 <P, y>, or P alone where ||y|| < 1e-12 (torch's clamp in F.normalize), times the mask.
 * <P, y> is the sum over the plane, accumulated in fp64 from per-block partials folded in a fixed order.  Global stage
 * (H or W under 21): the same with plain means over H * W from q rows 3..7 (xv = a_x^2 var_x, ...), N = 1, one p per pair,
 * P(r) = (g1 + 2 y(r) g3 + x(r) g4) / (H W).  One writer per element, no atomics: bitwise repeatable; no pair reads
 * another pair's numbers; nothing is read back to the host.  Launches are counted as NQA_K_ADISTS.
 * Workspace: nqa_adists_ts_backward_bytes(B, C, H, W) (0 for sizes that are refused): the five moment maps, P and the
 * fp64 partials; 16-byte aligned.  The regions lie in this order, each rounded up to 16 bytes, and all of them are still
 * there when the call returns: the partials (P * ceil(H W / 4096) doubles, plane-major, P = B * C), s = a_y^2 <P, y> (P
 * doubles), P (P * H W floats), the five moment maps (moment m of plane p at ((m * P + p) * mh * mw) floats; g1, g3, g4
 * have replaced moments 1, 3, 4); the global branch keeps nothing in its 16 bytes (tests/ts_backward_refs.py, layout).
 * Refused on the host, before any launch: NQA_E_ARG null pointer, non-positive size, coff < 0 or coff + C > ctot, more
 * than 65535 pairs, a misaligned workspace, or -- on a windowed stage with W % 4 == 0, where rows move as 16-byte
 * accesses -- x, y, ps or gy not 16-byte aligned; NQA_E_SHAPE H > 2^20, more than 2^30 pixels per plane, more than 2^31
 * blocks in a launch, or out_nhwc on a windowed stage with C % 32 != 0; NQA_E_WORKSPACE a short workspace (checked
 * last). */
size_t nqa_adists_ts_backward_bytes(int B, int C, int H, int W);
int nqa_adists_ts_backward(const float *x, const float *y, int B, int C, int H, int W, const float *q, const float *wgt,
                           int ctot, int coff, const float *ps, const float *u, int mask, int out_nhwc, void *workspace,
                           size_t workspace_bytes, float *gy, void *stream);

/* ---- the same four entry points for a window of `window` taps, 3 <= window <= 63, odd or even: the normalised
 * Gaussian of sigma window / 3 centred at window / 2 (integer division, so an even window is not symmetric), the taps of
 * nqa_adists_forward_n.  Everything above holds with 21 replaced by `window`:
 * h = H - window + 1, w = W - window + 1; a stage of nqa_adists_ts_backward_n is windowed iff H >= window && W >= window,
 * ps is (B, h, w) there and (B, 1, 1) on the global branch, which a map under the window in either direction takes.
 * Sums run in ascending tap order forwards and in ascending window order in the transposed pass, which walks the taps
 * mirrored.  Rows move as 16-byte accesses where W % 4 == 0 (the window-mean maps only where also (window - 1) % 4 == 0),
 * and the alignment rule is the one above: every pointer 16-byte aligned where W % 4 == 0 (ps of
 * nqa_adists_ts_backward_n only where mh * mw is a multiple of 4 as well: nothing else reads it in 16-byte pieces, and a
 * stage's ps inside a larger buffer need not start on a 16-byte boundary then).
 * The entry points above ARE these four at window == 21, under their own names in the messages, with one difference:
 * here window == 21 runs the 21-tap kernels, bit for bit, unless nqa_set_conv_variant carries 4096, which sends it to the
 * generic kernels too (tests, A/B runs); the entry points above run the 21-tap kernels whatever the variant says.
 * Refusals are those above, on the host and before any launch, and in addition NQA_E_ARG for a window outside [3, 63]
 * (the message names the range); NQA_E_SHAPE for H or W below `window` on the two moments entry points.
 * nqa_adists_ts_backward_bytes_n is 0 for a window outside the range as for every other refused size. */
int nqa_window_moments_forward_n(const float *x, const float *y, int P, int H, int W, int window, float *out,
                                 void *stream);
int nqa_window_moments_backward_n(const float *x, const float *y, int P, int H, int W, int window, const float *g0,
                                  const float *g1, const float *g2, const float *g3, const float *g4, float *gx, float *gy,
                                  void *stream);
size_t nqa_adists_ts_backward_bytes_n(int B, int C, int H, int W, int window);
int nqa_adists_ts_backward_n(const float *x, const float *y, int B, int C, int H, int W, int window, const float *q,
                             const float *wgt, int ctot, int coff, const float *ps, const float *u, int mask,
                             int out_nhwc, void *workspace, size_t workspace_bytes, float *gy, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NQA_H */
