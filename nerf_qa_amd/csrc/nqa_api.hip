// extern "C" surface of libnqa_hip.so (include/nqa.h): error plumbing, launch preparation, timing ring,
// and the drivers that chain the kernels into forward_once / DISTS.forward
// (nerf_qa/DISTS_pytorch/DISTS_pt.py:91-148).  The weight packers are in nqa_weights.hip.
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <thread>
#include <vector>

#include "nqa_stages.h"

namespace nqa {

// ---- errors ---------------------------------------------------------------------
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return NQA_E_LAUNCH;
  }
  return NQA_OK;
}

// ---- tuning state (nqa_common.h) ---------------------------------------------------
Tuning &tuning() {
  static thread_local Tuning t;
  return t;
}

// ---- launch preparation (nqa_common.h) ----------------------------------------------------
int current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}

int num_cus(const char *who) {
  static std::atomic<int> cus[64];  // (concurrent first calls both query and store the same value)
  const int dev = current_device() & 63;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (!n) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
      if (who) set_error("%s: cannot query the device", who);
      return 0;
    }
    n = prop.multiProcessorCount;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int raise_lds_limit(const void *kernel, std::atomic<bool> *done_dev, int bytes, const char *who) {
  std::atomic<bool> &done = done_dev[current_device() & 63];
  if (!done) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      set_error("%s: cannot raise the dynamic LDS limit to %d bytes", who, bytes);
      return NQA_E_LAUNCH;
    }
    done = true;
  }
  return NQA_OK;
}

// ---- timing ring ------------------------------------------------------------------
// Thread-local like the error string: a thread that enables timing brackets ITS OWN launches (on whatever
// streams it uses) and collects only those, so concurrent callers on other threads / streams are neither
// timed nor disturbed.  The events are created once per thread and reused.
static const int kRing = 16384;
static thread_local bool g_timing = false;
static thread_local std::vector<hipEvent_t> g_ev0, g_ev1;
static thread_local std::vector<int> g_cls;
static thread_local int g_used = 0;
// The events are created lazily, up to the high-water mark a thread actually used, and given back when the thread
// ends -- except on the thread that loaded the library (normally the process's main thread): its thread_locals are
// destroyed during process exit, when the HIP runtime may already be gone.
static const std::thread::id g_load_thread = std::this_thread::get_id();
struct TimingRingOwner {
  ~TimingRingOwner() {
    if (std::this_thread::get_id() == g_load_thread) return;
    for (hipEvent_t e : g_ev0) (void)hipEventDestroy(e);
    for (hipEvent_t e : g_ev1) (void)hipEventDestroy(e);
    g_ev0.clear();
    g_ev1.clear();
  }
};
static thread_local TimingRingOwner g_ring_owner;  // constructed after the vectors (first touched below), destroyed before them

TimedLaunch::TimedLaunch(int kc, hipStream_t s) : kclass(kc), stream(s), slot(-1) {
  if (!g_timing || g_used >= kRing) return;
  if ((int)g_ev0.size() <= g_used) {
    (void)&g_ring_owner;  // (odr-use: the owner exists in every thread that ever creates events)
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    g_ev0.push_back(a);
    g_ev1.push_back(b);
    g_cls.push_back(kc);
  }
  slot = g_used++;
  g_cls[slot] = kc;
  (void)hipEventRecord(g_ev0[slot], stream);
}
TimedLaunch::~TimedLaunch() {
  if (slot >= 0) (void)hipEventRecord(g_ev1[slot], stream);
}

// ---- drivers ----------------------------------------------------------------------------
// Elements of the largest activation map of the pyramid, per image.  For ordinary frames that is
// stage 1 (H*W*64), but the maps shrink by ceil(./2) while the channels double, so below ~8 pixels
// a side a LATER stage is the largest (a 1x1 frame: 64 elements at stage 1, 512 at stages 4 and 5);
// sizing the ping-pong buffers by stage 1 alone let those stages write past them.
size_t max_act_elems(int H, int W) {
  static const int kStageC[5] = {64, 128, 256, 512, 512};
  const PyrDims d = pyr_dims(H, W);
  size_t m = 0;
  for (int k = 0; k < 5; ++k) {
    const size_t e = (size_t)d.h[k] * d.w[k] * kStageC[k];
    m = e > m ? e : m;
  }
  return m;
}
static size_t act_bytes(int n, int H, int W, int prec) {
  if (is_mixed(prec)) {  // the largest map in BYTES: stages differ in element size
    static const int kStageC[5] = {64, 128, 256, 512, 512};
    const PyrDims d = pyr_dims(H, W);
    size_t m = 0;
    for (int k = 0; k < 5; ++k) {
      const size_t e = (size_t)d.h[k] * d.w[k] * kStageC[k] * prec_elem_bytes(stage_prec(prec, k));
      m = e > m ? e : m;
      if (k > 0) {  // stage k's input: stage k-1's pooled map in stage k's format
        const size_t p = (size_t)d.h[k] * d.w[k] * kStageC[k - 1] * prec_elem_bytes(stage_prec(prec, k));
        m = p > m ? p : m;
      }
    }
    return align_up((size_t)n * m, 256);
  }
  return align_up((size_t)n * max_act_elems(H, W) * prec_elem_bytes(prec), 256);
}

// `chan`: the widest H x W map the call addresses with 32-bit in-image byte offsets (the conv DMA
// plan): 64 channels for the pyramid paths (H, W are stage-1 sizes; later stages have 1/4 of the
// pixels per doubling of the channels), the layer's own input width for the single-operator calls.
// `mixed_ok`: the entry point takes the mixed modes.  `stage` >= 0: a single-operator call on a map of that pyramid
// stage (0-based), whose element size is the stage's own (stage_prec) -- in a mixed mode 2 or 4 bytes by stage.
static bool bad_dims(const char *who, int n, int H, int W, int prec, int chan = 512, bool mixed_ok = false,
                     int stage = -1) {
  if (n <= 0 || H <= 0 || W <= 0) {
    set_error("%s: non-positive size n=%d H=%d W=%d", who, n, H, W);
    return true;
  }
  if (!(mixed_ok ? prec_valid_pyramid(prec) : prec_valid(prec))) {
    set_error(is_mixed(prec) ? "%s: takes no mixed mode (prec %d): pass the kernel precision of the map's own stage"
                             : "%s: unknown prec %d", who, prec);
    return true;
  }
  const long eb = (long)prec_elem_bytes(stage >= 0 ? stage_prec(prec, stage) : prec);
  if (chan > 0 && (long)H * W * chan * eb >= (1L << 31)) {
    set_error("%s: map too large for 32-bit in-image byte offsets (H*W*%d channels*%d bytes >= 2^31)", who, chan,
              (int)eb);
    return true;
  }
  return false;
}

struct StatsPlan {
  StageDesc d;
  size_t doubles;
};
// `pooled[k]` = {Ho, Wo} where stage k's statistics come out of the fused pool+statistics pass
// ({0,0}: the plain NHWC pass over HW[k]); pooled == null: every stage runs the NCHW plane kernel.
static StatsPlan stats_plan(int B, const int *C, const int *HW, const int (*pooled)[2], int nstage, int prec,
                            const bool *fused = nullptr) {
  StatsPlan p;
  memset(&p, 0, sizeof(p));
  long off = 0;
  int coff = 0;
  for (int k = 0; k < nstage; ++k) {
    const bool nchw = !pooled || k == 0;
    const int kp = k >= 1 ? stage_prec(prec, k - 1) : prec;  // tap k comes out of pyramid stage k-1 (0-based)
    int nblk;
    if (nchw)
      nblk = cdiv(HW[k], stats_nchw_ppb(HW[k]));
    else if (fused && fused[k])  // (rows per pair reserved by the fused conv + pool + statistics kernels; unwritten rows are zero)
      nblk = k == 1 ? NQA_FUSED_PART_BLOCKS_S1 : NQA_FUSED_PART_BLOCKS;
    else if (pooled[k][0])
      nblk = pool_stats_tiles(pooled[k][0], pooled[k][1], C[k], kp, B, nullptr, nullptr);
    else
      nblk = cdiv(HW[k], stats_units_per_block(HW[k], C[k], kp, B));
    p.d.part_off[k] = off;
    p.d.nblk[k] = nblk;
    p.d.hw[k] = HW[k];
    p.d.c[k] = C[k];
    p.d.coff[k] = coff;
    off += (long)B * p.d.nblk[k] * C[k] * 5;
    coff += C[k];
  }
  p.d.nstage = nstage;
  p.d.ctot = coff;
  p.doubles = (size_t)off;
  return p;
}

}  // namespace nqa

using namespace nqa;

extern "C" {

int nqa_version(void) { return NQA_VERSION; }
const char *nqa_last_error(void) { return g_err; }

int nqa_set_conv_variant(int variant) {
  Tuning &t = tuning();
  if (variant == 1024) {  // the query: changes no choice, and starts the count again
    const int c = t.mixed_launches;
    t.mixed_launches = 0;
    return c;
  }
  const bool window_generic = variant > 0 && (variant & 2048) != 0;  // bit 11 rides above the query value 1024
  const int asked = variant;
  if (window_generic) variant -= 2048;
  // bit 12, for the _n window-moments entry points; counted only on top of a non-zero variant: a bare 4096 stays the
  // unknown variant it was before the bit existed
  const bool moments_generic = variant > 4096 && (variant & 4096) != 0;
  if (moments_generic) variant -= 4096;
  if (variant < 0 || variant > 1023 || (variant & 3) == 3 || (variant & 768) == 768) {
    set_error("set_conv_variant: unknown variant %d", asked);
    return NQA_E_ARG;
  }
  t.conv_variant = variant & 3;
  t.stage1_variant = (variant >> 2) & 1;
  t.window_legacy = (variant & 8) != 0;
  t.first_forms = (variant & 16) != 0;
  t.no_regw128 = (variant & 32) != 0;
  t.fuse_taps = !(variant & 64);
  t.fuse_stage1 = !(variant & 128);
  t.edge_grid = (variant >> 8) & 3;
  t.window_generic = window_generic;
  t.moments_generic = moments_generic;
  return NQA_OK;
}

int nqa_timing_enable(int on) {
  g_timing = on != 0;
  g_used = 0;
  return NQA_OK;
}

int nqa_timing_collect(int launches[NQA_K_COUNT], double ms[NQA_K_COUNT]) {
  for (int i = 0; i < NQA_K_COUNT; ++i) {
    launches[i] = 0;
    ms[i] = 0.0;
  }
  for (int s = 0; s < g_used; ++s) {
    float t = 0.f;
    if (hipEventSynchronize(g_ev1[s]) != hipSuccess || hipEventElapsedTime(&t, g_ev0[s], g_ev1[s]) != hipSuccess) {
      set_error("timing_collect: event %d failed", s);
      g_used = 0;
      return NQA_E_LAUNCH;
    }
    launches[g_cls[s]] += 1;
    ms[g_cls[s]] += (double)t;
  }
  g_used = 0;
  return NQA_OK;
}

int nqa_conv1_1(const float *x, int n, int H, int W, const void *packed, int prec, void *out, void *stream) {
  if (!x || !packed || !out) {
    set_error("conv1_1: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("conv1_1", n, H, W, prec, 64, true, 0)) return NQA_E_ARG;
  return conv1_1(x, n, H, W, packed, prec, out, static_cast<hipStream_t>(stream));
}

int nqa_conv1_fused(const float *x, int n, int H, int W, const void *packed, int prec, void *out, void *stream) {
  if (!x || !packed || !out) {
    set_error("conv1_fused: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("conv1_fused", n, H, W, prec, 64, true, 0)) return NQA_E_ARG;
  // a mixed mode: the fused form exactly where run_stages takes it, never another kernel under its name
  if (is_mixed(prec) && !stage1_is_fused(prec, W)) {
    set_error("conv1_fused: a mixed mode runs stage 1 fused only for W >= 16 with the first-forms bit of "
              "nqa_set_conv_variant clear (W = %d): nqa_conv1_1 + nqa_conv3x3_relu(layer 1) otherwise", W);
    return NQA_E_SHAPE;
  }
  return conv1_fused(x, nullptr, n, n, H, W, packed, prec, out, static_cast<hipStream_t>(stream));
}

int nqa_conv3x3_relu(const void *in, int n, int H, int W, int layer, const void *packed, int prec, void *out,
                     void *stream) {
  if (!in || !packed || !out) {
    set_error("conv3x3_relu: null pointer");
    return NQA_E_ARG;
  }
  if (layer < 1 || layer >= NQA_NUM_CONVS) {
    set_error("conv3x3_relu: layer %d out of range 1..12", layer);
    return NQA_E_ARG;
  }
  if (bad_dims("conv3x3_relu", n, H, W, prec, kConvs[layer].cin > kConvs[layer].cout ? kConvs[layer].cin : kConvs[layer].cout,
               true, kConvs[layer].stage))
    return NQA_E_ARG;
  return conv3x3(in, n, H, W, layer, packed, prec, out, static_cast<hipStream_t>(stream));
}

int nqa_l2pool(const void *in, int n, int H, int W, int C, int prec, void *out, void *stream) {
  if (!in || !out) {
    set_error("l2pool: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("l2pool", n, H, W, prec, C > 0 ? C : 1, true, 0)) return NQA_E_ARG;
  if (C <= 0 || C % 8) {
    set_error("l2pool: C=%d must be a positive multiple of 8", C);
    return NQA_E_SHAPE;
  }
  // a mixed mode: the pool INSIDE its 16-bit stages (half in, half out); the boundary pool is nqa_l2pool_f16_to_split16
  return l2pool(in, n, H, W, C, is_mixed(prec) ? NQA_PREC_F16 : prec, out, static_cast<hipStream_t>(stream));
}

int nqa_l2pool_f16_to_split16(const void *in, int n, int H, int W, int C, void *out, void *stream) {
  if (!in || !out) {
    set_error("l2pool_f16_to_split16: null pointer");
    return NQA_E_ARG;
  }
  // (sized by the 4-byte records it writes; its input is half as large)
  if (bad_dims("l2pool_f16_to_split16", n, H, W, NQA_PREC_F32S, C > 0 ? C : 1)) return NQA_E_ARG;
  if (C <= 0 || C % 16) {  // a split16 record holds 16 channels
    set_error("l2pool_f16_to_split16: C=%d must be a positive multiple of 16", C);
    return NQA_E_SHAPE;
  }
  return l2pool_to_split16(in, n, H, W, C, out, static_cast<hipStream_t>(stream));
}

int nqa_nhwc_to_nchw_f32(const void *in, int n, int H, int W, int C, int prec, float *out, void *stream) {
  if (!in || !out) {
    set_error("nhwc_to_nchw: null pointer");
    return NQA_E_ARG;
  }
  // the export kernel indexes with size_t: no 32-bit in-image offset bound here (a 1080p float tap is 531 MB
  // per image at 64 channels and must pass); only the grid's limits apply
  if (bad_dims("nhwc_to_nchw", n, H, W, prec, 0) || C <= 0) return NQA_E_ARG;
  if ((long)H * W > (1L << 31) - 64 || n > 65535 || C > 65535 * 64) {  // grid = (HW/64, C/64, n)
    set_error("nhwc_to_nchw: map too large for the launch grid (H*W=%ld, C=%d, n=%d)", (long)H * W, C, n);
    return NQA_E_SHAPE;
  }
  return nhwc_to_nchw(in, n, H * W, C, prec, out, static_cast<hipStream_t>(stream));
}

// Statistics plan of the fused DISTS path: stage 0 from the raw images (NCHW kernel), taps 1..4
// inside the fused pool+statistics pass (items = pooled pixels), tap 5 by the plain NHWC pass.
// which taps (index 1..5 of the statistics plan) the DISTS path runs fused with their conv (nqa_conv_pool.hip)
static void dists_fused_taps(int B, int H, int W, int prec, bool fused[6]) {
  const PyrDims d = pyr_dims(H, W);
  for (int k = 0; k < 6; ++k) fused[k] = false;
  fused[1] = conv1_pool_fusable(B, H, W, prec);
  fused[2] = conv_pool_fusable(3, B, d.h[1], d.w[1], prec, stage_prec(prec, 1));
}
static StatsPlan dists_stats_plan(int B, int H, int W, int prec, bool allow_fused = true) {
  const PyrDims d = pyr_dims(H, W);
  int C[6], HW[6], pooled[6][2];
  bool fused[6];
  dists_fused_taps(B, H, W, prec, fused);
  if (!allow_fused)
    for (int k = 0; k < 6; ++k) fused[k] = false;
  C[0] = 3;
  HW[0] = H * W;
  pooled[0][0] = pooled[0][1] = 0;
  for (int k = 0; k < 5; ++k) {
    C[k + 1] = kChns[k + 1];
    HW[k + 1] = d.h[k] * d.w[k];
    pooled[k + 1][0] = k < 4 ? d.h[k + 1] : 0;
    pooled[k + 1][1] = k < 4 ? d.w[k + 1] : 0;
  }
  return stats_plan(B, C, HW, pooled, 6, prec, fused);
}
// seam planes of the fused taps (behind the statistics partials in the workspace)
static size_t dists_seam_bytes(int B, int H, int W) {  // (one area: tap 1's planes are consumed before tap 2's are written)
  const PyrDims d = pyr_dims(H, W);
  const size_t s1 = conv_pool_seam_bytes(B, H, W, 64), s2 = conv_pool_seam_bytes(B, d.h[1], d.w[1], 128);
  return s1 > s2 ? s1 : s2;
}

size_t nqa_workspace_bytes(int n_images, int H, int W, int prec) {
  if (n_images <= 0 || H <= 0 || W <= 0) return 0;
  // (sized for the fused and for the unfused form of every tap: the choice can be switched per thread, nqa_set_conv_variant)
  const int B = (n_images + 1) / 2;
  const size_t pa = dists_stats_plan(B, H, W, prec, true).doubles, pb = dists_stats_plan(B, H, W, prec, false).doubles;
  return 2 * act_bytes(n_images, H, W, prec) + align_up((pa > pb ? pa : pb) * 8, 256) + dists_seam_bytes(B, H, W);
}

int nqa_vgg_pyramid(const float *x, int n, int H, int W, const void *packed, int prec, void *ws, size_t ws_bytes,
                    void *const taps[5], void *stream) {
  if (!x || !packed || !ws || !taps) {
    set_error("vgg_pyramid: null pointer");
    return NQA_E_ARG;
  }
  for (int k = 0; k < 5; ++k)
    if (!taps[k]) {
      set_error("vgg_pyramid: taps[%d] is null", k);
      return NQA_E_ARG;
    }
  if (bad_dims("vgg_pyramid", n, H, W, prec, 64, true)) return NQA_E_ARG;
  const size_t ab = act_bytes(n, H, W, prec);
  if (ws_bytes < 2 * ab) {
    set_error("vgg_pyramid: workspace %zu < %zu bytes", ws_bytes, 2 * ab);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *bufA = static_cast<char *>(ws), *bufB = bufA + ab;
  return run_stages(x, nullptr, n, bufA, bufB, n, H, W, packed, prec, taps,
                    [](int, void *, int, int, int, void *) { return 0; }, st);
}

int nqa_dists_forward(const float *x, const float *y, int B, int H, int W, const void *packed, int prec, void *ws,
                      size_t ws_bytes, float *s1, float *s2, void *stream) {
  if (!x || !y || !packed || !ws || !s1 || !s2) {
    set_error("dists_forward: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("dists_forward", B, H, W, prec, 64, true)) return NQA_E_ARG;
  const int n = 2 * B;
  const size_t need = nqa_workspace_bytes(n, H, W, prec);
  if (ws_bytes < need) {
    set_error("dists_forward: workspace %zu < %zu bytes", ws_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t ab = act_bytes(n, H, W, prec);
  char *bufA = static_cast<char *>(ws), *bufB = bufA + ab;
  double *part = reinterpret_cast<double *>(bufB + ab);
  const StatsPlan p = dists_stats_plan(B, H, W, prec);
  const size_t pa = p.doubles, pb = dists_stats_plan(B, H, W, prec, false).doubles;
  float *seam = reinterpret_cast<float *>(reinterpret_cast<char *>(part) + align_up((pa > pb ? pa : pb) * 8, 256));
  bool fused[6];
  dists_fused_taps(B, H, W, prec, fused);
  int rc;
  // feature 0 is the raw image (DISTS_pt.py:103): statistics straight from the inputs
  if ((rc = stats_nchw(x, y, B, 3, H * W, part + p.d.part_off[0], st))) return rc;
  // x images occupy [0,B), y images [B,2B) of one NHWC batch
  rc = run_stages(
      x, y, B, bufA, bufB, n, H, W, packed, prec, nullptr,
      [&](int k, void *tap, int hk, int wk, int ck, void *pool_dst) {
        double *pk = part + p.d.part_off[k + 1];
        const int kp = stage_prec(prec, k);  // (mixed mode: half taps up to stage 3, float ones behind)
        if (!pool_dst) return stats_nhwc(tap, B, hk * wk, ck, kp, pk, st);
        const bool boundary = is_mixed(prec) && kp == NQA_PREC_F16 && stage_prec(prec, k + 1) == NQA_PREC_F32S;
        const int rc2 = boundary ? pool_stats_to_split16(tap, B, hk, wk, ck, pool_dst, pk, st)
                                 : pool_stats(tap, B, hk, wk, ck, kp, pool_dst, pk, st);
        return rc2 ? rc2 : 1;
      },
      st,
      [&](int k, const void *inp, int hk, int wk, int layer, void *pool_dst) {
        if (!fused[k + 1]) return 0;
        const int rc2 = conv_pool_stats_fused(inp, B, hk, wk, layer, packed, prec, pool_dst, seam, part + p.d.part_off[k + 1], st);
        return rc2 ? rc2 : 1;
      },
      [&](void *pool_dst) {
        if (!fused[1]) return 0;
        const int rc2 = conv1_pool_stats_fused(x, y, B, H, W, packed, pool_dst, seam, part + p.d.part_off[1], st);
        return rc2 ? rc2 : 1;
      });
  if (rc) return rc;
  return finalize(part, p.d, B, s1, s2, st);
}

// ---- one reference against its K renders (nqa_group_stats.hip) ----
// Statistics plan of R groups of K renders over `nstage` maps: the partial sums in finalize's layout for B = R * K pairs.
// nchw[k]: map k is float planes (the plane kernel), else an NHWC tap in kprec[k].
static StatsPlan group_stats_plan(int R, int K, const int *C, const int *HW, const bool *nchw, const int *kprec, int nstage) {
  StatsPlan p;
  memset(&p, 0, sizeof(p));
  long off = 0;
  int coff = 0;
  for (int k = 0; k < nstage; ++k) {
    p.d.part_off[k] = off;
    p.d.nblk[k] = nchw[k] ? cdiv(HW[k], stats_nchw_ppb(HW[k])) : cdiv(HW[k], group_stats_units_per_block(HW[k], C[k], kprec[k], R));
    p.d.hw[k] = HW[k];
    p.d.c[k] = C[k];
    p.d.coff[k] = coff;
    off += (long)R * K * p.d.nblk[k] * C[k] * 5;
    coff += C[k];
  }
  p.d.nstage = nstage;
  p.d.ctot = coff;
  p.doubles = (size_t)off;
  return p;
}
// the image and the five taps of an H x W frame in mode `prec`
static StatsPlan group_forward_plan(int R, int K, int H, int W, int prec) {
  const PyrDims d = pyr_dims(H, W);
  int C[6], HW[6], kprec[6];
  bool nchw[6];
  for (int k = 0; k < 6; ++k) {
    C[k] = kChns[k];
    HW[k] = k ? d.h[k - 1] * d.w[k - 1] : H * W;
    kprec[k] = k ? stage_prec(prec, k - 1) : NQA_PREC_F32;
    nchw[k] = k == 0;
  }
  return group_stats_plan(R, K, C, HW, nchw, kprec, 6);
}
// finalize folds one pair per grid row: R * K pairs must fit a grid's second dimension
static const long kGroupMaxPairs = 65535;
static bool bad_group(const char *who, int R, int K) {
  if (R <= 0 || K <= 0) {
    set_error("%s: non-positive size R=%d K=%d", who, R, K);
    return true;
  }
  if ((long)R * K > kGroupMaxPairs) {
    set_error("%s: R*K = %ld pairs, more than %ld in one call", who, (long)R * K, kGroupMaxPairs);
    return true;
  }
  return false;
}

size_t nqa_dists_group_workspace_bytes(int R, int K, int H, int W, int prec) {
  if (R <= 0 || K <= 0 || H <= 0 || W <= 0 || (long)R * K > kGroupMaxPairs || !prec_valid_pyramid(prec)) return 0;
  return 2 * act_bytes(R + R * K, H, W, prec) + align_up(group_forward_plan(R, K, H, W, prec).doubles * 8, 256);
}

int nqa_dists_forward_group(const float *ref, const float *renders, int R, int K, int H, int W, const void *packed, int prec,
                            void *ws, size_t ws_bytes, float *s1, float *s2, void *stream) {
  if (!ref || !renders || !packed || !ws || !s1 || !s2) {
    set_error("dists_forward_group: null pointer");
    return NQA_E_ARG;
  }
  if (bad_group("dists_forward_group", R, K)) return NQA_E_ARG;
  const int n = R + R * K;
  if (bad_dims("dists_forward_group", n, H, W, prec, 64, true)) return NQA_E_ARG;
  const size_t need = nqa_dists_group_workspace_bytes(R, K, H, W, prec);
  if (ws_bytes < need) {
    set_error("dists_forward_group: workspace %zu < %zu bytes", ws_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t ab = act_bytes(n, H, W, prec);
  char *bufA = static_cast<char *>(ws), *bufB = bufA + ab;
  double *part = reinterpret_cast<double *>(bufB + ab);
  const StatsPlan p = group_forward_plan(R, K, H, W, prec);
  int rc;
  // feature 0 is the raw image (DISTS_pt.py:103): statistics straight from the inputs
  if ((rc = group_stats_nchw(ref, renders, R, K, 3, H * W, part + p.d.part_off[0], st))) return rc;
  // the references occupy images [0,R) of one NHWC batch, render (r, k) image R + r * K + k
  rc = run_stages(ref, renders, R, bufA, bufB, n, H, W, packed, prec, nullptr,
                  [&](int k, void *tap, int hk, int wk, int ck, void *) {
                    const int kp = stage_prec(prec, k);  // (mixed mode: half taps up to the boundary, float ones behind)
                    const char *rn = static_cast<const char *>(tap) + (size_t)R * hk * wk * ck * prec_elem_bytes(kp);
                    return group_stats_nhwc(tap, rn, R, K, hk * wk, ck, kp, part + p.d.part_off[k + 1], st);
                  },
                  st);
  if (rc) return rc;
  return finalize(part, p.d, R * K, s1, s2, st);
}

size_t nqa_dists_group_stats_bytes(int R, int K, int HW, int C, int prec, int nchw) {
  if (R <= 0 || K <= 0 || HW <= 0 || C <= 0 || (long)R * K > kGroupMaxPairs || !prec_valid(prec)) return 0;
  if (!nchw && !group_stats_nhwc_ok(C, prec)) return 0;
  const bool planes = nchw != 0;
  return align_up(group_stats_plan(R, K, &C, &HW, &planes, &prec, 1).doubles * 8, 256);
}

// The checks and the launch shared by nqa_dists_group_stats and nqa_dists_group_sums (`who` names the caller in the
// messages; the null-pointer check is the caller's): the partials land in `scratch` in the layout of *plan.
static int group_stats_launch(const char *who, const void *feat, int R, int K, int HW, int C, int prec, int nchw,
                              void *scratch, size_t scratch_bytes, StatsPlan *plan, hipStream_t st) {
  if (bad_group(who, R, K)) return NQA_E_ARG;
  if (HW <= 0 || C <= 0) {
    set_error("%s: non-positive size HW=%d C=%d", who, HW, C);
    return NQA_E_ARG;
  }
  if (!prec_valid(prec)) {
    set_error(is_mixed(prec) ? "%s: takes no mixed mode (prec %d): pass the kernel precision of the map's own stage"
                             : "%s: unknown prec %d", who, prec);
    return NQA_E_ARG;
  }
  const long eb = nchw ? 4 : (long)prec_elem_bytes(prec);  // (planes are float whatever prec is)
  if ((long)HW * C * eb >= (1L << 31)) {
    set_error("%s: map too large (HW*%d channels*%d bytes >= 2^31)", who, C, (int)eb);
    return NQA_E_ARG;
  }
  if (!nchw && !group_stats_nhwc_ok(C, prec)) {
    set_error("%s: no NHWC kernel for C=%d in prec %d (whole 16-byte groups, a power-of-two number of them)", who, C, prec);
    return NQA_E_SHAPE;
  }
  const bool planes = nchw != 0;
  *plan = group_stats_plan(R, K, &C, &HW, &planes, &prec, 1);
  if (scratch_bytes < plan->doubles * 8) {
    set_error("%s: scratch %zu < %zu bytes", who, scratch_bytes, plan->doubles * 8);
    return NQA_E_WORKSPACE;
  }
  double *part = static_cast<double *>(scratch);
  const size_t map_bytes = (size_t)HW * C * eb;
  const char *ren = static_cast<const char *>(feat) + (size_t)R * map_bytes;
  return nchw ? group_stats_nchw(static_cast<const float *>(feat), reinterpret_cast<const float *>(ren), R, K, C, HW, part, st)
              : group_stats_nhwc(feat, ren, R, K, HW, C, prec, part, st);
}

int nqa_dists_group_stats(const void *feat, int R, int K, int HW, int C, int prec, int nchw, void *scratch,
                          size_t scratch_bytes, float *s1, float *s2, void *stream) {
  if (!feat || !scratch || !s1 || !s2) {
    set_error("dists_group_stats: null pointer");
    return NQA_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  StatsPlan p;
  const int rc = group_stats_launch("dists_group_stats", feat, R, K, HW, C, prec, nchw, scratch, scratch_bytes, &p, st);
  if (rc) return rc;
  return finalize(static_cast<const double *>(scratch), p.d, R * K, s1, s2, st);
}

size_t nqa_stats_scratch_bytes(int B, const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS],
                               const int Wk[NQA_NUM_TAPS]) {
  if (B <= 0 || !C || !Hk || !Wk) return 0;
  int HW[6];
  for (int k = 0; k < 6; ++k) HW[k] = Hk[k] * Wk[k];
  return align_up(stats_plan(B, C, HW, nullptr, 6, NQA_PREC_F32).doubles * 8, 256);
}

int nqa_dists_stats_nchw(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B,
                         const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS], const int Wk[NQA_NUM_TAPS],
                         void *scratch, size_t scratch_bytes, float *s1, float *s2, void *stream) {
  if (!fx || !fy || !C || !Hk || !Wk || !scratch || !s1 || !s2 || B <= 0) {
    set_error("dists_stats_nchw: bad argument");
    return NQA_E_ARG;
  }
  int HW[6];
  for (int k = 0; k < 6; ++k) {
    if (!fx[k] || !fy[k] || C[k] <= 0 || Hk[k] <= 0 || Wk[k] <= 0) {
      set_error("dists_stats_nchw: bad feature %d", k);
      return NQA_E_ARG;
    }
    HW[k] = Hk[k] * Wk[k];
  }
  const StatsPlan p = stats_plan(B, C, HW, nullptr, 6, NQA_PREC_F32);
  if (scratch_bytes < p.doubles * 8) {
    set_error("dists_stats_nchw: scratch %zu < %zu bytes", scratch_bytes, p.doubles * 8);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(scratch);
  int rc;
  for (int k = 0; k < 6; ++k)
    if ((rc = stats_nchw(fx[k], fy[k], B, C[k], HW[k], part + p.d.part_off[k], st))) return rc;
  return finalize(part, p.d, B, s1, s2, st);
}

// ---- backward of nqa_dists_stats_nchw (forward_from_feats under autograd) ----
size_t nqa_stats_backward_bytes(int B, const int C[NQA_NUM_TAPS]) {
  if (B <= 0 || !C) return 0;
  long ctot = 0;
  for (int k = 0; k < 6; ++k) {
    if (C[k] <= 0) return 0;
    ctot += C[k];
  }
  return align_up((size_t)B * ctot * 6 * sizeof(double), 256);
}

int nqa_dists_stats_nchw_backward(const float *const fx[NQA_NUM_TAPS], const float *const fy[NQA_NUM_TAPS], int B,
                                  const int C[NQA_NUM_TAPS], const int Hk[NQA_NUM_TAPS], const int Wk[NQA_NUM_TAPS],
                                  const void *fwd_scratch, size_t fwd_bytes, const float *g_s1, const float *g_s2,
                                  void *coef, size_t coef_bytes, float *const gx[NQA_NUM_TAPS],
                                  float *const gy[NQA_NUM_TAPS], void *stream) {
  if (!fx || !fy || !C || !Hk || !Wk || !fwd_scratch || !g_s1 || !g_s2 || !coef || !gx || !gy || B <= 0) {
    set_error("dists_stats_nchw_backward: bad argument (null pointer or B <= 0)");
    return NQA_E_ARG;
  }
  int HW[6];
  for (int k = 0; k < 6; ++k) {
    if (!fx[k] || !fy[k] || C[k] <= 0 || Hk[k] <= 0 || Wk[k] <= 0) {
      set_error("dists_stats_nchw_backward: bad feature %d", k);
      return NQA_E_ARG;
    }
    if ((long)Hk[k] * Wk[k] > (1L << 30)) {  // (the gradient kernel's in-plane offsets are 32-bit)
      set_error("dists_stats_nchw_backward: feature %d has %ld > 2^30 pixels per plane", k, (long)Hk[k] * Wk[k]);
      return NQA_E_SHAPE;
    }
    HW[k] = Hk[k] * Wk[k];
  }
  const StatsPlan p = stats_plan(B, C, HW, nullptr, 6, NQA_PREC_F32);
  if (fwd_bytes < p.doubles * 8) {
    set_error("dists_stats_nchw_backward: forward scratch %zu < %zu bytes", fwd_bytes, p.doubles * 8);
    return NQA_E_WORKSPACE;
  }
  const size_t need = nqa_stats_backward_bytes(B, C);
  if (coef_bytes < need) {
    set_error("dists_stats_nchw_backward: coefficient buffer %zu < %zu bytes", coef_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *cf = static_cast<double *>(coef);
  int rc;
  if ((rc = stats_coef(static_cast<const double *>(fwd_scratch), p.d, B, g_s1, g_s2, cf, st))) return rc;
  return stats_grad(fx, fy, B, C, HW, cf, gx, gy, st);
}

// ---- conv + L2-pool + statistics as a single operator (tests, tools; the DISTS path calls the launcher directly) ----
static __global__ void part_reduce_kernel(const double *__restrict__ part, int nblk, int C, double *__restrict__ sums, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // (b, c, s)
  if (idx >= total) return;
  const long per = (long)C * 5;
  const long b = idx / per, cs = idx - b * per;
  double acc = 0.0;
  for (int k = 0; k < nblk; ++k) acc += part[((size_t)b * nblk + k) * per + cs];
  sums[idx] = acc;
}

static int fused_part_rows(int layer) { return layer == 1 ? NQA_FUSED_PART_BLOCKS_S1 : NQA_FUSED_PART_BLOCKS; }
int nqa_dists_fused_taps(int B, int H, int W, int prec, int fused[6]) {
  if (!fused) return NQA_E_ARG;
  if (bad_dims("dists_fused_taps", B, H, W, prec, 0, true)) return NQA_E_ARG;
  bool f[6];
  dists_fused_taps(B, H, W, prec, f);
  for (int k = 0; k < 6; ++k) fused[k] = f[k] ? 1 : 0;
  return NQA_OK;
}
size_t nqa_conv_pool_workspace_bytes(int B, int H, int W, int layer) {
  if (B <= 0 || H <= 0 || W <= 0 || layer < 1 || layer >= NQA_NUM_CONVS) return 0;
  const int C = kConvs[layer].cout;
  return align_up((size_t)B * fused_part_rows(layer) * C * 5 * sizeof(double), 256) + conv_pool_seam_bytes(B, H, W, C);
}

int nqa_conv1_pool_stats(const float *x, const float *y, int B, int H, int W, const void *packed, int prec, void *pooled,
                         double *sums, void *ws, size_t ws_bytes, void *stream) {
  if (!x || !y || !packed || !pooled || !sums || !ws || B <= 0 || H <= 0 || W <= 0) {
    set_error("conv1_pool_stats: bad argument");
    return NQA_E_ARG;
  }
  if (!conv1_pool_fusable(B, H, W, prec)) {
    set_error("conv1_pool_stats: no fused stage 1 for %d x %d frames in precision %d (B = %d)", H, W, prec, B);
    return NQA_E_SHAPE;
  }
  if (ws_bytes < nqa_conv_pool_workspace_bytes(B, H, W, 1)) {
    set_error("conv1_pool_stats: workspace %zu < %zu bytes", ws_bytes, nqa_conv_pool_workspace_bytes(B, H, W, 1));
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(ws);
  float *seam = reinterpret_cast<float *>(static_cast<char *>(ws) +
                                          align_up((size_t)B * NQA_FUSED_PART_BLOCKS_S1 * 64 * 5 * sizeof(double), 256));
  const int rc = conv1_pool_stats_fused(x, y, B, H, W, packed, pooled, seam, part, st);
  if (rc) return rc;
  const long total = (long)B * 64 * 5;
  part_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(part, NQA_FUSED_PART_BLOCKS_S1, 64, sums, total);
  return check_launch("part_reduce");
}

int nqa_conv_pool_stats(const void *in, int B, int H, int W, int layer, const void *packed, int prec, void *pooled,
                        double *sums, void *ws, size_t ws_bytes, void *stream) {
  if (!in || !packed || !pooled || !sums || !ws) {
    set_error("conv_pool_stats: null pointer");
    return NQA_E_ARG;
  }
  if (layer < 1 || layer >= NQA_NUM_CONVS || B <= 0 || H <= 0 || W <= 0 || !prec_valid_pyramid(prec)) {
    set_error("conv_pool_stats: bad argument (layer %d, B %d, %d x %d, prec %d)", layer, B, H, W, prec);
    return NQA_E_ARG;
  }
  const int kp = stage_prec(prec, kConvs[layer].stage);
  if (!conv_pool_fusable(layer, B, H, W, prec, kp)) {
    set_error("conv_pool_stats: no fused form for layer %d of a %d x %d map in precision %d (B = %d)", layer, H, W, prec, B);
    return NQA_E_SHAPE;
  }
  if (ws_bytes < nqa_conv_pool_workspace_bytes(B, H, W, layer)) {
    set_error("conv_pool_stats: workspace %zu < %zu bytes", ws_bytes, nqa_conv_pool_workspace_bytes(B, H, W, layer));
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = kConvs[layer].cout;
  double *part = static_cast<double *>(ws);
  float *seam = reinterpret_cast<float *>(static_cast<char *>(ws) + align_up((size_t)B * NQA_FUSED_PART_BLOCKS * C * 5 * sizeof(double), 256));
  const int rc = conv_pool_stats_fused(in, B, H, W, layer, packed, prec, pooled, seam, part, st);
  if (rc) return rc;
  const long total = (long)B * C * 5;
  part_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(part, NQA_FUSED_PART_BLOCKS, C, sums, total);
  return check_launch("part_reduce");
}

// ---- the pair path's pool + statistics pass and its last-tap statistics pass as single operators (tests, tools; the
// forwards call the launchers directly).  The launchers run unchanged; part_reduce_kernel folds their partials. ----
static const int kPairStatsMaxPairs = 65535;  // (stats_nhwc_kernel's grid.y)
// every host-side check the three entries share; HW: the pixels of one input map
static int pair_stats_bad(const char *who, int B, int H, int W, int C, int prec, bool split16_out) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) {
    set_error("%s: non-positive size B=%d H=%d W=%d C=%d", who, B, H, W, C);
    return NQA_E_ARG;
  }
  if (!prec_valid(prec)) {
    set_error(is_mixed(prec) ? "%s: takes no mixed mode (prec %d): pass the kernel precision of the map's own stage"
                             : "%s: unknown prec %d", who, prec);
    return NQA_E_ARG;
  }
  if (B > kPairStatsMaxPairs) {
    set_error("%s: B = %d pairs, at most %d in one call", who, B, kPairStatsMaxPairs);
    return NQA_E_ARG;
  }
  const long eb = (long)prec_elem_bytes(prec);
  if ((long)H * W > ((1L << 31) - 1) / ((long)C * eb)) {  // (no product of all four: that could overflow)
    set_error("%s: map too large (H*W*%d channels*%d bytes >= 2^31)", who, C, (int)eb);
    return NQA_E_ARG;
  }
  const int cpc = (int)(16 / eb), G = C / cpc;  // a thread owns one 16-byte channel group; 256 / G pixels side by side
  if (C % cpc || G > 256 || (G & (G - 1)) || (split16_out && C % 16)) {
    set_error("%s: no kernel for C=%d in prec %d (whole 16-byte channel groups, a power-of-two number of them up to 256%s)",
              who, C, prec, split16_out ? ", whole 16-channel split16 records" : "");
    return NQA_E_SHAPE;
  }
  return NQA_OK;
}
static int pool_stats_plan(int B, int H, int W, int C, int prec, int *tr, int *tc) {
  return pool_stats_tiles((H + 1) / 2, (W + 1) / 2, C, prec, B, tr, tc);
}

size_t nqa_pool_stats_workspace_bytes(int B, int H, int W, int C, int prec) {
  if (pair_stats_bad("pool_stats_workspace_bytes", B, H, W, C, prec, prec == NQA_PREC_F32S)) return 0;
  return align_up((size_t)B * pool_stats_plan(B, H, W, C, prec, nullptr, nullptr) * C * 5 * sizeof(double), 256);
}
size_t nqa_stats_nhwc_workspace_bytes(int B, int HW, int C, int prec) {
  if (pair_stats_bad("stats_nhwc_workspace_bytes", B, HW, 1, C, prec, false)) return 0;
  return align_up((size_t)B * cdiv(HW, stats_units_per_block(HW, C, prec, B)) * C * 5 * sizeof(double), 256);
}

int nqa_pool_stats_grid(int B, int H, int W, int C, int prec, int out[5]) {
  if (!out) {
    set_error("pool_stats_grid: null pointer");
    return NQA_E_ARG;
  }
  const int rc = pair_stats_bad("pool_stats_grid", B, H, W, C, prec, prec == NQA_PREC_F32S);
  if (rc) return rc;
  int TR, TC;
  const int nblk = pool_stats_plan(B, H, W, C, prec, &TR, &TC);
  out[0] = TR;
  out[1] = TC;
  out[2] = cdiv((W + 1) / 2, TC);
  out[3] = nblk;
  out[4] = nblk * B;
  return NQA_OK;
}
int nqa_stats_nhwc_grid(int B, int HW, int C, int prec, int out[3]) {
  if (!out) {
    set_error("stats_nhwc_grid: null pointer");
    return NQA_E_ARG;
  }
  const int rc = pair_stats_bad("stats_nhwc_grid", B, HW, 1, C, prec, false);
  if (rc) return rc;
  out[0] = stats_units_per_block(HW, C, prec, B);
  out[1] = cdiv(HW, out[0]);
  out[2] = 256 / (C / (int)(16 / prec_elem_bytes(prec)));
  return NQA_OK;
}

static int fold_partials(const double *part, int B, int nblk, int C, double *sums, hipStream_t st) {
  const long total = (long)B * C * 5;
  part_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(part, nblk, C, sums, total);
  return check_launch("part_reduce");
}
static int pool_stats_entry(const char *who, const void *feat, int B, int H, int W, int C, int prec, bool to_split16,
                            void *pooled, double *sums, void *ws, size_t ws_bytes, void *stream) {
  if (!feat || !pooled || !sums || !ws) {
    set_error("%s: null pointer", who);
    return NQA_E_ARG;
  }
  int rc = pair_stats_bad(who, B, H, W, C, prec, to_split16 || prec == NQA_PREC_F32S);
  if (rc) return rc;
  const int nblk = pool_stats_plan(B, H, W, C, prec, nullptr, nullptr);
  if ((long)nblk * B > 0x7fffffffL) {
    set_error("%s: %d tiles x %d pairs do not fit the launch grid", who, nblk, B);
    return NQA_E_SHAPE;
  }
  const size_t need = (size_t)B * nblk * C * 5 * sizeof(double);
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(ws);
  rc = to_split16 ? pool_stats_to_split16(feat, B, H, W, C, pooled, part, st) : pool_stats(feat, B, H, W, C, prec, pooled, part, st);
  if (rc) return rc;
  return fold_partials(part, B, nblk, C, sums, st);
}

int nqa_pool_stats(const void *feat, int B, int H, int W, int C, int prec, void *pooled, double *sums, void *ws,
                   size_t ws_bytes, void *stream) {
  return pool_stats_entry("pool_stats", feat, B, H, W, C, prec, false, pooled, sums, ws, ws_bytes, stream);
}
int nqa_pool_stats_f16_to_split16(const void *feat_f16, int B, int H, int W, int C, void *pooled_split16, double *sums,
                                  void *ws, size_t ws_bytes, void *stream) {
  return pool_stats_entry("pool_stats_f16_to_split16", feat_f16, B, H, W, C, NQA_PREC_F16, true, pooled_split16, sums, ws,
                          ws_bytes, stream);
}
int nqa_stats_nhwc(const void *feat, int B, int HW, int C, int prec, double *sums, void *ws, size_t ws_bytes,
                   void *stream) {
  if (!feat || !sums || !ws) {
    set_error("stats_nhwc: null pointer");
    return NQA_E_ARG;
  }
  int rc = pair_stats_bad("stats_nhwc", B, HW, 1, C, prec, false);
  if (rc) return rc;
  const int nblk = cdiv(HW, stats_units_per_block(HW, C, prec, B));
  const size_t need = (size_t)B * nblk * C * 5 * sizeof(double);
  if (ws_bytes < need) {
    set_error("stats_nhwc: workspace %zu < %zu bytes", ws_bytes, need);
    return NQA_E_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(ws);
  if ((rc = stats_nhwc(feat, B, HW, C, prec, part, st))) return rc;
  return fold_partials(part, B, nblk, C, sums, st);
}

// ---- the group statistics' five sums and plan (tests, tools): nqa_dists_group_stats' launch, folded instead of finalised ----
int nqa_dists_group_sums(const void *feat, int R, int K, int HW, int C, int prec, int nchw, void *scratch,
                         size_t scratch_bytes, double *sums, void *stream) {
  if (!feat || !scratch || !sums) {
    set_error("dists_group_sums: null pointer");
    return NQA_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  StatsPlan p;
  const int rc = group_stats_launch("dists_group_sums", feat, R, K, HW, C, prec, nchw, scratch, scratch_bytes, &p, st);
  if (rc) return rc;
  return fold_partials(static_cast<const double *>(scratch), R * K, p.d.nblk[0], C, sums, st);
}
int nqa_dists_group_stats_grid(int R, int K, int HW, int C, int prec, int nchw, int out[4]) {
  if (!out) {
    set_error("dists_group_stats_grid: null pointer");
    return NQA_E_ARG;
  }
  if (bad_group("dists_group_stats_grid", R, K)) return NQA_E_ARG;
  if (HW <= 0 || C <= 0) {
    set_error("dists_group_stats_grid: non-positive size HW=%d C=%d", HW, C);
    return NQA_E_ARG;
  }
  if (!prec_valid(prec)) {
    set_error("dists_group_stats_grid: prec %d is not one of the kernel-level modes", prec);
    return NQA_E_ARG;
  }
  if (!nchw && !group_stats_nhwc_ok(C, prec)) {
    set_error("dists_group_stats_grid: no NHWC kernel for C=%d in prec %d", C, prec);
    return NQA_E_SHAPE;
  }
  out[0] = nchw ? stats_nchw_ppb(HW) : group_stats_units_per_block(HW, C, prec, R);
  out[1] = cdiv(HW, out[0]);
  out[2] = nchw ? 256 : 256 / (C / (int)(16 / prec_elem_bytes(prec)));
  out[3] = cdiv(out[0] < HW ? out[0] : HW, out[2]);
  return NQA_OK;
}

int nqa_dists_score(const float *s1, const float *s2, const float *alpha, const float *beta, int B, float *out,
                    void *stream) {
  if (!s1 || !s2 || !alpha || !beta || !out || B <= 0) {
    set_error("dists_score: bad argument");
    return NQA_E_ARG;
  }
  return score(s1, s2, alpha, beta, B, out, static_cast<hipStream_t>(stream));
}


// ---- backward pass (DISTS require_grad=True; nqa_backward.hip) -----------------------------------------------------
int nqa_conv3x3_split(const void *in_split16, int n, int H, int W, int cin, int cout, const void *packed_conv, int relu,
                      float *out_nhwc, void *stream) {
  if (!in_split16 || !packed_conv || !out_nhwc) {
    set_error("conv3x3_split: null pointer");
    return NQA_E_ARG;
  }
  if (cout <= 0 || cin <= 0 || cout % 64 || cin % 16) {
    set_error("conv3x3_split: cout %d must be a multiple of 64, cin %d of 16", cout, cin);
    return NQA_E_SHAPE;
  }
  if (bad_dims("conv3x3_split", n, H, W, NQA_PREC_F32S, cin > cout ? cin : cout)) return NQA_E_ARG;
  return conv3x3_split_generic(in_split16, n, H, W, cin, cout, packed_conv, conv_split_bias_off(cout, cin), relu,
                               out_nhwc, static_cast<hipStream_t>(stream));
}

int nqa_relu_mask_split16(const float *g_nhwc, const void *act_nhwc, int act_is_split16, long pixels, int C,
                          void *out_split16, void *stream) {
  if (!g_nhwc || !act_nhwc || !out_split16 || pixels <= 0 || C <= 0 || C % 16) {
    set_error("relu_mask_split16: bad argument (C %d must be a positive multiple of 16)", C);
    return NQA_E_ARG;
  }
  return relu_mask_split16(g_nhwc, act_nhwc, act_is_split16, pixels, C, out_split16, static_cast<hipStream_t>(stream));
}

int nqa_l2pool_backward(const float *tap_nhwc, const void *pooled_split16, const float *g_pooled_nhwc, int n, int H, int W,
                        int C, float *g_tap_nhwc, void *stream) {
  if (!tap_nhwc || !pooled_split16 || !g_pooled_nhwc || !g_tap_nhwc || C <= 0 || C % 16) {
    set_error("l2pool_backward: bad argument");
    return NQA_E_ARG;
  }
  if (bad_dims("l2pool_backward", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  return l2pool_backward(tap_nhwc, pooled_split16, g_pooled_nhwc, n, H, W, C, g_tap_nhwc, static_cast<hipStream_t>(stream));
}

int nqa_conv1_1_backward(const float *gm_nhwc, const float *w_oihw_dev, int n, int H, int W, float *g_image_nchw,
                         void *stream) {
  if (!gm_nhwc || !w_oihw_dev || !g_image_nchw) {
    set_error("conv1_1_backward: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("conv1_1_backward", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  return conv1_1_backward(gm_nhwc, w_oihw_dev, n, H, W, g_image_nchw, static_cast<hipStream_t>(stream));
}

// ---- DISTS as a loss (nqa_loss_backward.hip and the scaled forms of nqa_backward.hip) -------------------------------
static bool loss_bad_c(int C) { return C < 16 || C > 1024 || C % 16 || 256 % (C / 4); }

size_t nqa_dists_stats_nhwc_backward_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || loss_bad_c(C) || (long)H * W > (1L << 30)) return 0;
  return align_up(loss_stats_backward_doubles(B, H * W, C) * sizeof(double), 256);
}

int nqa_dists_stats_nhwc_backward(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C, const float *g_s1,
                                  const float *g_s2, long g_stride, void *workspace, size_t workspace_bytes, float *gx_nhwc,
                                  float *gy_nhwc, void *stream) {
  if (!tx_nhwc || !ty_nhwc || !g_s1 || !g_s2 || !workspace || (!gx_nhwc && !gy_nhwc) || B <= 0 || B > 65535 || H <= 0 ||
      W <= 0 || g_stride < C) {
    set_error("dists_stats_nhwc_backward: bad argument (null pointer, no gradient to write, B %d outside 1..65535, "
              "%d x %d, or g_stride %ld < C %d)", B, H, W, g_stride, C);
    return NQA_E_ARG;
  }
  if (loss_bad_c(C)) {
    set_error("dists_stats_nhwc_backward: C %d must be a power of two in 16..1024", C);
    return NQA_E_SHAPE;
  }
  if ((long)H * W > (1L << 30)) {
    set_error("dists_stats_nhwc_backward: %ld > 2^30 pixels per image", (long)H * W);
    return NQA_E_SHAPE;
  }
  if (((uintptr_t)tx_nhwc | (uintptr_t)ty_nhwc | (uintptr_t)gx_nhwc | (uintptr_t)gy_nhwc) & 15) {
    set_error("dists_stats_nhwc_backward: the maps must be 16-byte aligned");
    return NQA_E_ARG;
  }
  const size_t need = nqa_dists_stats_nhwc_backward_bytes(B, H, W, C);
  if (workspace_bytes < need) {
    set_error("dists_stats_nhwc_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return loss_stats_backward(tx_nhwc, ty_nhwc, B, H * W, C, g_s1, g_s2, g_stride, static_cast<double *>(workspace), gx_nhwc,
                             gy_nhwc, static_cast<hipStream_t>(stream));
}

// ---- the same statistics for a loss against a prepared target: the forward keeps the sums, the backward starts there ----
// What the two entry points below check alike; 0 or the error code, with the message set under `who`.
static int loss_target_bad(const char *who, bool null_ptr, int B, int H, int W, int C, long stride, uintptr_t maps) {
  if (null_ptr || B <= 0 || B > 65535 || H <= 0 || W <= 0 || stride < C) {
    set_error("%s: bad argument (null pointer, B %d outside 1..65535, %d x %d, or stride %ld < C %d)", who, B, H, W, stride,
              C);
    return NQA_E_ARG;
  }
  if (loss_bad_c(C)) {
    set_error("%s: C %d must be a power of two in 16..1024", who, C);
    return NQA_E_SHAPE;
  }
  if ((long)H * W > (1L << 30)) {
    set_error("%s: %ld > 2^30 pixels per image", who, (long)H * W);
    return NQA_E_SHAPE;
  }
  if (maps & 15) {
    set_error("%s: the maps must be 16-byte aligned, the fp64 buffers 8-byte", who);
    return NQA_E_ARG;
  }
  return NQA_OK;
}

size_t nqa_dists_stats_target_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || loss_bad_c(C) || (long)H * W > (1L << 30)) return 0;
  return loss_stats_partials_doubles(B, H * W, C) * sizeof(double);
}

int nqa_dists_stats_target(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C, void *partials,
                           size_t partials_bytes, float *s1, float *s2, long s_stride, void *stream) {
  const char *who = "dists_stats_target";
  if (int rc = loss_target_bad(who, !tx_nhwc || !ty_nhwc || !partials || !s1 || !s2, B, H, W, C, s_stride,
                               (uintptr_t)tx_nhwc | (uintptr_t)ty_nhwc | ((uintptr_t)partials & 7)))
    return rc;
  const size_t need = nqa_dists_stats_target_bytes(B, H, W, C);
  if (partials_bytes < need) {
    set_error("%s: partials %zu < %zu bytes", who, partials_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return loss_stats_target(tx_nhwc, ty_nhwc, B, H * W, C, static_cast<double *>(partials), s1, s2, s_stride,
                           static_cast<hipStream_t>(stream));
}

size_t nqa_dists_stats_nhwc_backward_from_bytes(int B, int C) {
  if (B <= 0 || loss_bad_c(C)) return 0;
  return align_up(loss_stats_coef_doubles(B, C) * sizeof(double), 256);
}

int nqa_dists_stats_nhwc_backward_from(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C,
                                       const void *partials, size_t partials_bytes, const float *g_s1, const float *g_s2,
                                       long g_stride, void *coef, size_t coef_bytes, float *gx_nhwc, float *gy_nhwc,
                                       void *stream) {
  const char *who = "dists_stats_nhwc_backward_from";
  if (int rc = loss_target_bad(who, !tx_nhwc || !ty_nhwc || !partials || !g_s1 || !g_s2 || !coef || (!gx_nhwc && !gy_nhwc), B,
                               H, W, C, g_stride,
                               (uintptr_t)tx_nhwc | (uintptr_t)ty_nhwc | (uintptr_t)gx_nhwc | (uintptr_t)gy_nhwc |
                                   (((uintptr_t)partials | (uintptr_t)coef) & 7)))
    return rc;
  const size_t need_part = nqa_dists_stats_target_bytes(B, H, W, C);
  if (partials_bytes < need_part) {
    set_error("%s: partials %zu < %zu bytes", who, partials_bytes, need_part);
    return NQA_E_WORKSPACE;
  }
  const size_t need = nqa_dists_stats_nhwc_backward_from_bytes(B, C);
  if (coef_bytes < need) {
    set_error("%s: coefficient buffer %zu < %zu bytes", who, coef_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return loss_stats_backward_from(tx_nhwc, ty_nhwc, B, H * W, C, static_cast<const double *>(partials), g_s1, g_s2, g_stride,
                                  static_cast<double *>(coef), gx_nhwc, gy_nhwc, static_cast<hipStream_t>(stream));
}

int nqa_dists_stats_nhwc_grad_y_add(const float *tx_nhwc, const float *ty_nhwc, int B, int H, int W, int C,
                                    const void *partials, size_t partials_bytes, const float *g_s1, const float *g_s2,
                                    long g_stride, void *coef, size_t coef_bytes, float *gy_inout, void *stream) {
  const char *who = "dists_stats_nhwc_grad_y_add";
  if (int rc = loss_target_bad(who, !tx_nhwc || !ty_nhwc || !partials || !g_s1 || !g_s2 || !coef || !gy_inout, B, H, W, C,
                               g_stride,
                               (uintptr_t)tx_nhwc | (uintptr_t)ty_nhwc | (uintptr_t)gy_inout |
                                   (((uintptr_t)partials | (uintptr_t)coef) & 7)))
    return rc;
  const size_t need_part = nqa_dists_stats_target_bytes(B, H, W, C);
  if (partials_bytes < need_part) {
    set_error("%s: partials %zu < %zu bytes", who, partials_bytes, need_part);
    return NQA_E_WORKSPACE;
  }
  const size_t need = nqa_dists_stats_nhwc_backward_from_bytes(B, C);
  if (coef_bytes < need) {
    set_error("%s: coefficient buffer %zu < %zu bytes", who, coef_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return loss_stats_grad_y_add(tx_nhwc, ty_nhwc, B, H * W, C, static_cast<const double *>(partials), g_s1, g_s2, g_stride,
                               static_cast<double *>(coef), gy_inout, static_cast<hipStream_t>(stream));
}

size_t nqa_grad_exponent_bytes(int n, long per_image) {
  if (n <= 0 || per_image <= 0 || per_image % 4) return 0;
  return align_up((size_t)n * grad_exponent_nblk(per_image) * sizeof(unsigned), 256);
}

int nqa_grad_exponent(const float *g, int n, long per_image, void *workspace, size_t workspace_bytes, int *k, int *k_total,
                      void *stream) {
  if (!g || !workspace || !k || n <= 0 || n > 65535 || per_image <= 0) {
    set_error("grad_exponent: bad argument (null pointer, n %d outside 1..65535 or per_image %ld <= 0)", n, per_image);
    return NQA_E_ARG;
  }
  if (per_image % 4 || ((uintptr_t)g & 15)) {
    set_error("grad_exponent: per_image %ld must be a multiple of 4 and g 16-byte aligned", per_image);
    return NQA_E_SHAPE;
  }
  const size_t need = nqa_grad_exponent_bytes(n, per_image);
  if (workspace_bytes < need) {
    set_error("grad_exponent: workspace %zu < %zu bytes", workspace_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return grad_exponent(g, n, per_image, static_cast<unsigned *>(workspace), k, k_total, static_cast<hipStream_t>(stream));
}

int nqa_relu_mask_split16_scaled(const float *g_nhwc, const void *act_nhwc, int act_is_split16, int n,
                                 long pixels_per_image, int C, const int *k, void *out_split16, void *stream) {
  if (!g_nhwc || !act_nhwc || !k || !out_split16 || n <= 0 || pixels_per_image <= 0 || C <= 0 || C % 16) {
    set_error("relu_mask_split16_scaled: bad argument (null pointer, n %d, %ld pixels, C %d must be a positive multiple of 16)",
              n, pixels_per_image, C);
    return NQA_E_ARG;
  }
  return relu_mask_split16_scaled(g_nhwc, act_nhwc, act_is_split16, n, pixels_per_image, C, k, out_split16,
                                  static_cast<hipStream_t>(stream));
}

int nqa_l2pool_backward_scaled(const float *tap_nhwc, const float *g_pooled_nhwc, const float *g_tap_nhwc, const int *k_total,
                               int n, int H, int W, int C, float *out_nhwc, void *stream) {
  if (!tap_nhwc || !g_pooled_nhwc || !g_tap_nhwc || !k_total || !out_nhwc || C <= 0 || C % 16) {
    set_error("l2pool_backward_scaled: bad argument");
    return NQA_E_ARG;
  }
  if (bad_dims("l2pool_backward_scaled", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  return l2pool_backward_scaled(tap_nhwc, g_pooled_nhwc, g_tap_nhwc, k_total, n, H, W, C, out_nhwc,
                                static_cast<hipStream_t>(stream));
}

int nqa_conv1_1_backward_scaled(const float *g_nhwc, const void *relu1_1_split16, const float *w_oihw_dev, const int *k,
                                const int *k_total, int n, int H, int W, float *g_image_nchw, void *stream) {
  if (!g_nhwc || !w_oihw_dev || !k || !k_total || !g_image_nchw) {
    set_error("conv1_1_backward_scaled: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("conv1_1_backward_scaled", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  return conv1_1_backward_scaled(g_nhwc, relu1_1_split16, w_oihw_dev, k, k_total, n, H, W, g_image_nchw,
                                 static_cast<hipStream_t>(stream));
}

// ---- the half gradient chain (grad_precision "f16"; nqa_backward.hip, nqa_loss_backward.hip, conv3x3_half_generic) ----
int nqa_conv3x3_half(const void *in_f16_nhwc, int n, int H, int W, int cin, int cout, const void *packed_conv,
                     void *out_f16_nhwc, void *stream) {
  if (!in_f16_nhwc || !packed_conv || !out_f16_nhwc) {
    set_error("conv3x3_half: null pointer");
    return NQA_E_ARG;
  }
  if (cout <= 0 || cin <= 0 || cout % 64 || cin % 32) {
    set_error("conv3x3_half: cout %d must be a multiple of 64, cin %d of 32", cout, cin);
    return NQA_E_SHAPE;
  }
  if (bad_dims("conv3x3_half", n, H, W, NQA_PREC_F16, cin > cout ? cin : cout)) return NQA_E_ARG;
  if (((uintptr_t)in_f16_nhwc | (uintptr_t)out_f16_nhwc | (uintptr_t)packed_conv) & 15) {
    set_error("conv3x3_half: the maps and the packed layer must be 16-byte aligned");
    return NQA_E_ARG;
  }
  return conv3x3_half_generic(in_f16_nhwc, n, H, W, cin, cout, packed_conv, conv_half_bias_off(cout, cin), out_f16_nhwc,
                              static_cast<hipStream_t>(stream));
}

int nqa_relu_mask_f16_scaled(const void *g_nhwc, int g_is_half, const void *act_nhwc, int act_is_split16, int n,
                             long pixels_per_image, int C, const int *k, void *out_f16, void *stream) {
  if (!g_nhwc || !act_nhwc || !k || !out_f16 || n <= 0 || pixels_per_image <= 0) {
    set_error("relu_mask_f16_scaled: bad argument (null pointer, n %d or %ld pixels per image not positive)", n,
              pixels_per_image);
    return NQA_E_ARG;
  }
  if (C <= 0 || C % 16) {
    set_error("relu_mask_f16_scaled: C %d must be a positive multiple of 16", C);
    return NQA_E_SHAPE;
  }
  if (((uintptr_t)g_nhwc | (uintptr_t)act_nhwc | (uintptr_t)out_f16) & 15) {
    set_error("relu_mask_f16_scaled: the maps must be 16-byte aligned");
    return NQA_E_ARG;
  }
  if ((long)n * pixels_per_image > (1L << 31) * 256 / (C / 8)) {  // (the grid is one 32-bit count of 256-thread blocks)
    set_error("relu_mask_f16_scaled: %d x %ld pixels of %d channels are more than one launch takes", n, pixels_per_image, C);
    return NQA_E_SHAPE;
  }
  return relu_mask_f16_scaled(g_nhwc, g_is_half != 0, act_nhwc, act_is_split16, n, pixels_per_image, C, k, out_f16,
                              static_cast<hipStream_t>(stream));
}

int nqa_grad_exponent_half(const void *g, int g_is_half, int n, long per_image, void *workspace, size_t workspace_bytes,
                           int *k, int *k_total, void *stream) {
  if (!g || !workspace || !k || n <= 0 || n > 65535 || per_image <= 0 || ((uintptr_t)g & 15)) {
    set_error("grad_exponent_half: bad argument (null pointer, g not 16-byte aligned, n %d outside 1..65535 or per_image "
              "%ld <= 0)", n, per_image);
    return NQA_E_ARG;
  }
  if (per_image % (g_is_half ? 8 : 4)) {
    set_error("grad_exponent_half: per_image %ld must be a multiple of %d", per_image, g_is_half ? 8 : 4);
    return NQA_E_SHAPE;
  }
  const size_t need = nqa_grad_exponent_bytes(n, per_image);
  if (workspace_bytes < need) {
    set_error("grad_exponent_half: workspace %zu < %zu bytes", workspace_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return grad_exponent_half(g, g_is_half != 0, n, per_image, static_cast<unsigned *>(workspace), k, k_total,
                            static_cast<hipStream_t>(stream));
}

int nqa_l2pool_backward_scaled_half(const float *tap_nhwc, const void *g_pooled_f16, const float *g_tap_nhwc,
                                    const int *k_total, int n, int H, int W, int C, float *out_nhwc, void *stream) {
  if (!tap_nhwc || !g_pooled_f16 || !g_tap_nhwc || !k_total || !out_nhwc) {
    set_error("l2pool_backward_scaled_half: null pointer");
    return NQA_E_ARG;
  }
  if (C <= 0 || C % 16) {
    set_error("l2pool_backward_scaled_half: C %d must be a positive multiple of 16", C);
    return NQA_E_SHAPE;
  }
  if (bad_dims("l2pool_backward_scaled_half", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  if ((((uintptr_t)tap_nhwc | (uintptr_t)g_tap_nhwc | (uintptr_t)out_nhwc) & 15) || ((uintptr_t)g_pooled_f16 & 7)) {
    set_error("l2pool_backward_scaled_half: the float maps must be 16-byte aligned, the half map 8-byte");
    return NQA_E_ARG;
  }
  return l2pool_backward_scaled_half(tap_nhwc, g_pooled_f16, g_tap_nhwc, k_total, n, H, W, C, out_nhwc,
                                     static_cast<hipStream_t>(stream));
}

int nqa_conv1_1_backward_scaled_half(const void *g_f16_nhwc, const void *relu1_1_split16, const float *w_oihw_dev,
                                     const int *k, const int *k_total, int n, int H, int W, float *g_image_nchw,
                                     void *stream) {
  if (!g_f16_nhwc || !w_oihw_dev || !k || !k_total || !g_image_nchw) {
    set_error("conv1_1_backward_scaled_half: null pointer");
    return NQA_E_ARG;
  }
  if (bad_dims("conv1_1_backward_scaled_half", n, H, W, NQA_PREC_F32, 0)) return NQA_E_ARG;
  if ((uintptr_t)g_f16_nhwc & 1) {
    set_error("conv1_1_backward_scaled_half: the half map must be 2-byte aligned");
    return NQA_E_ARG;
  }
  return conv1_1_backward_scaled_half(g_f16_nhwc, relu1_1_split16, w_oihw_dev, k, k_total, n, H, W, g_image_nchw,
                                      static_cast<hipStream_t>(stream));
}

// ---- windowed moments of the A-DISTS head (nqa_window_moments_n.hip, nqa_window_moments.hip) ------------------------
// One checked implementation per operation.  Each old name is its _n form at a window of 21 under its own name `who`,
// with MomentsKernels::Taps21 where the _n name passes Tuned; 21 cannot trip the window-range refusal.
static int window_bad_shape(const char *who, int P, int H, int W, int window) {
  if (P <= 0) {
    set_error("%s: bad argument (P %d <= 0)", who, P);
    return NQA_E_ARG;
  }
  if (int rc = window_check_n(who, window)) return rc;
  if (H < window || W < window) {
    set_error("%s: %d x %d is smaller than the %d x %d window", who, H, W, window, window);
    return NQA_E_SHAPE;
  }
  return 0;
}
// (checked after the pointers' alignment, so that what refuses a call can be told apart without a launch)
static int window_too_large(const char *who, int H, int W) {
  if (H > (1 << 20) || (long)H * W > (1L << 30)) {
    set_error("%s: %d x %d: H > 2^20 or more than 2^30 pixels per plane", who, H, W);
    return NQA_E_SHAPE;
  }
  return 0;
}

static int moments_forward(const char *who, int window, MomentsKernels kernels, const float *x, const float *y, int P,
                           int H, int W, float *out, void *stream) {
  if (!x || !out) {
    set_error("%s: bad argument (null pointer)", who);
    return NQA_E_ARG;
  }
  if (int rc = window_bad_shape(who, P, H, W, window)) return rc;
  if (W % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 15)) {  // (rows move as 16-byte accesses then)
    set_error("%s: with W %d a multiple of 4 the maps must be 16-byte aligned", who, W);
    return NQA_E_ARG;
  }
  if (int rc = window_too_large(who, H, W)) return rc;
  return window_moments_forward(x, y, P, H, W, window, kernels, out, static_cast<hipStream_t>(stream));
}

static int moments_backward(const char *who, int window, MomentsKernels kernels, const float *x, const float *y, int P,
                            int H, int W, const float *const (&g)[5], float *gx, float *gy, void *stream) {
  if (!x || (!gx && !gy) || (!y && (g[1] || g[3] || g[4] || gy))) {
    set_error("%s: bad argument (null pointer, no gradient to write, or y's terms given without y)", who);
    return NQA_E_ARG;
  }
  if (int rc = window_bad_shape(who, P, H, W, window)) return rc;
  if (W % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)g[0] | (uintptr_t)g[1] | (uintptr_t)g[2] |
                      (uintptr_t)g[3] | (uintptr_t)g[4] | (uintptr_t)gx | (uintptr_t)gy) & 15)) {
    set_error("%s: with W %d a multiple of 4 the maps must be 16-byte aligned", who, W);
    return NQA_E_ARG;
  }
  if (int rc = window_too_large(who, H, W)) return rc;
  return window_moments_backward(x, y, P, H, W, window, kernels, g, gx, gy, static_cast<hipStream_t>(stream));
}

int nqa_window_moments_forward(const float *x, const float *y, int P, int H, int W, float *out, void *stream) {
  return moments_forward("window_moments_forward", 21, MomentsKernels::Taps21, x, y, P, H, W, out, stream);
}

int nqa_window_moments_forward_n(const float *x, const float *y, int P, int H, int W, int window, float *out,
                                 void *stream) {
  return moments_forward("window_moments_forward_n", window, MomentsKernels::Tuned, x, y, P, H, W, out, stream);
}

int nqa_window_moments_backward(const float *x, const float *y, int P, int H, int W, const float *g0, const float *g1,
                                const float *g2, const float *g3, const float *g4, float *gx, float *gy, void *stream) {
  return moments_backward("window_moments_backward", 21, MomentsKernels::Taps21, x, y, P, H, W, {g0, g1, g2, g3, g4}, gx,
                          gy, stream);
}

int nqa_window_moments_backward_n(const float *x, const float *y, int P, int H, int W, int window, const float *g0,
                                  const float *g1, const float *g2, const float *g3, const float *g4, float *gx, float *gy,
                                  void *stream) {
  return moments_backward("window_moments_backward_n", window, MomentsKernels::Tuned, x, y, P, H, W, {g0, g1, g2, g3, g4},
                          gx, gy, stream);
}

// ---- one stage of the A-DISTS head's backward towards y (nqa_adists_backward.hip) ------------------------------------
// The refusals that depend on sizes alone; quiet (who null) for the _bytes query.
static int ts_bad_sizes(const char *who, int B, int C, int H, int W, int ctot, int coff, int out_nhwc, int window) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ctot <= 0 || coff < 0 || (long)coff + C > ctot || B > 65535) {
    if (who)
      set_error("%s: bad argument (B %d, C %d, H %d, W %d, ctot %d, coff %d: non-positive size, channels outside q, or "
                "more than 65535 pairs)", who, B, C, H, W, ctot, coff);
    return NQA_E_ARG;
  }
  if (H > (1 << 20) || (long)H * W > (1L << 30)) {
    if (who) set_error("%s: %d x %d: H > 2^20 or more than 2^30 pixels per plane", who, H, W);
    return NQA_E_SHAPE;
  }
  if (!adists_ts_backward_fits(B, C, H, W, window)) {
    if (who) set_error("%s: %d planes of %d x %d need more than 2^31 blocks in one launch (slice the batch)", who, B * C, H, W);
    return NQA_E_SHAPE;
  }
  if (out_nhwc && H >= window && W >= window && C % 32) {
    if (who) set_error("%s: an NHWC gradient of a windowed stage needs C %% 32 == 0, got C %d", who, C);
    return NQA_E_SHAPE;
  }
  return 0;
}

static size_t ts_backward_bytes(int window, int B, int C, int H, int W) {
  if (window < 3 || window > 63 || ts_bad_sizes(nullptr, B, C, H, W, C, 0, 0, window)) return 0;
  return adists_ts_backward_bytes(B, C, H, W, window);
}

static int ts_backward(const char *who, int window, MomentsKernels kernels, const float *x, const float *y, int B, int C,
                       int H, int W, const float *q, const float *wgt, int ctot, int coff, const float *ps, const float *u,
                       int mask, int out_nhwc, void *workspace, size_t workspace_bytes, float *gy, void *stream) {
  if (!x || !y || !q || !wgt || !ps || !u || !workspace || !gy) {
    set_error("%s: bad argument (null pointer)", who);
    return NQA_E_ARG;
  }
  if (int rc = window_check_n(who, window)) return rc;
  if (int rc = ts_bad_sizes(who, B, C, H, W, ctot, coff, out_nhwc, window)) return rc;
  // the windowed stage runs the planar window-moments kernels and inherits their rule; ps moves as 16-byte accesses
  // only where its planes of mh x mw floats are whole 16-byte rows too (always at 21); the workspace holds doubles
  const bool rows16 = W % 4 == 0 && H >= window && W >= window;
  const bool ps16 = rows16 && ((long)(H - window + 1) * (W - window + 1)) % 4 == 0;
  if (((uintptr_t)workspace & 15) || (rows16 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gy) & 15)) ||
      (ps16 && ((uintptr_t)ps & 15))) {
    set_error("%s: the workspace, and with W %d a multiple of 4 the maps, must be 16-byte aligned", who, W);
    return NQA_E_ARG;
  }
  const size_t need = adists_ts_backward_bytes(B, C, H, W, window);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return NQA_E_WORKSPACE;
  }
  return adists_ts_backward(x, y, B, C, H, W, window, kernels, q, wgt, ctot, coff, ps, u, mask != 0, out_nhwc != 0,
                            workspace, gy, static_cast<hipStream_t>(stream));
}

size_t nqa_adists_ts_backward_bytes(int B, int C, int H, int W) { return ts_backward_bytes(21, B, C, H, W); }

size_t nqa_adists_ts_backward_bytes_n(int B, int C, int H, int W, int window) {
  return ts_backward_bytes(window, B, C, H, W);
}

int nqa_adists_ts_backward(const float *x, const float *y, int B, int C, int H, int W, const float *q, const float *wgt,
                           int ctot, int coff, const float *ps, const float *u, int mask, int out_nhwc, void *workspace,
                           size_t workspace_bytes, float *gy, void *stream) {
  return ts_backward("adists_ts_backward", 21, MomentsKernels::Taps21, x, y, B, C, H, W, q, wgt, ctot, coff, ps, u, mask,
                     out_nhwc, workspace, workspace_bytes, gy, stream);
}

int nqa_adists_ts_backward_n(const float *x, const float *y, int B, int C, int H, int W, int window, const float *q,
                             const float *wgt, int ctot, int coff, const float *ps, const float *u, int mask,
                             int out_nhwc, void *workspace, size_t workspace_bytes, float *gy, void *stream) {
  return ts_backward("adists_ts_backward_n", window, MomentsKernels::Tuned, x, y, B, C, H, W, q, wgt, ctot, coff, ps, u,
                     mask, out_nhwc, workspace, workspace_bytes, gy, stream);
}

}  // extern "C"
