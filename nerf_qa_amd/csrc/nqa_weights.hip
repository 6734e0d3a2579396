// The packed weight blob, host code only: where every section lies (one walk per mode, the accessors of nqa_common.h
// read its table) and the packers that fill it -- one per weight format.  The format itself is described once, in
// nqa_common.h ("Packed weight blob"); tests/test_cpu_pack_digests.py holds every blob to recorded bytes.
#include <math.h>
#include <string.h>

#include "nqa_common.h"

namespace nqa {

// ---- layout -------------------------------------------------------------------------------------------------------------
static constexpr size_t kAlign = 256;                      // every section but the fragment areas starts on this
static constexpr size_t kW0Bytes = 27 * 64 * 4;            // conv1_1: float w[27][64]
static constexpr size_t kW1MfmaBytes = 3 * 64 * 2 * 8 * 2;  // conv1_1 as 32x32 fragments [ky][cout][h][8 halfs]
static constexpr size_t kW1M16Bytes = 4 * 2 * 64 * 8 * 2;   // conv1_1 as 16x16x32 fragments [4 tiles][2 MFMAs][64 lanes][8 halfs], per term
static const int kRegwFirst = 1, kRegwLast = 4;            // conv1_2, conv2_1 (Cin 64); conv2_2, conv3_1 (Cin 128)

static size_t rows_bytes(int cout, int cin, size_t weight_bytes) { return align_up((size_t)cout * cin * 9 * weight_bytes, kAlign); }
static size_t bias_bytes(int cout) { return align_up((size_t)cout * 4 + 4, kAlign); }  // float bias[cout], then 1 / weight scale

struct BlobLayout {
  size_t layer[NQA_NUM_CONVS];  // the layer's weights: floats (layer 0), rows (layers 1..12)
  size_t bias[NQA_NUM_CONVS];
  size_t w1_mfma;               // conv1_1, 32x32 fragments
  size_t regw[kRegwLast + 1];   // [kRegwFirst..kRegwLast]: the layer's register fragments
  size_t w1_m16;                // conv1_1, 16x16x32 fragments
  size_t bytes;
  // which fragment sections the mode carries: terms per weight in them (0: none, as in NQA_PREC_F32; 1: the 16-bit
  // modes; 2: (hi, lo), the mixed modes and NQA_PREC_F32S) and the last layer that has register fragments
  int frag_terms, regw_last;
};

// the sections of mode `prec` in blob order
static BlobLayout walk_layout(int prec) {
  BlobLayout L;
  memset(&L, 0, sizeof(L));
  const bool two_term = is_mixed(prec) || prec == NQA_PREC_F32S;
  L.frag_terms = two_term ? 2 : prec_elem_bytes(prec) == 2 ? 1 : 0;
  L.regw_last = !L.frag_terms ? 0 : prec == NQA_PREC_F32S ? kRegwFirst + 1 : kRegwLast;  // (f32s: conv1_2, conv2_1)
  // bytes per weight of the rows: a mixed mode holds f16 (hi, lo) pairs up to its boundary and f32s rows behind it
  const size_t weight_bytes = is_mixed(prec) ? 4 : prec_elem_bytes(prec);
  size_t o = kZeroPage;
  L.layer[0] = o;
  L.bias[0] = o + kW0Bytes;
  o += align_up(kW0Bytes + 64 * 4, kAlign);
  L.w1_mfma = o;
  o += kW1MfmaBytes;
  for (int l = 1; l < NQA_NUM_CONVS; ++l) {
    L.layer[l] = o;
    o += rows_bytes(kConvs[l].cout, kConvs[l].cin, weight_bytes);
    L.bias[l] = o;
    o += bias_bytes(kConvs[l].cout);
  }
  for (int l = kRegwFirst; l <= kRegwLast; ++l) {
    L.regw[l] = o;
    if (l <= L.regw_last) o += (size_t)kConvs[l].cout * kConvs[l].cin * 9 * 2 * L.frag_terms;
  }
  L.w1_m16 = o;
  o += kW1M16Bytes * L.frag_terms;
  L.bytes = o;
  return L;
}

// built once (all eight modes); an unknown mode reads as an empty blob
static const BlobLayout &blob_layout(int prec) {
  static const struct Table {
    BlobLayout mode[NQA_PREC_F16W + 1], none;
    Table() {
      for (int p = 0; p <= NQA_PREC_F16W; ++p) mode[p] = walk_layout(p);
      memset(&none, 0, sizeof(none));
    }
  } table;
  return prec_valid_pyramid(prec) ? table.mode[prec] : table.none;
}

size_t layer_offset(int layer, int prec) { return blob_layout(prec).layer[layer]; }
size_t layer_bias_offset(int layer, int prec) { return blob_layout(prec).bias[layer]; }
size_t layer0_mfma_offset(int prec) { return blob_layout(prec).w1_mfma; }
size_t regw_offset(int layer, int prec) { return blob_layout(prec).regw[layer]; }
size_t layer0_m16_offset(int prec) { return blob_layout(prec).w1_m16; }
size_t conv_split_bias_off(int cout, int cin) { return rows_bytes(cout, cin, 4); }
size_t conv_half_bias_off(int cout, int cin) { return rows_bytes(cout, cin, 2); }

// ---- elements ------------------------------------------------------------------------------------------------------------
static uint16_t f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);                    // round to nearest even
}
static uint16_t f32_to_f16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7FFFFFFFu;
  if (u >= 0x7F800000u) return (uint16_t)(sign | (u > 0x7F800000u ? 0x7E00u : 0x7C00u));
  if (u >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // rounds to >= 65520 -> inf
  if (u < 0x33000001u) return (uint16_t)sign;               // < 2^-25 (or == 2^-25 tie -> 0)
  const int e = (int)(u >> 23) - 127;
  uint32_t m = (u & 0x7FFFFFu) | 0x800000u;
  int shift;
  uint32_t base;
  if (e < -14) {  // subnormal half
    shift = 13 + (-14 - e);
    base = 0;
  } else {
    shift = 13;
    base = (uint32_t)(e + 15) << 10;
    m &= 0x7FFFFFu;
  }
  uint32_t r = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (uint16_t)(sign | (base + r));
}
static float f16_to_f32(uint16_t hv) {
  const int e = (hv >> 10) & 31, m = hv & 1023;
  float v;
  if (e == 0) v = ldexpf((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = ldexpf((float)(m | 1024), e - 25);
  return (hv & 0x8000) ? -v : v;
}
// a weight in the format of 16-bit mode `prec`
static uint16_t to_16bit(float v, int prec) { return prec == NQA_PREC_BF16 ? f32_to_bf16(v) : f32_to_f16(v); }
// the two f16 terms of a (scaled) weight
static void split_half(float v, uint16_t &hi, uint16_t &lo) {
  hi = f32_to_f16(v);
  lo = f32_to_f16(v - f16_to_f32(hi));
}

// Power of two that puts a layer's largest |w| in [512, 1024), for the layers stored as (hi, lo).  A VGG weight is ~1e-2,
// whose residual after the f16 `hi` (~5e-6) is a SUBNORMAL half with an absolute quantum of 6e-8 -- 25 times coarser
// than float32 relative to the weight, which left 2e-6 of noise on every pre-activation and flipped nearly-dead
// channels of A-DISTS (oracle/knife_edge_study.py).  Scaled, hi and lo are both normal halves (22-23 significant bits
// together); the scale is exact and the conv epilogue multiplies the accumulator by 1/s (also exact) before the bias.
static int weight_scale_exp(const float *w, size_t count) {
  float wmax = 0.f;
  for (size_t i = 0; i < count; ++i) wmax = fmaxf(wmax, fabsf(w[i]));
  int k = 0;
  if (wmax > 0.f && isfinite(wmax)) {
    k = (int)floor(log2(1024.0 / (double)wmax));
    k = k < -8 ? -8 : (k > 24 ? 24 : k);
  }
  return k;
}

// ---- packers: one per format (nqa_common.h, "Packed weight blob"); w is OIHW, every weight is stored times `scale` -----------
enum RowKind {
  kRowsFloat,    // 4 floats per position, 16 input channels per tile
  kRows16,       // 8 bf16 / f16 per position, 32 channels per tile
  kRowsSplit,    // f32s: 16 channels per tile as [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15]
  kRowsTwoTerm,  // 32 channels per tile, each kernel row as [hi: 3 taps][lo: 3 taps]
};
// rows of one layer: tiles [cout/64][cin/KC], each [9 taps] (two-term: [ky][hi, lo][kx]) of [64 rows][4 positions of 16
// bytes], chunk c of row n at position c ^ swizzle(n).  m16: the swizzle of the 16x16x32 MFMA, else the 32x32x16's.
// prec16: the format of kRows16 elements.
static void pack_rows(const float *w, int cout, int cin, RowKind kind, bool m16, int prec16, float scale, void *dst) {
  const int cpc = kind == kRowsFloat ? 4 : 8;                              // elements per position
  const int kc = kind == kRowsFloat || kind == kRowsSplit ? 16 : 32;        // input channels per tile
  const int nslab = kind == kRowsTwoTerm ? 18 : 9, ncc = cin / kc;
  float *const d32 = static_cast<float *>(dst);
  uint16_t *const d16 = static_cast<uint16_t *>(dst);
  for (int ct = 0; ct < cout / 64; ++ct)
    for (int cc = 0; cc < ncc; ++cc)
      for (int s = 0; s < nslab; ++s)
        for (int n = 0; n < 64; ++n)
          for (int pos = 0; pos < 4; ++pos) {
            const int c = pos ^ (m16 ? ((n >> 2) & 1) * 2 : (n >> 2) & 3);
            // the slab's tap, the chunk's first channel inside the tile, and which term this (slab, chunk) holds
            int t = s, ci = c * cpc, part = 0;
            if (kind == kRowsSplit) ci = (c & 1) * 8, part = c >> 1;
            if (kind == kRowsTwoTerm) t = s / 6 * 3 + s % 3, part = s / 3 & 1;
            if (part) continue;  // a lo chunk is written with its hi
            const size_t e0 = (((((size_t)ct * ncc + cc) * nslab + s) * 64 + n) * 4 + pos) * cpc;
            const size_t lo0 = kind == kRowsSplit ? e0 ^ 16 : e0 + 3 * 64 * 4 * 8;  // position ^ 2 of the row / 3 slabs on
            const float *src = w + ((size_t)(ct * 64 + n) * cin + cc * kc + ci) * 9 + t;
            for (int j = 0; j < cpc; ++j) {
              const float v = src[j * 9] * scale;
              if (kind == kRowsFloat) d32[e0 + j] = v;
              else if (kind == kRows16) d16[e0 + j] = to_16bit(v, prec16);
              else split_half(v, d16[e0 + j], d16[lo0 + j]);
            }
          }
}

// a whole layer as 16x16x32 MFMA A fragments [cout/16 tiles][nterm][cin/32 * 9 k-steps][64 lanes][8 halfs]: k-step ks =
// chunk * 9 + tap, element j of lane (l15, c4) is w[16 * tile + l15][32 * chunk + 8 * c4 + j][tap].  nterm 1: in
// prec16's format (a kernel's 32-channel group is two consecutive tiles); nterm 2: the tile's hi, then its lo.
static void pack_layer_frags(const float *w, int cout, int cin, int nterm, int prec16, float scale, uint16_t *dst) {
  const int nks = cin / 32 * 9;
  for (int g = 0; g < cout / 16; ++g)
    for (int ks = 0; ks < nks; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int co = 16 * g + (lane & 15), ci = 32 * (ks / 9) + 8 * (lane >> 4) + j, t = ks % 9;
          const float v = w[((size_t)co * cin + ci) * 9 + t] * scale;
          const size_t e = ((((size_t)g * nterm) * nks + ks) * 64 + lane) * 8 + j;
          if (nterm == 1) dst[e] = to_16bit(v, prec16);
          else split_half(v, dst[e], dst[e + (size_t)nks * 64 * 8]);
        }
}

// conv1_1 as 16x16x32 A fragments [4 tiles of 16 channels][2 MFMAs][nterm][64 lanes][8 halfs]; MFMA m contracts kernel
// rows 2m and 2m+1: k = 8 * c4 + j = 16 * (ky - 2m) + 4 * kx + c (kx, c padded to 4; zero for ky = 3)
static void pack_w1_m16(const float *w0, int nterm, int prec16, float scale, uint16_t *dst) {
  for (int im = 0; im < 4 * 2; ++im)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int k = 8 * (lane >> 4) + j, ky = 2 * (im & 1) + (k >> 4), kx = (k >> 2) & 3, c = k & 3;
        const int co = 16 * (im >> 1) + (lane & 15);
        const float v = (ky < 3 && kx < 3 && c < 3) ? w0[(co * 3 + c) * 9 + ky * 3 + kx] * scale : 0.f;
        const size_t e = (((size_t)im * nterm) * 64 + lane) * 8 + j;
        if (nterm == 1) dst[e] = to_16bit(v, prec16);
        else split_half(v, dst[e], dst[e + 64 * 8]);
      }
}

// conv1_1 as 32x32 A fragments [ky][cout][h][8]: element j of half h is (kx = 2h + j/4, c = j%4), zero for kx = 3 or c = 3
static void pack_w1_mfma(const float *w0, int prec16, uint16_t *dst) {
  for (int ky = 0; ky < 3; ++ky)
    for (int co = 0; co < 64; ++co)
      for (int hj = 0; hj < 16; ++hj) {
        const int kx = hj / 4, c = hj % 4;
        dst[(ky * 64 + co) * 16 + hj] = to_16bit((kx < 3 && c < 3) ? w0[(co * 3 + c) * 9 + ky * 3 + kx] : 0.f, prec16);
      }
}

// layer 0 as the float kernels read it: w[k][cout], k = (ky*3+kx)*3 + c
static void pack_w0(const float *w0, float *dst) {
  for (int co = 0; co < 64; ++co)
    for (int c = 0; c < 3; ++c)
      for (int t = 0; t < 9; ++t) dst[(t * 3 + c) * 64 + co] = w0[(co * 3 + c) * 9 + t];
}

}  // namespace nqa

using namespace nqa;

extern "C" {

size_t nqa_packed_weights_bytes(int prec) { return blob_layout(prec).bytes; }

int nqa_pack_vgg_weights(const float *const w_host[NQA_NUM_CONVS], const float *const b_host[NQA_NUM_CONVS], int prec,
                         void *packed_host) {
  if (!w_host || !b_host || !packed_host) {
    set_error("pack_vgg_weights: null pointer");
    return NQA_E_ARG;
  }
  if (!prec_valid_pyramid(prec)) {
    set_error("pack_vgg_weights: unknown prec %d", prec);
    return NQA_E_ARG;
  }
  const BlobLayout &L = blob_layout(prec);
  char *blob = static_cast<char *>(packed_host);
  memset(blob, 0, L.bytes);  // (the zero page, the padding, and the 32x32 fragments of the modes that have none)
  pack_w0(w_host[0], reinterpret_cast<float *>(blob + L.layer[0]));
  memcpy(blob + L.bias[0], b_host[0], 64 * 4);
  if (L.frag_terms == 1) pack_w1_mfma(w_host[0], prec, reinterpret_cast<uint16_t *>(blob + L.w1_mfma));
  for (int l = 1; l < NQA_NUM_CONVS; ++l) {
    const ConvSpec &cs = kConvs[l];
    // the kernel precision that reads this layer: in a mixed mode f16 kernels on two-term weights up to the boundary,
    // f32s kernels behind it
    const int lprec = stage_prec(prec, cs.stage);
    const RowKind kind = layer_terms(prec, l) == 2 ? kRowsTwoTerm : lprec == NQA_PREC_F32S ? kRowsSplit
                         : lprec == NQA_PREC_F32 ? kRowsFloat : kRows16;
    const bool split = kind == kRowsTwoTerm || kind == kRowsSplit;  // stored as (hi, lo) of the weight times 2^k
    const int k = split ? weight_scale_exp(w_host[l], (size_t)cs.cout * cs.cin * 9) : 0;
    const float scale = ldexpf(1.f, k), inv = ldexpf(1.f, -k);
    // 16x16x32 swizzle for the 16-bit igemm layers (2..12); 32x32x16 for conv1_2 (shared with the fused stage-1
    // kernel), float and f32s
    pack_rows(w_host[l], cs.cout, cs.cin, kind, l >= 2 && (kind == kRows16 || kind == kRowsTwoTerm), lprec, scale,
              blob + L.layer[l]);
    memcpy(blob + L.bias[l], b_host[l], (size_t)cs.cout * 4);
    memcpy(blob + L.bias[l] + (size_t)cs.cout * 4, &inv, 4);
    if (l >= kRegwFirst && l <= L.regw_last)  // (two-term fragments carry the scale of the layer's rows)
      pack_layer_frags(w_host[l], cs.cout, cs.cin, L.frag_terms, prec, scale, reinterpret_cast<uint16_t *>(blob + L.regw[l]));
  }
  if (L.frag_terms) {
    // two-term: the weights times a power of two; 1 / that scale in the first float of the 32x32-fragment area
    const int k1 = L.frag_terms == 2 ? weight_scale_exp(w_host[0], 64 * 27) : 0;
    const float inv1 = ldexpf(1.f, -k1);
    if (L.frag_terms == 2) memcpy(blob + L.w1_mfma, &inv1, 4);
    pack_w1_m16(w_host[0], L.frag_terms, prec, ldexpf(1.f, k1), reinterpret_cast<uint16_t *>(blob + L.w1_m16));
  }
  return NQA_OK;
}

// one 3x3 layer in the f32s row format, zero bias (nqa_conv3x3_split)
size_t nqa_packed_conv_split_bytes(int cout, int cin) {
  if (cout <= 0 || cin <= 0 || cout % 64 || cin % 16) return 0;
  return conv_split_bias_off(cout, cin) + bias_bytes(cout);
}

int nqa_pack_conv_split(const float *w_oihw, int cout, int cin, void *packed_host) {
  if (!w_oihw || !packed_host || cout <= 0 || cin <= 0 || cout % 64 || cin % 16) {
    set_error("pack_conv_split: bad argument (cout %d must be a multiple of 64, cin %d of 16)", cout, cin);
    return NQA_E_ARG;
  }
  char *blob = static_cast<char *>(packed_host);
  memset(blob, 0, nqa_packed_conv_split_bytes(cout, cin));  // (bias = 0)
  const int k = weight_scale_exp(w_oihw, (size_t)cout * cin * 9);
  const float inv = ldexpf(1.f, -k);
  pack_rows(w_oihw, cout, cin, kRowsSplit, false, 0, ldexpf(1.f, k), blob);
  memcpy(blob + conv_split_bias_off(cout, cin) + (size_t)cout * 4, &inv, 4);
  return NQA_OK;
}

// one 3x3 layer in the f16 row format, zero bias (nqa_conv3x3_half)
size_t nqa_packed_conv_half_bytes(int cout, int cin) {
  if (cout <= 0 || cin <= 0 || cout % 64 || cin % 32) return 0;
  return conv_half_bias_off(cout, cin) + bias_bytes(cout);
}

int nqa_pack_conv_half(const float *w_oihw, int cout, int cin, void *packed_host) {
  if (!w_oihw || !packed_host || cout <= 0 || cin <= 0 || cout % 64 || cin % 32) {
    set_error("pack_conv_half: bad argument (cout %d must be a multiple of 64, cin %d of 32)", cout, cin);
    return NQA_E_ARG;
  }
  char *blob = static_cast<char *>(packed_host);
  memset(blob, 0, nqa_packed_conv_half_bytes(cout, cin));  // (bias = 0; the float behind it, a scale elsewhere, is not read)
  // the swizzle of the MFMA that nqa_conv3x3_half runs the layer on: 16x16x32 on 128-channel tiles, else 32x32x16
  pack_rows(w_oihw, cout, cin, kRows16, cout % 128 == 0, NQA_PREC_F16, 1.f, blob);
  return NQA_OK;
}

}  // extern "C"
