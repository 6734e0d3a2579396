// Device pieces shared by the register-weights kernels (gfx950): conv3x3_regw_kernel, conv3x3_regw128_kernel,
// conv1_regw_kernel, conv1_regw_split_kernel, conv3x3_regw_split_kernel (nqa_conv.hip), conv3x3_regw128_pool_kernel
// (nqa_conv_pool.hip) and conv1_pool_kernel (nqa_conv1_pool.hip).  They are one idea -- a wave's weight fragments stay
// in registers, a halo image in LDS is walked with immediate offsets, tiles are dealt to persistent blocks -- and what
// they have in common is written here once.  Everything is __device__ __forceinline__ or constexpr; nothing launches or
// allocates.  These kernels are register-budgeted and their waits are counted by hand: a change here is judged by
// tools/kernel_isa_diff.py (every kernel's instruction stream against the parent commit's), see DESIGN.md.
#pragma once
#include "nqa_common.h"

namespace nqa {

// destination type of the LDS-DMA builtin (buffer_load ... lds)
typedef __attribute__((address_space(3))) void lds_void_t;

// A buffer offset no image reaches: a DMA lane or a store with it transfers nothing, but the instruction is still issued
// and still counts once in vmcnt -- which is what keeps the counted waits of these kernels the same for every wave.
constexpr unsigned kOOB = 0x80000000u;

// ImageNet input normalisation (x - mean) / std (DISTS_pt.py:92)
constexpr float kMean[3] = {0.485f, 0.456f, 0.406f};
constexpr float kStd[3] = {0.229f, 0.224f, 0.225f};

// LDS row swizzle: chunk c of row r sits at position c ^ lds_swz(r).  The 32x32x16 MFMA reads one
// chunk of 32 consecutive rows per instruction (rows spread by (r>>2)&3); the 16x16x32 MFMA reads
// all four chunks of 16 consecutive rows (chunk = lane>>4), which is conflict-free from any base
// row with 2*((r>>2)&1) (found by exhaustive search over the ds_read_b128 lane groups).
template <bool M16>
__host__ __device__ inline int lds_swz(int r) {
  return M16 ? ((r >> 2) & 1) * 2 : (r >> 2) & 3;
}

__device__ __forceinline__ float dpp_row_shr1(float v) {  // lane l of each 16-lane row reads lane l-1; lane 0 reads 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_row_shl1(float v) {  // lane l reads lane l+1; lane 15 reads 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xF, 0xF, true));
}

// ---- tile dealing --------------------------------------------------------------------------------------------------
// XCD-aware: workgroups are dealt round-robin over the 8 XCDs, so ids equal mod 8 share an L2.  XCD x owns tiles
// [T*x/8, T*(x+1)/8), dealt round-robin to its blocks: the workgroups that share an L2 walk a contiguous range of tiles
// and neighbouring tiles' halo overlap is an L2 hit (speed only; any placement is correct).  Block-uniform: tile `it`
// of this block is first + it * stride, it < count.  tests/persistent_refs.py models this function.
struct TileRun {
  int first, stride, count;
  __device__ __forceinline__ explicit TileRun(int total_tiles) {
    const int nblk = gridDim.x, nx = nblk < 8 ? nblk : 8;  // (a grid of fewer than 8 blocks has fewer classes)
    const int xcd = blockIdx.x % nx, jb = blockIdx.x / nx;
    const int blk_per_xcd = (nblk - xcd + nx - 1) / nx;  // blocks with id = xcd (mod nx)
    const int t_lo = (int)((long)total_tiles * xcd / nx), t_hi = (int)((long)total_tiles * (xcd + 1) / nx);
    first = t_lo + jb;
    stride = blk_per_xcd;
    count = t_lo + jb < t_hi ? (t_hi - t_lo - jb - 1) / blk_per_xcd + 1 : 0;
  }
  // image n and origin (x0, y0) of pixel tile t of a (tiles_x x tiles_y tiles of TH x TW) x images grid
  template <int TH, int TW>
  __device__ __forceinline__ static void decode(int t, int tiles_x, int tiles_y, int &n, int &x0, int &y0) {
    n = t / (tiles_x * tiles_y);
    const int t2 = t - n * (tiles_x * tiles_y), by = t2 / tiles_x;
    x0 = (t2 - by * tiles_x) * TW;
    y0 = by * TH;
  }
  template <int TH, int TW>
  __device__ __forceinline__ void coords(int it, int tiles_x, int tiles_y, int &n, int &x0, int &y0) const {
    decode<TH, TW>(first + it * stride, tiles_x, tiles_y, n, x0, y0);
  }
};

// The pool kernels' dealing: block b owns the CONTIGUOUS run of units [lo, hi) (a strip is walked top to bottom with the
// row above carried in registers); the blocks that share an XCD (ids equal mod 8) own adjacent runs, i.e. neighbouring
// strips, whose two shared halo columns then hit one L2.
__device__ __forceinline__ void unit_run(int total_units, int &u_lo, int &u_hi) {
  const int nblk = gridDim.x;
  int run;
  {
    const int qq = nblk >> 3, rr = nblk & 7, xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    run = nblk < 8 ? (int)blockIdx.x : (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + local;
  }
  u_lo = (int)((long)total_units * run / nblk);
  u_hi = (int)((long)total_units * (run + 1) / nblk);
}

// ---- weights ---------------------------------------------------------------------------------------------------------
// The blob's register-weights format (nqa_common.h): per 16-channel tile and k-step one 16x16x32 MFMA A fragment, 16 bytes
// per lane.  Channel group g of a layer = two fragment sets i of NKS k-steps: two 16-channel tiles (one-term weights), or
// the f16 (hi, lo) parts of ONE tile's weights (two-term).  One fragment, straight into registers; the kernels keep the
// loops over (i, ks) -- a helper that filled their wf[2][NKS] changed most of them.
template <int NKS>
__device__ __forceinline__ u32x4 load_wfrag(const char *wreg, int g, int i, int ks, int lane) {
  return *reinterpret_cast<const u32x4 *>(wreg + ((((size_t)g * 2 + i) * NKS + ks) * 64 + lane) * 16);
}

// ---- halo image of 64-byte pixel records, filled by LDS-DMA ------------------------------------------------------------
// DMA plan of one 32-channel chunk: item j (16 B; j = round * threads + tid) is quarter (j&3)^swz of halo pixel
// q = j>>2 = (row hy, column hx) of an HWD-wide patch of NQ pixels.  Items past the patch get a row that is never
// inside any image: a past-the-end item or tile issues the same DMA pieces, all out of range, so every wave issues
// the same number per tile and the ring is retired with one counted vmcnt.
// The chunk swizzle goes by the pixel's COLUMN in the patch, not by its linear index: equally conflict-free (a row of
// the patch only shifts the phase of the pattern), and a tap's LDS address is then one per-lane constant per kx plus
// compile-time offsets -- no address arithmetic in the k loop (tap_offset).
// (Returned per item as scalars: filling the kernels' p_hy / p_hx / p_c arrays inside a helper changed their code.)
struct HaloItem {
  int hy, hx, c;
};
template <int NQ, int HWD>
__device__ __forceinline__ HaloItem halo_item(int j) {
  const int q = j >> 2;
  HaloItem it;
  it.hy = q < NQ ? q / HWD : -100000;
  it.hx = q - (q / HWD) * HWD;
  it.c = (j & 3) ^ lds_swz<true>(it.hx);
  return it;
}
// per-lane byte offset of the lane's fragment (quarter c4) of patch column `col` (any patch row, 16-pixel group 0); the
// kernels keep one per tap column kx, col = l15 + kx
__device__ __forceinline__ int tap_offset(int col, int c4) { return col * 64 + ((c4 ^ lds_swz<true>(col)) << 4); }

// ---- the three-term f32s k loop ------------------------------------------------------------------------------------------
// conv1_2 / conv2_1 in f32s: a wave = 16 output channels x RW tile rows x GPP groups of 16 columns; wf = the f16 (hi, lo)
// fragments of its weights; the halo image at `slot` holds per pixel and 32-channel chunk (CH_BYTES apart) a record of
// PITCH bytes, [32 channels hi | LO: 32 channels lo | pad].  q0[g] = byte offset of the lane's hi fragment at the wave's
// first halo row, tap kx = 0, chunk 0 (the caller keeps it opaque).
// BOTH rows of the wave in one k loop: a step = one halo row hr (0..RW+1 below the wave's first output row) x one column
// tap kx x one 32-channel chunk; its four fragments (hi, lo x two 16-column groups) feed output row r = hr - ky for every
// kernel row ky that exists -- 6 MFMAs in the first and last halo row, 12 in the middle two.  24 steps and 96 fragment
// reads per tile instead of 36 and 144: with four waves of a CU in conv1_2 at once the row-at-a-time form asked the LDS
// for 128 clocks of reads per 96 clocks of MFMA.
// acc[0]: hi*hi; acc[1]: the two cross terms w_lo*a_hi + w_hi*a_lo (2^-11 of the first: one accumulator, they are added
// in the end anyway), per group and output row -- 32 registers; a third set spilled.
template <int RW, int GPP, int HWD, int PITCH, int CH_BYTES, int LO>
__device__ __forceinline__ void split3_kloop(const char *slot, const int (&q0)[GPP], const u32x4 (&wf)[2][18],
                                             f32x4 (&acc)[2][GPP][RW]) {
  u32x4 bh[2][GPP], bl[2][GPP];
  auto load_s = [&](int s, u32x4(&h)[GPP], u32x4(&l)[GPP]) {
    const int cc = s / 12, hr = (s - cc * 12) / 3, kx = s - cc * 12 - hr * 3;
#pragma unroll
    for (int g = 0; g < GPP; ++g) {
      h[g] = *reinterpret_cast<const u32x4 *>(slot + q0[g] + (cc * CH_BYTES + (hr * HWD + kx) * PITCH));
      l[g] = *reinterpret_cast<const u32x4 *>(slot + q0[g] + (cc * CH_BYTES + (hr * HWD + kx) * PITCH + LO));
    }
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < GPP; ++g)
#pragma unroll
      for (int r = 0; r < RW; ++r) acc[i][g][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NSTEP = 2 * (RW + 2) * 3;
  static_assert(RW == 2, "the step -> (chunk, halo row, tap) map is written for two rows per wave");
  load_s(0, bh[0], bl[0]);
#pragma unroll
  for (int s2 = 0; s2 < NSTEP; ++s2) {
    if (s2 + 1 < NSTEP) load_s(s2 + 1, bh[(s2 + 1) & 1], bl[(s2 + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    const int cc = s2 / 12, hr = (s2 - cc * 12) / 3, kx = s2 - cc * 12 - hr * 3;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int ky = hr - r;
      if (ky < 0 || ky > 2) continue;
      const int ks = cc * 9 + ky * 3 + kx;
#pragma unroll
      for (int term = 0; term < 3; ++term)  // (a cross accumulator's two MFMAs are a term apart: never back to back)
#pragma unroll
        for (int g = 0; g < GPP; ++g)
          acc[term ? 1 : 0][g][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
              __builtin_bit_cast(f16x8, wf[term == 1 ? 1 : 0][ks]),
              __builtin_bit_cast(f16x8, term == 2 ? bl[s2 & 1][g] : bh[s2 & 1][g]), acc[term ? 1 : 0][g][r], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace nqa
