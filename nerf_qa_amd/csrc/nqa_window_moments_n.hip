// Windowed moments of the A-DISTS head and their backward for a RUN-TIME window size n (3 <= n <= 63, odd or even):
// the generic form of nqa_window_moments.hip's two kernels, with their contract (include/nqa.h).  The host side of both
// families ends here: window_moments_forward / _backward take the window and a MomentsKernels, and runs_generic() below
// is the one place that sends a call to these kernels or to the 21-tap ones.
//
//   window_moments_n_fwd_kernel   the two (five) maps of n x n Gaussian window means of x (and y), h = H - n + 1,
//                                 w = W - n + 1; the products x^2, y^2, xy are formed in registers on the way into LDS
//   window_moments_n_bwd_kernel   gx = W^T g0 + 2 x W^T g2 + y W^T g4 and its mirror, a GATHER: every pixel sums over the
//                                 windows that contain it, the upstream maps folded in the fixed order g0 .. g4
//
// The shape is the 21-tap kernels': P = B * C independent planes, a block of 256 threads owns a TH x 64 tile of what it
// writes, stages the (TH + n - 1) x (64 + n - 1) halo tile of ONE averaged quantity in LDS (zero outside the map), takes
// its n-tap column sums (a thread per column and 8 rows) and the n-tap row sums of those (a thread per 4 adjacent columns,
// 16-byte LDS reads).  One quantity is in LDS at a time -- the forward re-reads x and y per moment instead of holding both
// tiles -- so a block needs (TH + n - 1 + TH) x round4(64 + n - 1) floats: TH = 24 up to n = 21 (the 21-tap tile), 16
// above, which is 48 128 bytes at n = 63: three blocks fit a CU's 160 KiB (DESIGN.md 4.20 has the table).
//
// The taps are a kernel-argument table indexed by block-uniform integers (scalar loads), built on the host by the generic
// scoring kernels' arithmetic (window_taps_n, nqa_adists.hip), and nothing is assumed about symmetry: an even window's
// centre is n / 2, so it has none.  Output o of a pass sums tap k against position o + k for k ascending.  The transposed
// correlation of the backward is the same pair of passes over the upstream map padded with n - 1 zeros on every side with
// the table REVERSED (pixel r meets window i = r - n + 1 + k through tap n - 1 - k): its sums run in ascending window
// order.  A pass is walked in blocks of R positions; a block whose R x R (output, position) pairs all lie inside the
// window runs without a test, the first block and the last one or two test every pair, so no value is ever multiplied
// by a tap it does not meet (a pixel outside a window cannot reach it, whatever its size: head.py's upstreams of 1e12
// sit next to ordinary ones).  One writer per element, no atomics: bitwise repeatable.  A side that is not asked for
// costs nothing and the other side's instructions do not depend on it.
//
// 16-byte global accesses: the input planes where W % 4 == 0; the window-mean planes (forward's stores, backward's
// upstream) where also (n - 1) % 4 == 0, so that w % 4 == 0 and the backward's halo origin c0 - (n - 1) stays a multiple
// of 4.  Everything else moves as single floats; the entry points ask for 16-byte alignment exactly where the 21-tap
// ones do (W % 4 == 0).
#include <math.h>

#include "nqa_window_moments.h"

namespace nqa {

static constexpr int kNTW = 64;    // columns of a tile of outputs
static constexpr int kNVRows = 8;  // rows per thread of the vertical pass

struct TapsN {
  float g[64];  // taps 0 .. n-1 (reversed for the backward); zeros behind them
};

// rows of a tile of outputs, and the floats of dynamic LDS a block needs
__host__ __device__ inline int tile_rows_n(int n) { return n <= 21 ? 24 : 16; }
__host__ __device__ inline int tile_stride_n(int n) { return (kNTW + n - 1 + 3) & ~3; }
__host__ __device__ inline int tile_floats_n(int n) { return (2 * tile_rows_n(n) + n - 1) * tile_stride_n(n); }

// acc[o] += sum_k g[k] * v(o + k), o < R, k < n, walking the positions p = o + k upwards in blocks of R (so k ascends
// for every o).  load(pb, checked, v) fills v[j] with position pb + j; in a checked block positions past n + R - 2 are
// asked for but never used.
template <int R, bool CHECK, typename L>
__device__ __forceinline__ void tap_block(const TapsN &gw, int n, int pb, L load, float (&acc)[R]) {
  float t[2 * R - 1];  // t[i] = g[pb - (R - 1) + i]
#pragma unroll
  for (int i = 0; i < 2 * R - 1; ++i) {
    const int k = pb - (R - 1) + i;
    t[i] = gw.g[CHECK ? min(max(k, 0), 63) : k];
  }
  float v[R];
  load(pb, CHECK, v);
#pragma unroll
  for (int j = 0; j < R; ++j) {
#pragma unroll
    for (int o = 0; o < R; ++o) {
      const int k = pb + j - o;
      if (!CHECK || (k >= 0 && k < n)) acc[o] = fmaf(t[j - o + R - 1], v[j], acc[o]);
    }
  }
}

template <int R, typename L>
__device__ __forceinline__ void tap_walk(const TapsN &gw, int n, L load, float (&acc)[R]) {
  const int nblk = (n + 2 * R - 2) / R;  // blocks over the n + R - 1 positions
  const int full = n / R;                // blocks 1 .. full - 1 lie wholly inside every output's window
  tap_block<R, true>(gw, n, 0, load, acc);
  int b = 1;
  for (; b < full; ++b) tap_block<R, false>(gw, n, b * R, load, acc);
  for (; b < nblk; ++b) tap_block<R, true>(gw, n, b * R, load, acc);
}

// the averaged quantity from its operands: a, a^2 or a b
__device__ __forceinline__ float term_n(int mode, float a, float b) { return mode == 0 ? a : mode == 1 ? a * a : a * b; }

// Stage term(a, b) of the ih x iws halo tile whose first element is (r0, c0) of the nr x nc planes into LDS, zero where
// it leaves the plane.  vec: c0 and nc are multiples of 4 and the planes 16-byte aligned, so every 4-column chunk is
// wholly inside or wholly outside and moves as one 16-byte access.  b is read only in mode 2.
__device__ inline void stage_tile_n(const float *__restrict__ a, const float *__restrict__ b, int mode, int nr, int nc,
                                    int r0, int c0, bool vec, int ih, int iws, float *tile) {
  if (vec) {
    const int cpr = iws / 4;
    for (int i = threadIdx.x; i < ih * cpr; i += 256) {
      const int lr = i / cpr, lc = (i - lr * cpr) * 4;
      const int r = r0 + lr, c = c0 + lc;
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (r >= 0 && r < nr && c >= 0 && c < nc) {
        va = *reinterpret_cast<const f32x4 *>(a + (size_t)r * nc + c);
        if (mode == 2) vb = *reinterpret_cast<const f32x4 *>(b + (size_t)r * nc + c);
      }
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = term_n(mode, va[e], vb[e]);
      *reinterpret_cast<f32x4 *>(tile + lr * iws + lc) = o;
    }
  } else {
    for (int i = threadIdx.x; i < ih * iws; i += 256) {
      const int lr = i / iws, lc = i - lr * iws;
      const int r = r0 + lr, c = c0 + lc;
      float va = 0.f, vb = 0.f;
      if (r >= 0 && r < nr && c >= 0 && c < nc) {
        va = a[(size_t)r * nc + c];
        if (mode == 2) vb = b[(size_t)r * nc + c];
      }
      tile[i] = term_n(mode, va, vb);
    }
  }
}

// Column sums: V[o][c] = sum_k g[k] * tile[o + k][c], o < th, c < iws (the tile holds th + n - 1 rows of iws floats).
__device__ inline void vertical_pass_n(const TapsN &gw, int n, const float *tile, int th, int iws, float *V) {
  const int items = iws * (th / kNVRows);  // <= 256 for every (th, n) in use; the loop is for the general case
  for (int it = threadIdx.x; it < items; it += 256) {
    const int g = it / iws, col = it - g * iws, row0 = g * kNVRows;
    const float *src = tile + row0 * iws + col;
    float acc[kNVRows];
#pragma unroll
    for (int o = 0; o < kNVRows; ++o) acc[o] = 0.f;
    tap_walk<kNVRows>(
        gw, n,
        [&](int pb, bool checked, float (&v)[kNVRows]) {
#pragma unroll
          for (int j = 0; j < kNVRows; ++j) {
            const int p = checked ? min(pb + j, n + kNVRows - 2) : pb + j;  // (<= the tile's last row th + n - 2)
            v[j] = src[p * iws];
          }
        },
        acc);
#pragma unroll
    for (int o = 0; o < kNVRows; ++o) V[(row0 + o) * iws + col] = acc[o];
  }
}

// Row sums of 4 adjacent outputs: out[e] = sum_k g[k] * vrow[e + k], vrow 16-byte aligned.  The last block's reads end
// at column col4 + round4(n + 3) - 1 <= iws - 1.
__device__ __forceinline__ void horizontal_item_n(const TapsN &gw, int n, const float *vrow, float (&out)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = 0.f;
  tap_walk<4>(
      gw, n,
      [&](int pb, bool, float (&v)[4]) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(vrow + pb);
        v[0] = q[0];
        v[1] = q[1];
        v[2] = q[2];
        v[3] = q[3];
      },
      out);
}

// grid (cdiv(w, 64), cdiv(h, TH), planes), tile_floats_n(n) floats of dynamic LDS.  out: moment m of plane p at
// ((m * P + p) * h * w); P: planes of the whole call, p0: the first plane of this launch.  PAIR: five moments of (x, y);
// else E[x], E[x^2] of x.
template <bool PAIR>
__global__ __launch_bounds__(256) void window_moments_n_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                   int H, int W, int P, int p0, TapsN gw, int n,
                                                                   float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds_wmn[];
  const int th = tile_rows_n(n), ih = th + n - 1, iws = tile_stride_n(n);
  float *const tile = lds_wmn, *const V = lds_wmn + ih * iws;
  const int h = H - (n - 1), w = W - (n - 1);
  const int p = p0 + blockIdx.z, oy0 = blockIdx.y * th, ox0 = blockIdx.x * kNTW;
  const bool vec_in = (W & 3) == 0, vec_out = vec_in && ((n - 1) & 3) == 0;
  const float *xp = x + (size_t)p * H * W, *yp = PAIR ? y + (size_t)p * H * W : nullptr;
  const size_t plane = (size_t)h * w;
  for (int m = 0; m < (PAIR ? 5 : 2); ++m) {
    const int q = PAIR ? m : 2 * m;  // x, y, x^2, y^2, xy
    const float *a = (q == 1 || q == 3) ? yp : xp;
    stage_tile_n(a, yp, q < 2 ? 0 : q < 4 ? 1 : 2, H, W, oy0, ox0, vec_in, ih, iws, tile);
    __syncthreads();
    vertical_pass_n(gw, n, tile, th, iws, V);
    __syncthreads();
    float *o = out + ((size_t)m * P + p) * plane;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int it = threadIdx.x + u * 256;
      const int row = it / (kNTW / 4), col4 = (it % (kNTW / 4)) * 4;
      if (it < th * (kNTW / 4) && oy0 + row < h && ox0 + col4 < w) {
        float r[4];
        horizontal_item_n(gw, n, V + row * iws + col4, r);
        store4(o + (size_t)(oy0 + row) * w, ox0 + col4, w, vec_out, r);
      }
    }
    // (the next moment's stage writes the tile, which nobody reads any more; its barrier precedes the next write of V)
  }
}

struct WindowGradsN {
  const float *g[5];  // upstream of E[x], E[y], E[x^2], E[y^2], E[xy], each (P, h, w); null = zero (or not needed)
};

// grid (cdiv(W, 64), cdiv(H, TH), planes), tile_floats_n(n) floats of dynamic LDS; gw holds the taps REVERSED.  The host
// has already dropped the maps the wanted sides do not read (g0, g2 without gx; g1, g3 without gy).
__global__ __launch_bounds__(256) void window_moments_n_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                   int H, int W, int p0, WindowGradsN wg, TapsN gw, int n,
                                                                   float *__restrict__ gx, float *__restrict__ gy) {
  extern __shared__ __attribute__((aligned(16))) float lds_wmn[];
  const int th = tile_rows_n(n), ih = th + n - 1, iws = tile_stride_n(n);
  float *const tile = lds_wmn, *const V = lds_wmn + ih * iws;
  const int h = H - (n - 1), w = W - (n - 1);
  const int p = p0 + blockIdx.z, r0 = blockIdx.y * th, c0 = blockIdx.x * kNTW;
  const bool vec_in = (W & 3) == 0, vec_up = vec_in && ((n - 1) & 3) == 0;
  const size_t in_plane = (size_t)p * H * W, g_plane = (size_t)p * h * w;
  // this thread's pixels: item u = (row, 4 columns)
  bool live[2];
  size_t at[2];
  int col[2];
  float xr[2][4], yr[2][4], ax[2][4], ay[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int it = threadIdx.x + u * 256;
    const int row = it / (kNTW / 4), col4 = (it % (kNTW / 4)) * 4;
    live[u] = it < th * (kNTW / 4) && r0 + row < H && c0 + col4 < W;
    col[u] = c0 + col4;
    at[u] = in_plane + (size_t)(r0 + row) * W;
    if (vec_in) {  // (W % 4 == 0: the four columns are inside together, one 16-byte load each)
      f32x4 xv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
      if (live[u]) xv = *reinterpret_cast<const f32x4 *>(x + at[u] + col[u]);
      if (live[u] && y) yv = *reinterpret_cast<const f32x4 *>(y + at[u] + col[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xr[u][e] = xv[e];
        yr[u][e] = yv[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = live[u] && col[u] + e < W;
        xr[u][e] = in ? x[at[u] + col[u] + e] : 0.f;
        yr[u][e] = (in && y) ? y[at[u] + col[u] + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ax[u][e] = ay[u][e] = 0.f;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    if (!wg.g[q]) continue;  // (uniform over the grid)
    stage_tile_n(wg.g[q] + g_plane, nullptr, 0, h, w, r0 - (n - 1), c0 - (n - 1), vec_up, ih, iws, tile);
    __syncthreads();
    vertical_pass_n(gw, n, tile, th, iws, V);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!live[u]) continue;
      const int it = threadIdx.x + u * 256;
      float a[4];
      horizontal_item_n(gw, n, V + (it / (kNTW / 4)) * iws + (it % (kNTW / 4)) * 4, a);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (q == 0) ax[u][e] = a[e];
        if (q == 1) ay[u][e] = a[e];
        if (q == 2) ax[u][e] = fmaf(2.f * xr[u][e], a[e], ax[u][e]);
        if (q == 3) ay[u][e] = fmaf(2.f * yr[u][e], a[e], ay[u][e]);
        if (q == 4) {
          ax[u][e] = fmaf(yr[u][e], a[e], ax[u][e]);
          ay[u][e] = fmaf(xr[u][e], a[e], ay[u][e]);
        }
      }
    }
    // (the next map's stage writes the tile, which nobody reads any more; its barrier precedes the next write of V)
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!live[u]) continue;
    if (gx) store4(gx + at[u], col[u], W, vec_in, ax[u]);
    if (gy) store4(gy + at[u], col[u], W, vec_in, ay[u]);
  }
}

// ---------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------
static TapsN taps_n(int n, bool reversed) {
  TapsN t = {};
  const float *g = window_taps_n(n);
  for (int k = 0; k < n; ++k) t.g[k] = g[reversed ? n - 1 - k : k];
  return t;
}

// THE choice between the two kernel families, for both directions and, through them, the stage backward: every window
// but 21 has the generic kernels alone; 21 runs the 21-tap ones unless the caller leaves it to a tuning state that asks
// for the generic ones.
static bool runs_generic(int n, MomentsKernels kernels) {
  return n != 21 || (kernels == MomentsKernels::Tuned && tuning().moments_generic);
}

int window_moments_forward(const float *x, const float *y, int P, int H, int W, int n, MomentsKernels kernels, float *out,
                           hipStream_t st) {
  if (!runs_generic(n, kernels)) return window_moments_forward_21(x, y, P, H, W, out, st);
  const int h = H - (n - 1), w = W - (n - 1), th = tile_rows_n(n);
  const size_t lds = (size_t)tile_floats_n(n) * sizeof(float);
  const TapsN gw = taps_n(n, false);
  return launch_plane_chunks("window_moments_n_fwd", P, cdiv(w, kNTW), cdiv(h, th), st, [&](dim3 grid, int p0) {
    if (y) window_moments_n_fwd_kernel<true><<<grid, 256, lds, st>>>(x, y, H, W, P, p0, gw, n, out);
    else window_moments_n_fwd_kernel<false><<<grid, 256, lds, st>>>(x, nullptr, H, W, P, p0, gw, n, out);
  });
}

int window_moments_backward(const float *x, const float *y, int P, int H, int W, int n, MomentsKernels kernels,
                            const float *const g[5], float *gx, float *gy, hipStream_t st) {
  if (!runs_generic(n, kernels)) return window_moments_backward_21(x, y, P, H, W, g, gx, gy, st);
  const WindowGradsN wg = wanted_grads<WindowGradsN>(g, gx, gy);
  const size_t lds = (size_t)tile_floats_n(n) * sizeof(float);
  const TapsN gw = taps_n(n, true);
  const int th = tile_rows_n(n);
  return launch_plane_chunks("window_moments_n_bwd", P, cdiv(W, kNTW), cdiv(H, th), st, [&](dim3 grid, int p0) {
    window_moments_n_bwd_kernel<<<grid, 256, lds, st>>>(x, y, H, W, p0, wg, gw, n, gx, gy);
  });
}

}  // namespace nqa
