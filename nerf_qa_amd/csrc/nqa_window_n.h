// The windowed pass for a RUN-TIME window size n (3 <= n <= 63, odd or even): the generic form of the three 21-tap
// kernels of nqa_adists.hip, included there once (inside namespace nqa, behind div_nr and wave_sum3, which it uses).
// The 21-tap kernels keep their ring of horizontal sums in registers, one slot per row body of a 21-fold unrolled loop;
// that needs n at compile time.  Here the ring lives in LDS:
//   * a block is ONE wave.  NHWC taps: it owns one output column and a strip of output rows, lane = channel of a
//     64-channel block (the lanes kernel's shape).  Planes (stage 0): lane = one of 64 adjacent output columns.
//   * per input row the lane takes the n-tap HORIZONTAL sums of (x, y, x^2, y^2, xy) from 2 n loads and stores them
//     into slot (row mod n) of its own column of the ring, float ring[n][5][64]: 1280 n bytes per wave, every access
//     a 64-lane row of consecutive dwords (no bank conflict), every lane reading only what it wrote itself, so there
//     is no barrier anywhere.  Two such waves must fit a CU's 160 KiB: n <= 63 (2 x 63 x 1280 = 161 280 <= 163 840).
//   * once n rows are in, the n-tap VERTICAL sums walk the ring from the oldest slot to the newest -- tap j meets
//     slot (newest + 1 + j) mod n, written as two runs without a modulo -- and the per-pixel terms follow.
// The taps are a kernel-argument table (GaussN) indexed by wave-uniform j: scalar loads, nothing assumed about
// symmetry (an even window's centre is n / 2, so it has none).  Sums run in ascending tap order.
// The group forms (K renders per reference, adists_window_lanes_kernel's comment) are the same bodies with GRP = true.
// No include guard: included once.

struct GaussN {
  float g[64];  // taps 0 .. n-1 of gaussian(n, n / 3); zeros behind them
};

// gamma term, T and S of one (pixel, channel) from the five window means of the raw maps: win_row's expressions
// (ADISTS.py:84-86, 182-183) on div_nr, for sums that do not come out of a register ring.
__device__ __forceinline__ void win_n_terms(const float (&m)[5], float ix, float iy, float wc, float &gterm, float &tt,
                                            float &ss) {
  gterm = div_nr(m[2] - m[0] * m[0], m[0] + 1e-12f);
  const float mx = ix * m[0], my = iy * m[1];
  const float vx = ix * ix * m[2] - mx * mx, vy = iy * iy * m[3] - my * my;
  const float cov = ix * iy * m[4] - mx * my;
  tt = wc * div_nr(2.f * mx * my + 1e-6f, mx * mx + my * my + 1e-6f);
  ss = wc * div_nr(2.f * cov + 1e-6f, vx + vy + 1e-6f);
}

// One input row of one lane: the horizontal sums of taps lx(j), ly(j) into ring slot `slot` (rl = the lane's column of
// the ring); when `full`, the vertical sums m over the n slots, oldest first.
// The loads run two batches of U taps ahead of the arithmetic (a block is one wave and the ring leaves room for few
// waves per CU, so the latency has to be hidden inside the wave): xa / ya hold the row's first batch on entry, and
// leave holding the NEXT row's (lxn, lyn; issued before the vertical pass) when there is one.  n is rounded up to
// whole batches: a tap index past the window is clamped to n - 1 -- a pixel the window reads anyway -- and meets one
// of the zeros behind the taps in the table, so the sums are those of the n taps, bit for bit.
constexpr int kWinNBatch = 4;
template <typename FX, typename FY, typename GX, typename GY>
__device__ __forceinline__ void win_n_row(int n, const GaussN &gw, float *rl, int slot, bool full, bool more, FX lx, FY ly,
                                          GX lxn, GY lyn, float (&xa)[kWinNBatch], float (&ya)[kWinNBatch],
                                          float (&m)[5]) {
  constexpr int U = kWinNBatch;
  float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
  auto taps = [&](int j0, const float (&xs)[U], const float (&ys)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float gx = gw.g[j0 + u] * xs[u], gy = gw.g[j0 + u] * ys[u];
      h0 += gx;
      h1 += gy;
      h2 = fmaf(gx, xs[u], h2);
      h3 = fmaf(gy, ys[u], h3);
      h4 = fmaf(gx, ys[u], h4);
    }
  };
  float xb[U], yb[U];
  for (int j0 = 0; j0 < n; j0 += 2 * U) {  // (j0 + 2 U - 1 <= 63: inside the table)
    if (j0 + U < n) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = min(j0 + U + u, n - 1);
        xb[u] = lx(j);
        yb[u] = ly(j);
      }
    }
    taps(j0, xa, ya);
    if (j0 + 2 * U < n) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = min(j0 + 2 * U + u, n - 1);
        xa[u] = lx(j);
        ya[u] = ly(j);
      }
    }
    if (j0 + U < n) taps(j0 + U, xb, yb);
  }
  if (more) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(u, n - 1);
      xa[u] = lxn(j);
      ya[u] = lyn(j);
    }
  }
  float *const sl = rl + slot * 320;
  sl[0] = h0;
  sl[64] = h1;
  sl[128] = h2;
  sl[192] = h3;
  sl[256] = h4;
  if (full) {
    m[0] = m[1] = m[2] = m[3] = m[4] = 0.f;
    int j = 0;
    auto run = [&](int s0, int s1) {  // slots [s0, s1) meet taps j, j + 1, ...
#pragma unroll 4
      for (int s = s0; s < s1; ++s, ++j) {
        const float wv = gw.g[j];
        const float *const r = rl + s * 320;
        m[0] = fmaf(wv, r[0], m[0]);
        m[1] = fmaf(wv, r[64], m[1]);
        m[2] = fmaf(wv, r[128], m[2]);
        m[3] = fmaf(wv, r[192], m[3]);
        m[4] = fmaf(wv, r[256], m[4]);
      }
    };
    run(slot + 1, n);
    run(0, slot + 1);
  }
}

// the first batch of a row (win_n_row's xa / ya on entry)
template <typename FX, typename FY>
__device__ __forceinline__ void win_n_first(int n, FX lx, FY ly, float (&xa)[kWinNBatch], float (&ya)[kWinNBatch]) {
#pragma unroll
  for (int u = 0; u < kWinNBatch; ++u) {
    const int j = min(u, n - 1);
    xa[u] = lx(j);
    ya[u] = ly(j);
  }
}

// NHWC taps, C a multiple of 64.  grid (Wo, strips, pairs), 64 threads, 1280 n bytes of dynamic LDS.  The strip's three
// output columns are banked in the lanes (lane l: output row 64 k + l of the current group of 64) and leave per group:
// stored by the first channel block, added to by the later ones, the last one scaling gamma by 1 / C
// (window_lds_body's flush).
template <typename P, bool GRP>
__device__ __forceinline__ void window_n_lanes_body(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W, int C,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, const GaussN &gw, int n,
    int strip, float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int K) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef typename P::T T;
  extern __shared__ __attribute__((aligned(16))) float ring_n[];
  const int lane = threadIdx.x;
  const int b = blockIdx.z;
  const int xi = GRP ? b / K : b;
  const bool lead = !GRP || b - xi * K == 0;
  const int Ho = H - (n - 1), Wo = W - (n - 1);
  const int ox = blockIdx.x;  // < Wo: the grid's x is Wo
  const int oy0 = blockIdx.y * strip;
  const int nout = min(strip, Ho - oy0);
  const int nrows = nout + n - 1;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  float *const rl = ring_n + lane;
  float acc_g = 0.f, acc_t = 0.f, acc_s = 0.f;
  for (int cb = 0; cb < C; cb += 64) {
    const int c = cb + lane;
    const float ix = q[0 * st + qo + c], iy = q[1 * st + qo + c], wc = wgt[(size_t)xi * ctot + coff + c];
    const T *px = fx + ((size_t)(xi * H + oy0) * W + ox) * C + c;  // rows oy0 .. oy0 + nrows - 1 <= H - 1,
    const T *py = fy + ((size_t)(b * H + oy0) * W + ox) * C + c;   // columns ox .. ox + n - 1 <= W - 1
    auto flush = [&](int orow) {
      const int r = (orow & ~63) + lane;
      if (r <= orow) {
        const size_t o = ((size_t)b * Ho + oy0 + r) * Wo + ox;
        const size_t og = ((size_t)xi * Ho + oy0 + r) * Wo + ox;
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
    int slot = 0;
    const size_t rowe = (size_t)W * C;  // elements between two rows
    float xa[kWinNBatch], ya[kWinNBatch];
    win_n_first(n, [&](int j) { return P::to_f(px[(size_t)j * C]); }, [&](int j) { return P::to_f(py[(size_t)j * C]); }, xa,
                ya);
    for (int rr = 0; rr < nrows; ++rr) {
      const bool full = rr >= n - 1;
      float m[5];
      win_n_row(n, gw, rl, slot, full, rr + 1 < nrows, [&](int j) { return P::to_f(px[(size_t)j * C]); },
                [&](int j) { return P::to_f(py[(size_t)j * C]); }, [&](int j) { return P::to_f(px[rowe + (size_t)j * C]); },
                [&](int j) { return P::to_f(py[rowe + (size_t)j * C]); }, xa, ya, m);
      px += rowe;
      py += rowe;
      slot = slot + 1 == n ? 0 : slot + 1;
      if (full) {
        float gs, ts, sss;
        win_n_terms(m, ix, iy, wc, gs, ts, sss);
        wave_sum3(gs, ts, sss);
        const int orow = rr - (n - 1);
        if (lane == (orow & 63)) {
          acc_g += gs;
          acc_t += ts;
          acc_s += sss;
        }
        if ((orow & 63) == 63 || orow == nout - 1) flush(orow);
      }
    }
  }
#endif
}

template <typename P>
__global__ __launch_bounds__(64) void adists_window_n_lanes_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W, int C,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, GaussN gw, int n, int strip,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw) {
  window_n_lanes_body<P, false>(fx, fy, H, W, C, q, B, ctot, coff, wgt, gw, n, strip, gamma, tw, sw, 1);
}
template <typename P>
__global__ __launch_bounds__(64) void adists_window_n_lanes_group_kernel(
    const typename P::T *__restrict__ fx, const typename P::T *__restrict__ fy, int H, int W, int C,
    const float *__restrict__ q, int B, int ctot, int coff, const float *__restrict__ wgt, GaussN gw, int n, int strip,
    float *__restrict__ gamma, float *__restrict__ tw, float *__restrict__ sw, int K) {
  window_n_lanes_body<P, true>(fx, fy, H, W, C, q, B, ctot, coff, wgt, gw, n, strip, gamma, tw, sw, K);
}

// Stage 0: three float planes, NCHW.  grid (ceil(Wo / 64), strips, pairs), 64 threads, 1280 n bytes of dynamic LDS.
// Nothing is reduced across lanes; the three channels are accumulated into the maps one after the other by the same
// lane (plain read-modify-write, window_planar_body's), gamma / 3 with the last.
template <bool GRP>
__device__ __forceinline__ void window_n_planar_body(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, const GaussN &gw, int n, int strip, float *__restrict__ gamma,
    float *__restrict__ tw, float *__restrict__ sw, int K) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) float ring_n[];
  const int lane = threadIdx.x;
  const int b = blockIdx.z;
  const int xi = GRP ? b / K : b;
  const bool lead = !GRP || b - xi * K == 0;
  const int Ho = H - (n - 1), Wo = W - (n - 1);
  const int ox = blockIdx.x * 64 + lane;
  const bool live = ox < Wo;
  const int oxc = live ? ox : Wo - 1;  // dead lanes re-read the last column and store nothing
  const int oy0 = blockIdx.y * strip;
  const int nout = min(strip, Ho - oy0);
  const int nrows = nout + n - 1;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  float *const rl = ring_n + lane;
  for (int c = 0; c < 3; ++c) {
    const float ix = q[0 * st + qo + c], iy = q[1 * st + qo + c], wc = wgt[(size_t)xi * ctot + coff + c];
    const float *px = x + ((size_t)(xi * 3 + c) * H + oy0) * W + oxc;  // columns oxc .. oxc + n - 1 <= W - 1
    const float *py = y + ((size_t)(b * 3 + c) * H + oy0) * W + oxc;
    int slot = 0;
    float xa[kWinNBatch], ya[kWinNBatch];
    win_n_first(n, [&](int j) { return px[j]; }, [&](int j) { return py[j]; }, xa, ya);
    for (int rr = 0; rr < nrows; ++rr) {
      const bool full = rr >= n - 1;
      float m[5];
      win_n_row(n, gw, rl, slot, full, rr + 1 < nrows, [&](int j) { return px[j]; }, [&](int j) { return py[j]; },
                [&](int j) { return px[W + j]; }, [&](int j) { return py[W + j]; }, xa, ya, m);
      px += W;
      py += W;
      slot = slot + 1 == n ? 0 : slot + 1;
      if (full && live) {
        float gterm, tt, ss;
        win_n_terms(m, ix, iy, wc, gterm, tt, ss);
        const size_t o = ((size_t)b * Ho + oy0 + rr - (n - 1)) * Wo + ox;
        if (lead) {
          float *const gp = gamma + ((size_t)xi * Ho + oy0 + rr - (n - 1)) * Wo + ox;
          const float gsum = c == 0 ? gterm : *gp + gterm;
          *gp = c == 2 ? gsum / 3.f : gsum;
        }
        tw[o] = c == 0 ? tt : tw[o] + tt;
        sw[o] = c == 0 ? ss : sw[o] + ss;
      }
    }
  }
#endif
}

__global__ __launch_bounds__(64) void adists_window_n_planar_kernel(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, GaussN gw, int n, int strip, float *__restrict__ gamma,
    float *__restrict__ tw, float *__restrict__ sw) {
  window_n_planar_body<false>(x, y, H, W, q, B, ctot, coff, wgt, gw, n, strip, gamma, tw, sw, 1);
}
__global__ __launch_bounds__(64) void adists_window_n_planar_group_kernel(
    const float *__restrict__ x, const float *__restrict__ y, int H, int W, const float *__restrict__ q, int B,
    int ctot, int coff, const float *__restrict__ wgt, GaussN gw, int n, int strip, float *__restrict__ gamma,
    float *__restrict__ tw, float *__restrict__ sw, int K) {
  window_n_planar_body<true>(x, y, H, W, q, B, ctot, coff, wgt, gw, n, strip, gamma, tw, sw, K);
}
