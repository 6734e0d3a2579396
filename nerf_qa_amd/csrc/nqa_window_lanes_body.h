// Body of adists_window_lanes_kernel and of its group form adists_window_lanes_group_kernel (nqa_adists.hip), included
// once into each with NQA_LANES_GROUP 0 / 1: the two kernels are ONE text, and the pairwise one compiles from exactly
// the tokens it always had (as an inlined device function its register allocation drifted by a few VGPRs).
//   pairwise: pair b reads x image b, weights row b, and writes its gamma map;
//   group:    pair b = r * K + k reads x image and weights row r = b / K; gamma, a function of x alone, is written once
//             per reference, by the k = 0 pair, at image r.
// No include guard: this is a fragment of a function body.
  typedef typename P::T T;
  // the wave index as a provably uniform value, so the row pointers and loop bounds stay scalar
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.z;
#if NQA_LANES_GROUP
  const int xi = b / K;
  const bool lead = b - xi * K == 0;
#else
  const int xi = b;
  constexpr bool lead = true;
#endif
  const int Ho = H - (kWin - 1), Wo = W - (kWin - 1);
  const int ox = blockIdx.x * 4 + wave;  // 4 adjacent columns per block: their neighbour loads overlap in L1
  if (ox >= Wo) return;
  const int oy0 = blockIdx.y * 64;
  const int nout = min(64, Ho - oy0);
  const int nrows = nout + kWin - 1;
  const size_t st = (size_t)B * ctot, qo = (size_t)b * ctot + coff;
  float acc_g = 0.f, acc_t = 0.f, acc_s = 0.f;  // lane l: output row oy0 + l
  for (int cb = 0; cb < C; cb += 64) {
    const int c = cb + lane;
    const float ix = q[0 * st + qo + c], iy = q[1 * st + qo + c], wc = wgt[(size_t)xi * ctot + coff + c];
    const T *px = fx + ((size_t)(xi * H + oy0) * W + ox) * C + cb;  // wave-uniform; the lane is added per load
    const T *py = fy + ((size_t)(b * H + oy0) * W + ox) * C + cb;
    // ring of the last 21 rows' horizontal sums, slot = grp*7 + sub (a dynamically indexed ring -- a switch
    // over 21 slots -- makes hipcc shuttle all of it through AGPRs every row, so the row loop is unrolled).
    // The five running sums travel as two float pairs + one float so that the 2 x 21 taps per
    // (pixel, channel) are packed v_pk_fma_f32 / v_pk_mul_f32: 4 + 3 instructions per tap pair.
    f32x2 r01[3][7], r23[3][7];
    float r4[3][7];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int u = 0; u < 7; ++u) {
        r01[g][u] = r23[g][u] = (f32x2){0.f, 0.f};
        r4[g][u] = 0.f;
      }
    // 21 rows per trip, fully unrolled: the ring slot (grp*7 + sub) of every row body is a compile-time
    // constant, so a row's sums drop into their slot without selects and the vertical tap weights are
    // immediates of the kernel-argument window (no table loads)
    for (int rr0 = 0; rr0 < nrows; rr0 += 21) {
#pragma unroll
      for (int grp = 0; grp < 3; ++grp)
#pragma unroll
      for (int sub = 0; sub < 7; ++sub) {
        const int rr = rr0 + grp * 7 + sub;
        if (rr < nrows) {
          // all 42 loads go out back to back before any arithmetic (left to itself hipcc pairs each
          // load with its use and pays the memory latency 21 times per row)
          T xr[kWin], yr[kWin];
#pragma unroll
          for (int j = 0; j < kWin; ++j) {
            xr[j] = px[(size_t)j * C + lane];
            yr[j] = py[(size_t)j * C + lane];
          }
          px += (size_t)W * C;
          py += (size_t)W * C;
          __builtin_amdgcn_sched_barrier(0);
          f32x2 h01 = {0.f, 0.f}, h23 = {0.f, 0.f};
          float h4 = 0.f;
#pragma unroll
          for (int j = 0; j < kWin; ++j) {
            const f32x2 v = {P::to_f(xr[j]), P::to_f(yr[j])};
            const f32x2 gv = gw.g[j] * v;
            h01 += gv;
            h23 = gv * v + h23;
            h4 = fmaf(gv[0], v[1], h4);
          }
          r01[grp][sub] = h01;
          r23[grp][sub] = h23;
          r4[grp][sub] = h4;
          if (rr >= kWin - 1) {
            f32x2 m01 = {0.f, 0.f}, m23 = {0.f, 0.f};
            float m4 = 0.f;
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
              for (int u = 0; u < 7; ++u) {
                const float wv = gw.g[(kWin - 1 - (grp * 7 + sub) + g * 7 + u) % kWin];  // slot (g,u) at this phase
                m01 = wv * r01[g][u] + m01;
                m23 = wv * r23[g][u] + m23;
                m4 = fmaf(wv, r4[g][u], m4);
              }
            const float m0 = m01[0], m1 = m01[1], m2 = m23[0], m3 = m23[1];
            const float gterm = div_nr(m2 - m0 * m0, m0 + 1e-12f);
            const float mx = ix * m0, my = iy * m1;
            const float vx = ix * ix * m2 - mx * mx, vy = iy * iy * m3 - my * my;
            const float cov = ix * iy * m4 - mx * my;
            const float tt = wc * div_nr(2.f * mx * my + 1e-6f, mx * mx + my * my + 1e-6f);
            const float ss = wc * div_nr(2.f * cov + 1e-6f, vx + vy + 1e-6f);
            const float gs = wave_sum(gterm), ts = wave_sum(tt), sss = wave_sum(ss);
            if (lane == rr - (kWin - 1)) {
              acc_g += gs;
              acc_t += ts;
              acc_s += sss;
            }
          }
        }
      }
    }
  }
  if (lane < nout) {
    const size_t o = ((size_t)b * Ho + oy0 + lane) * Wo + ox;
    if (lead) gamma[((size_t)xi * Ho + oy0 + lane) * Wo + ox] = acc_g / (float)C;
    tw[o] = acc_t;
    sw[o] = acc_s;
  }
