// Generic epilogue body of gemm_nt_split_kernel (gemm_split_f16.hip): accumulators -> outputs with every bound and
// flag tested (edge tiles, unaligned outputs, both outputs at once, long-K master accumulators).  A textual include
// rather than a lambda: a by-reference capture of the accumulator array keeps a scratch copy of it alive in the main
// loop for the larger instantiations.
{
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int mrow0 = m0 + (wm * TM + i) * 32;
      // (wave-uniform; a `break` here keeps the loop from unrolling in the larger instantiations, and a
      // dynamically indexed accumulator array lives in scratch)
      if (mrow0 < M) {
      float4 v4[32 / RPI];
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r];
          if (LONGK) v += master[i][j][r];
          stg[(4 * h + (r & 3) + 8 * (r >> 2)) * LDW + j * 32 + l31] = v;
        }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int p = 0; p < 32 / RPI; ++p) v4[p] = *reinterpret_cast<const float4 *>(stg + (p * RPI + er) * LDW + ec);
      __builtin_amdgcn_wave_barrier();
      float4 r4[32 / RPI];
      if (has_res) {
#pragma unroll
        for (int p = 0; p < 32 / RPI; ++p) {
          const int m = mrow0 + p * RPI + er;
          r4[p] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (m < M && nw < N) {
            const float *rp = res + (size_t)m * ldr + nw;
            if (vecR && nw + 3 < N) {
              r4[p] = *reinterpret_cast<const float4 *>(rp);
            } else {
              r4[p].x = rp[0];
              if (nw + 1 < N) r4[p].y = rp[1];
              if (nw + 2 < N) r4[p].z = rp[2];
              if (nw + 3 < N) r4[p].w = rp[3];
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < 32 / RPI; ++p) {
        const int m = mrow0 + p * RPI + er;
        if (m >= M) continue;
        if (nw >= N) {
          // pad columns N .. ldcs/2 of the split output are the zero K padding of the consumer
          if (Cs && nw < (int)(ldcs >> 1)) {
            unsigned short *sp = Cs + (size_t)m * ldcs + (o_plain ? nw : (nw >> 5) * 64 + (nw & 31));
            *reinterpret_cast<uint2 *>(sp) = make_uint2(0u, 0u);
            // (reduced-precision mode: no lo half of C_split is written, padding included - include/cra5_amd.h)
            if (NPROD == 3) *reinterpret_cast<uint2 *>(sp + 32) = make_uint2(0u, 0u);
          }
          continue;
        }
        float o[4] = {v4[p].x, v4[p].y, v4[p].z, v4[p].w};
        const float rr[4] = {r4[p].x, r4[p].y, r4[p].z, r4[p].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = o[c] * wscale_inv + bv[c];
        if (do_gelu) {   // two columns per packed-fp32 instruction (gelu_erf2 == gelu_erf per element)
          const float2v g01 = gelu_erf2(float2v{o[0], o[1]}), g23 = gelu_erf2(float2v{o[2], o[3]});
          o[0] = g01[0];
          o[1] = g01[1];
          o[2] = g23[0];
          o[3] = g23[1];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = o[c];
          if (has_res) v += rr[c];
          o[c] = (nw + c < N) ? v : 0.f;
        }
        if (C) {
          float *cp = C + (size_t)m * ldc + nw;
          if (vecC && nw + 3 < N) {
            *reinterpret_cast<float4 *>(cp) = make_float4(o[0], o[1], o[2], o[3]);
          } else {
            cp[0] = o[0];
            if (nw + 1 < N) cp[1] = o[1];
            if (nw + 2 < N) cp[2] = o[2];
            if (nw + 3 < N) cp[3] = o[3];
          }
        }
        if (Cs) {
          // split layout: 128-byte chunk per 32 columns = [32 hi | 32 lo]; 4 columns -> 8 B + 8 B.
          // Columns >= N inside the group are written as zero (they are K padding of the consumer).
          unsigned h01, l01, h23, l23;
          cra5_split_pair(o[0], o[1], h01, l01);
          cra5_split_pair(o[2], o[3], h23, l23);
          unsigned short *sp = Cs + (size_t)m * ldcs + (o_plain ? nw : (nw >> 5) * 64 + (nw & 31));
          *reinterpret_cast<uint2 *>(sp) = make_uint2(h01, h23);
          if (NPROD == 3) *reinterpret_cast<uint2 *>(sp + 32) = make_uint2(l01, l23);
        }
      }
      }
    }
}
