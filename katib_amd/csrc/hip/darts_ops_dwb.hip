// DARTS depthwise / pooling backward kernels (dw_bwd tiles, dw_bwd_plane, pool_bwd)
// and their launch heuristics. See darts_ops.hip for the design notes.
#include "darts_ops_dev.h"

namespace katib_hip {

// ------------------------------------------------------------------------------------------------
// dw_bwd: transposed depthwise. For own output rows [oy0, oy0+TR): dW_dw += dd * act(in);
// for own input rows [oy0*S, (oy0+TR)*S): ga = sum_taps dw * dd, masked by act'(in).
// PREBN: input = z_prev (pre-BN), act = relu(BN(.)) -> writes g_prev and reductions for BN bwd.
// else  : input = x, act = relu -> gx += ga * (x > 0).
// ------------------------------------------------------------------------------------------------
template <int K, int DIL, int S, bool PREBN>
__global__ void __launch_bounds__(256) dw_bwd_kernel(DwBwdBatch bt) {
  const DwBwdArgs& a = bt.e[blockIdx.y];
  constexpr int P = 64, KK = K * K;
  const int C = a.C, H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo;
  const int TR = P / Wo;
  const int tiles = Ho / TR;
  const int ntiles = a.N * tiles;
  const int pad = a.pad;
  const int r = (K - 1) / 2 * DIL;         // == pad for these ops
  const int h = (r + S - 1) / S;           // halo output rows
  const int OR = TR + 2 * h;               // staged dd rows
  const int IR = (TR - 1) * S + (K - 1) * DIL + 1;
  const int IW = (Wo - 1) * S + (K - 1) * DIL + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sDD = smem;                        // [CH][OR][Wo]
  float* sIn = sDD + a.chunk * OR * Wo;     // [CH][IR][IW]
  float* sMean = sIn + a.chunk * IR * IW;   // [C]
  float* sInv = sMean + C;
  float* sRed = sInv + C;                   // [2C] block-local BN-bwd partials (PREBN)
  float* sGW = sRed + 2 * C;                // [C*K*K] block-local depthwise weight grads
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int c = tid; c < C; c += 256) {
    if (PREBN) bn_coeffs(a.inbn, c, sMean[c], sInv[c]);
    sRed[c] = 0.f;
    sRed[C + c] = 0.f;
  }
  if (a.gW)
    for (int i = tid; i < C * KK; i += 256) sGW[i] = 0.f;
  __syncthreads();
  const int own_in = TR * S;  // own input rows [oy0*S, oy0*S + own_in)
  const int nq = own_in * W;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = t / tiles, oy0 = (t % tiles) * TR;
    const int iy0 = oy0 * S - pad;
    const size_t xin = (size_t)n * C * H * W;
    const float* ddn = a.dd + (size_t)n * C * Ho * Wo;
    for (int c0 = 0; c0 < C; c0 += a.chunk) {
      const int cn = min(a.chunk, C - c0);
      #pragma unroll 4  // keep several global loads of the staging pass in flight
      for (int i = tid; i < cn * OR * Wo; i += 256) {
        int cc = i / (OR * Wo), rr = (i / Wo) % OR, q = i % Wo;
        int oy = oy0 - h + rr;
        sDD[i] = (oy >= 0 && oy < Ho) ? ddn[((size_t)(c0 + cc) * Ho + oy) * Wo + q] : 0.f;
      }
      if (a.gW) {
        #pragma unroll 4  // keep several global loads of the staging pass in flight
        for (int i = tid; i < cn * IR * IW; i += 256) {
          int cc = i / (IR * IW), rr = (i / IW) % IR, q = i % IW;
          int iy = iy0 + rr, ix = -pad + q, c = c0 + cc;
          float v = 0.f;
          if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = xval<PREBN>(a.x, xin + ((size_t)c * H + iy) * W + ix);
            if (PREBN) v = (v - sMean[c]) * sInv[c];
            v = fmaxf(v, 0.f);
          }
          sIn[i] = v;
        }
      }
      __syncthreads();
      // weight grads: thread per (channel, tap), summed over the tile's 64 output pixels
      if (a.gW) {
        for (int job = tid; job < cn * KK; job += 256) {
          const int cc = job / KK, tap = job % KK, ky = tap / K, kx = tap % K;
          const float* dd = sDD + (cc * OR + h) * Wo;
          const float* in = sIn + (cc * IR + ky * DIL) * IW + kx * DIL;
          float s = 0.f;
          for (int ty = 0; ty < TR; ++ty)
            for (int tx = 0; tx < Wo; ++tx) s += dd[ty * Wo + tx] * in[ty * S * IW + tx * S];
          sGW[(c0 + cc) * KK + tap] += s;  // unique owner
        }
      }
      // input grads for own input rows: the tap geometry depends only on the pixel q, so it
      // is computed once per pixel (branch-free masks) and reused for every channel. A tile
      // owns nq = 64*S*S input pixels: at stride 1 the block's 4 waves take 4 channel groups
      // of the same 64 pixels (wave-uniform channel -> scalar weight loads, wave-level sums).
      const int qspan = (nq < 256 && 256 % nq == 0) ? nq : 256;
      const int G = 256 / qspan;
      for (int q0 = 0; q0 < nq; q0 += qspan) {
        const int q = q0 + tid % qspan;
        const int cg = __builtin_amdgcn_readfirstlane(tid / qspan);
        const int rr = q / W, ix = q - rr * W;
        const int iy = oy0 * S + rr;
        const bool ok = q < nq && iy < H;
        int srow[K], ocol[K];
        float mrow[K], mcol[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          int ty = iy + pad - k * DIL;  // = oy * S when valid
          int oy = ty >= 0 ? ty / S : -1;
          bool v = ok && ty >= 0 && (ty % S) == 0 && oy < Ho;
          srow[k] = v ? oy - (oy0 - h) : 0;
          mrow[k] = v ? 1.f : 0.f;
          int tx = ix + pad - k * DIL;
          int ox = tx >= 0 ? tx / S : -1;
          bool u = ok && tx >= 0 && (tx % S) == 0 && ox < Wo;
          ocol[k] = u ? ox : 0;
          mcol[k] = u ? 1.f : 0.f;
        }
        for (int cc = cg; cc < cn; cc += G) {
          const int c = c0 + cc;
          const float* wk = a.dw + c * KK;  // wave-uniform -> scalar loads
          const float* dd = sDD + cc * OR * Wo;
          float ga = 0.f;
#pragma unroll
          for (int ky = 0; ky < K; ++ky) {
            float rowacc = 0.f;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) rowacc += mcol[kx] * wk[ky * K + kx] * dd[srow[ky] * Wo + ocol[kx]];
            ga += mrow[ky] * rowacc;
          }
          const size_t xi = ((size_t)(n * C + c) * H + iy) * W + ix;
          if (PREBN) {
            float g = 0.f, gy = 0.f;
            if (ok) {
              float y = (xval<true>(a.x, xi) - sMean[c]) * sInv[c];
              g = y > 0.f ? ga : 0.f;
              gy = g * y;
              a.gout[xi] = g;
            }
            if (a.red) {
              g = wave_sum(g);
              gy = wave_sum(gy);
              if (lane == 0) {
                atomicAdd(sRed + c, g);  // one LDS atomic per wave per channel
                atomicAdd(sRed + C + c, gy);
              }
            }
          } else if (ok) {
            const float gm = xval<false>(a.x, xi) > 0.f ? ga : 0.f;
            if (a.overwrite) a.gout[xi] = gm;
            else if (gm != 0.f) a.gout[xi] += gm;
          }
        }
      }
      __syncthreads();
    }
  }
  if (PREBN && a.red)
    for (int i = tid; i < 2 * C; i += 256) atomicAdd(a.red + rep_slot() * 2 * C + i, (double)sRed[i]);
  if (a.gW)
    for (int i = tid; i < C * KK; i += 256) atomicAdd(a.gW + (size_t)rep_slot() * a.gstride + i, sGW[i]);
}

// ------------------------------------------------------------------------------------------------
// pool_bwd: the gradient of one cell state from every edge that reads it (PoolBwdArgs), per (n,c)
// plane: gx (+)= avg^T(sum_e dz_avg_e) + max^T(sum_e dz_max_e) + sum_e (wid_e * dout_e + conv parts_e)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// the entry's sources read where they are used, through the kernel-argument segment: copied into
// registers with the rest of the entry they are ~100 scalar registers, all live from the first
// instruction on, and most of them spill
typedef const PoolBwdSrc __attribute__((address_space(4))) * PoolSrcPtr;

template <int S, bool V4 = false>
__device__ __forceinline__ void pool_bwd_body(const PoolBwdArgs& a, PoolSrcPtr src, const int bx) {
  const int C = a.C, H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, HWo = Ho * Wo;
  const int nc = bx, c = nc % C;
  const size_t ob = (size_t)nc * HWo;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sGa = smem;                                          // [HWo] sum_e dz_avg / window count
  float* sGm = smem + HWo;                                    // [HWo] sum_e dz_max
  unsigned char* sArg = (unsigned char*)(smem + 2 * HWo);     // [HWo] argmax tap
  // the plane's coefficients: (mean, 1 / std) of both pooled tensors, then per source the two
  // BN-backward means of its avg pool and of its max pool
  __shared__ float sCo[4 + 4 * kMaxShare];
  KSTAMP(0);
  // every replica pair-sum in ONE memory round trip: 16-lane groups take the avg pool's BN
  // statistics, the max pool's, and per source the BN-backward sums (S1, S2) of its avg and of its
  // max pool - folded (rep 1) or not (rep kRep: two loads per lane). One thread per BN walking kRep
  // replicas in rounds of 8 was four dependent round trips (~2.8 us of a ~10 us workgroup, phase
  // stamps r06). The sources are picked with constant indices: a dynamic index into the argument
  // copy would send it to scratch
  if (threadIdx.x < 16 * (2 + 2 * kMaxShare)) {
    const int grp = threadIdx.x >> 4, j = threadIdx.x & 15;
    const bool stats = grp < 2;
    const BNRef& b = grp & 1 ? a.bnm : a.bna;
    const bool on = (grp & 1 ? a.zm != nullptr : a.za != nullptr);
    const double* p1 = nullptr;
    size_t off2 = 0;
    int rep = 0, rs = 0;
#pragma unroll
    for (int e = 0; e < kMaxShare; ++e) {
      if (e < a.nsrc && (grp >> 1) == e + 1) {
        const float* gw = grp & 1 ? src[e].m.w : src[e].a.w;
        const double* g1 = grp & 1 ? src[e].m.S1 : src[e].a.S1;
        const double* g2 = grp & 1 ? src[e].m.S2 : src[e].a.S2;
        const int grep = grp & 1 ? src[e].m.rep : src[e].a.rep;
        const int grs = grp & 1 ? src[e].m.rstride : src[e].a.rstride;
        if (gw && g1) {
          p1 = g1;
          off2 = g2 - g1;
          rep = grep;
          rs = grep == 1 ? 0 : grs;
        }
      }
    }
    double s = 0.0, s2 = 0.0;
    if (stats) {
      if (on && !b.eval) {
        for (int r = j; r < b.rep; r += 16) {
          s += b.sums[(size_t)r * b.rstride + c];
          s2 += b.sums[(size_t)r * b.rstride + b.C + c];
        }
      }
    } else if (p1) {
      for (int r = j; r < rep; r += 16) {
        s += p1[(size_t)r * rs + c];
        s2 += p1[(size_t)r * rs + off2 + c];
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    if (j == 0) {
      float* o = sCo + 2 * grp;  // stats: 0 / 2; source e: 4 + 4 e (avg), 4 + 4 e + 2 (max)
      if (stats) {
        if (!on || b.eval) {  // eval: every source scales by its own running variance; zhat is unused
          o[0] = 0.f;
          o[1] = 1.f;
        } else {  // as bn_moments / bn_coeffs
          const double m = s * (double)b.inv_count;
          double v = s2 * (double)b.inv_count - m * m;
          if (v < 0) v = 0;
          o[0] = (float)m;
          o[1] = rsqrtf((float)v + b.eps);
        }
      } else {  // as gs_means (no sums - eval, or the edge lacks this pool: 0)
        o[0] = (float)(s * (double)b.inv_count);
        o[1] = (float)(s2 * (double)b.inv_count);
      }
    }
  }
  __syncthreads();
  KSTAMP(1);
  // (the same values in every lane: kept in scalar registers)
  const float ma = wave_uniform(sCo[0]), ia = wave_uniform(sCo[1]), mm = wave_uniform(sCo[2]), im = wave_uniform(sCo[3]);
  // per source: weight * 1 / std of each pool (0: the edge lacks it), its BN-backward means, its
  // identity weight
  float ca[kMaxShare], a1[kMaxShare], a2[kMaxShare], cm[kMaxShare], m1[kMaxShare], m2[kMaxShare], wid[kMaxShare];
#pragma unroll
  for (int e = 0; e < kMaxShare; ++e) {
    ca[e] = cm[e] = wid[e] = 0.f;
    a1[e] = wave_uniform(sCo[4 + 4 * e]);
    a2[e] = wave_uniform(sCo[5 + 4 * e]);
    m1[e] = wave_uniform(sCo[6 + 4 * e]);
    m2[e] = wave_uniform(sCo[7 + 4 * e]);
    if (e < a.nsrc) {
      if (a.za && src[e].a.w)
        ca[e] = src[e].a.w[src[e].a.widx] * (a.bna.eval ? rsqrtf(src[e].a.rvar[c] + a.bna.eps) : ia);
      if (a.zm && src[e].m.w)
        cm[e] = src[e].m.w[src[e].m.widx] * (a.bnm.eval ? rsqrtf(src[e].m.rvar[c] + a.bnm.eps) : im);
      if (src[e].w_id) wid[e] = src[e].w_id[src[e].id_idx];
    }
  }
  if constexpr (V4) {
    // 4 consecutive outputs / input pixels per thread: every operand one 16-byte (amax: 4-byte)
    // access instead of four 4-byte ones - a quarter of the memory requests in flight for the
    // same bytes (HWo, H*W % 4 == 0 and every operand 16-byte aligned: host-checked)
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (int o4 = threadIdx.x * 4; o4 < HWo; o4 += 1024) {
      // every load of the pass issued before the first use (they sit behind wave-uniform tests, and
      // a load consumed inside its own test is one memory round trip per test); then zhat once per
      // pixel and every source's BN backward of both pools summed (a source without that pool: c = 0)
      f4 za4 = {0.f, 0.f, 0.f, 0.f}, zm4 = {0.f, 0.f, 0.f, 0.f}, gd[kMaxShare];
      unsigned am4 = 0xffffffffu;
      if (a.za) za4 = zld4(a.za + ob + o4);
      if (a.zm) {
        zm4 = zld4(a.zm + ob + o4);
        am4 = *reinterpret_cast<const unsigned*>(a.amax + ob + o4);
      }
#pragma unroll
      for (int e = 0; e < kMaxShare; ++e) {
        gd[e] = f4{0.f, 0.f, 0.f, 0.f};
        if (e < a.nsrc && ((a.za && src[e].a.w) || (a.zm && src[e].m.w)))
          gd[e] = *reinterpret_cast<const f4*>(src[e].dout + ob + o4);
      }
      const f4 zha = (za4 - ma) * ia, zhm = (zm4 - mm) * im;
      f4 da = {0.f, 0.f, 0.f, 0.f}, dm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < kMaxShare; ++e) {
        da += ca[e] * (gd[e] - a1[e] - zha * a2[e]);
        dm += cm[e] * (gd[e] - m1[e] - zhm * m2[e]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = o4 + t, oy = o / Wo, ox = o - oy * Wo;
        const int y0 = max(oy * S - 1, 0), y1 = min(oy * S + 1, H - 1);
        const int x0 = max(ox * S - 1, 0), x1 = min(ox * S + 1, W - 1);
        sGa[o] = da[t] / (float)((y1 - y0 + 1) * (x1 - x0 + 1));
      }
      *reinterpret_cast<f4*>(sGm + o4) = dm;
      *reinterpret_cast<unsigned*>(sArg + o4) = am4;
    }
    __syncthreads();
    KSTAMP(2);
    const size_t pb = (size_t)nc * H * W;
    for (int q4 = threadIdx.x * 4; q4 < H * W; q4 += 1024) {
      f4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < kMaxShare; ++e) {  // every source's identity skip and conv input-gradient parts:
        if (e < a.nsrc) {                    // a source's loads all issued before the first is used
          f4 dv = {0.f, 0.f, 0.f, 0.f}, xv[4];
          if (src[e].w_id) dv = *reinterpret_cast<const f4*>(src[e].dout + pb + q4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            xv[j] = f4{0.f, 0.f, 0.f, 0.f};
            if (j < src[e].nextra) xv[j] = *reinterpret_cast<const f4*>(src[e].extra[j] + pb + q4);
          }
          g += wid[e] * dv;
#pragma unroll
          for (int j = 0; j < 4; ++j) g += xv[j];
        }
      }
      const int iy = q4 / W, ix0 = q4 - iy * W;  // 4 pixels of one row (W % 4 == 0)
      if constexpr (S == 1) {
        // stride 1: the quad's 3 x 6 window of outputs (rows iy - 1 .. iy + 1, columns ix0 - 1 ..
        // ix0 + 4; Ho = H, Wo = W) read once - a 16-byte / 4-byte LDS read for the middle four
        // columns and two scalars per row and array - instead of 9 neighbours x 3 arrays per pixel
        // (27 reads per row instead of 108 per quad); out-of-range neighbours read as ga = gm = 0 and
        // tap 255, and the sums run in the per-pixel loop's order
        float wa[3][6], wm[3][6];
        unsigned char wt[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int oy = iy - 1 + r;
          const bool rok = oy >= 0 && oy < Ho;
          const int o = (rok ? oy : 0) * Wo + ix0;
          const f4 ga4 = *reinterpret_cast<const f4*>(sGa + o), gm4 = *reinterpret_cast<const f4*>(sGm + o);
          const unsigned t4 = *reinterpret_cast<const unsigned*>(sArg + o);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            wa[r][k + 1] = rok ? ga4[k] : 0.f;
            wm[r][k + 1] = rok ? gm4[k] : 0.f;
            wt[r][k + 1] = rok ? (unsigned char)(t4 >> (8 * k)) : 255;
          }
          const bool lok = rok && ix0 > 0, hok = rok && ix0 + 4 < Wo;
          wa[r][0] = lok ? sGa[o - 1] : 0.f;
          wm[r][0] = lok ? sGm[o - 1] : 0.f;
          wt[r][0] = lok ? sArg[o - 1] : 255;
          wa[r][5] = hok ? sGa[o + 4] : 0.f;
          wm[r][5] = hok ? sGm[o + 4] : 0.f;
          wt[r][5] = hok ? sArg[o + 4] : 255;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float v = 0.f;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cx = 0; cx < 3; ++cx) {  // output (iy - 1 + r, ix0 + t - 1 + cx): tap (2 - r) * 3 + (2 - cx)
              v += wa[r][t + cx];
              if (wt[r][t + cx] == (2 - r) * 3 + (2 - cx)) v += wm[r][t + cx];
            }
          g[t] += v;
        }
        f4* dst = reinterpret_cast<f4*>(a.gx + pb + q4);
        *dst = a.overwrite ? g : *dst + g;
        continue;
      }
      if constexpr (S == 2) {
        // stride 2: the quad (ix0 = 4k) meets output columns 2k .. 2k + 2 and output rows m = iy / 2
        // and, for odd iy, m + 1 - a 2 x 3 window read once (an 8-byte pair + a scalar per row and
        // array); pixel t reads columns t / 2 .. (t + 1) / 2. Out-of-range outputs read as 0 / tap 255
        float wa[2][3], wm[2][3];
        unsigned char wt[2][3];
        const int m = iy >> 1, k2 = ix0 >> 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int oy = m + r;
          const bool rok = oy < Ho && (r == 0 || (iy & 1));
          const int o = (rok ? oy : m) * Wo + k2;
          typedef float f2 __attribute__((ext_vector_type(2)));
          const f2 ga2 = *reinterpret_cast<const f2*>(sGa + o), gm2 = *reinterpret_cast<const f2*>(sGm + o);
          const unsigned short t2 = *reinterpret_cast<const unsigned short*>(sArg + o);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            wa[r][c] = rok ? ga2[c] : 0.f;
            wm[r][c] = rok ? gm2[c] : 0.f;
            wt[r][c] = rok ? (unsigned char)(t2 >> (8 * c)) : 255;
          }
          const bool hok = rok && k2 + 2 < Wo;
          wa[r][2] = hok ? sGa[o + 2] : 0.f;
          wm[r][2] = hok ? sGm[o + 2] : 0.f;
          wt[r][2] = hok ? sArg[o + 2] : 255;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float v = 0.f;
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = t / 2; c <= (t + 1) / 2; ++c) {  // output (m + r, 2k + c)
              v += wa[r][c];
              if (wt[r][c] == (iy - 2 * (m + r) + 1) * 3 + (t - 2 * c + 1)) v += wm[r][c];
            }
          g[t] += v;
        }
        f4* dst = reinterpret_cast<f4*>(a.gx + pb + q4);
        *dst = a.overwrite ? g : *dst + g;
        continue;
      }
      const int oy_lo = iy - 1 < 0 ? 0 : (iy - 1 + S - 1) / S, oy_hi = min((iy + 1) / S, Ho - 1);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ix = ix0 + t;
        const int ox_lo = ix - 1 < 0 ? 0 : (ix - 1 + S - 1) / S, ox_hi = min((ix + 1) / S, Wo - 1);
        float v = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
          for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const int o = oy * Wo + ox;
            v += sGa[o];
            if (sArg[o] == (iy - oy * S + 1) * 3 + (ix - ox * S + 1)) v += sGm[o];
          }
        g[t] += v;
      }
      f4* dst = reinterpret_cast<f4*>(a.gx + pb + q4);
      *dst = a.overwrite ? g : *dst + g;
    }
    KSTAMP(3);
    return;
  }
  for (int o = threadIdx.x; o < HWo; o += 256) {
    int oy = o / Wo, ox = o % Wo;
    const float zha = a.za ? (z2f(a.za[ob + o]) - ma) * ia : 0.f;
    const float zhm = a.zm ? (z2f(a.zm[ob + o]) - mm) * im : 0.f;
    float da = 0.f, dm = 0.f;
#pragma unroll
    for (int e = 0; e < kMaxShare; ++e) {
      if (e < a.nsrc && ((a.za && src[e].a.w) || (a.zm && src[e].m.w))) {
        const float g = src[e].dout[ob + o];
        if (a.za && src[e].a.w) da += ca[e] * (g - a1[e] - zha * a2[e]);
        if (a.zm && src[e].m.w) dm += cm[e] * (g - m1[e] - zhm * m2[e]);
      }
    }
    int y0 = max(oy * S - 1, 0), y1 = min(oy * S + 1, H - 1);
    int x0 = max(ox * S - 1, 0), x1 = min(ox * S + 1, W - 1);
    sGa[o] = da / (float)((y1 - y0 + 1) * (x1 - x0 + 1));
    sGm[o] = dm;
    sArg[o] = a.zm ? a.amax[ob + o] : 255;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < H * W; q += 256) {
    int iy = q / W, ix = q % W;
    float g = 0.f;
    // outputs whose 3x3 window (pad 1) covers (iy, ix): oy*S - 1 <= iy <= oy*S + 1
    int oy_lo = iy - 1 < 0 ? 0 : (iy - 1 + S - 1) / S, oy_hi = min((iy + 1) / S, Ho - 1);
    int ox_lo = ix - 1 < 0 ? 0 : (ix - 1 + S - 1) / S, ox_hi = min((ix + 1) / S, Wo - 1);
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int o = oy * Wo + ox;
        g += sGa[o];
        int tap = (iy - oy * S + 1) * 3 + (ix - ox * S + 1);
        if (sArg[o] == tap) g += sGm[o];
      }
    }
#pragma unroll
    for (int e = 0; e < kMaxShare; ++e) {  // identity skips and conv input grads (constant indices: a
      if (e < a.nsrc) {                    // dynamic index into the argument copy sends it to scratch)
        if (src[e].w_id) g += wid[e] * src[e].dout[(size_t)nc * H * W + q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < src[e].nextra) g += src[e].extra[j][(size_t)nc * H * W + q];
      }
    }
    if (a.overwrite) a.gx[(size_t)nc * H * W + q] = g;
    else a.gx[(size_t)nc * H * W + q] += g;
  }
}

// stride-1 and stride-2 pool backward of several cell states in one launch (different states: different gx)
template <bool V4>
__global__ void __launch_bounds__(256) pool_bwd_multi_kernel(PoolBwdBatch bt) {
  const PoolBwdArgs a = bt.e[blockIdx.y];  // copy: see dwpw_plane_multi_kernel
  if ((int)blockIdx.x >= a.N * a.C) return;
  // (bt is the kernel's only argument: it starts the kernel-argument segment)
  typedef const PoolBwdBatch __attribute__((address_space(4))) * BatchPtr;
  PoolSrcPtr src = ((BatchPtr)__builtin_amdgcn_kernarg_segment_ptr())->e[blockIdx.y].src;
  if (a.S == 1) pool_bwd_body<1, V4>(a, src, blockIdx.x);
  else pool_bwd_body<2, V4>(a, src, blockIdx.x);
}


// ------------------------------------------------------------------------------------------------
// dw_bwd_plane: dw_bwd for narrow layers (C <= 16), the backward twin of dwpw_plane. One
// workgroup per (image, band of input rows): the dd rows the band's input pixels reach (plus a
// zero border of PO = ceil(pad/S), so every tap lands inside the staged grid) and act(in) of the
// band are staged with one coalesced burst (and, when accumulating, the current input gradient),
// then
//   input grads : thread per own input pixel, all channels: ga = sum_taps w * dd (transposed
//                 depthwise gather from LDS), masked by act'(in); PREBN keeps the BN-backward
//                 sums per thread and reduces once per block;
//   weight grads: thread per (channel, tap[, pixel part]) summing act(in) * dd over the band.
// Every input pixel belongs to exactly one band, so both sums are complete without overlap.
// Replaces the 64-pixel tiles whose halo rows were re-staged per tile behind two barriers.
// ------------------------------------------------------------------------------------------------
template <int K, int DIL, int S, bool PREBN, int C>
__device__ __forceinline__ void dw_bwd_plane_body(const DwBwdArgs& a, const int bx, const int nb, const int dbg) {
  constexpr int KK = K * K, PAD = (K - 1) / 2 * DIL, PO = (PAD + S - 1) / S, SH = S == 2 ? 1 : 0;
  const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo;
  // channel groups: depthwise backward never mixes channels, so wider layers run as a.C / C
  // independent C-channel groups (blockIdx.x = (image * nb + band) * G + group)
  const int G = a.C / C, grp = bx % G, nbx = bx / G, c0 = grp * C;
  const int n = nbx / nb, band = nbx - n * nb;
  const int BRi = H / nb, iy0 = band * BRi, nrow = BRi;
  const int oyA = (iy0 - PAD) >> SH;                 // floor division (S in {1, 2})
  const int oyB = (iy0 + nrow - 1 + PAD) >> SH;
  // row pitches of the staged planes: darts_plane_layout.h (stride 1: tile_pitch for the tile map)
  const int ODR = oyB - oyA + 1, ODW = plane_pitch(Wo + 2 * PO, S), PIN = plane_pitch(W, S), NP = nrow * W;
  const bool accum = !PREBN && !a.overwrite;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sWt = smem;                    // [C][KK] depthwise weights (dwb_head_floats)
  float* sGW = smem + C * 25;           // [C][KK] block-local depthwise weight gradients
  float* sDD = smem + dwb_head_floats(C);  // [C][ODR][ODW]
  float* sIn = sDD + C * ODR * ODW;     // [C][nrow][PIN] act(in)
  float* sOld = sIn + C * nrow * PIN;   // [C][nrow][PIN] current gradient (accumulate mode)
  __shared__ float sMean[C], sInv[C], sRed[2 * C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  KSTAMP(0);
  // the group's depthwise weights in LDS, loaded with the prologue: read from global memory
  // inside the tap loops, every weight was its own load + s_waitcnt vmcnt(0) (the compiler may
  // not hoist them above the gradient stores, which could alias) - 9-25 serial round trips per
  // channel in the middle of the compute phase
  for (int i = tid; i < C * KK; i += 256) {
    sGW[i] = 0.f;
    sWt[i] = a.dw[c0 * KK + i];
  }
  if (tid < C) {
    if (PREBN) bn_coeffs(a.inbn, c0 + tid, sMean[tid], sInv[tid]);
    sRed[tid] = 0.f;
    sRed[C + tid] = 0.f;
  }
  // only the input-BN staging reads the prologue's LDS (sMean / sInv) before the staging barrier
  if (PREBN) __syncthreads();
  KSTAMP(1);
  // staging with 16-byte loads (the band's rows are contiguous per channel; W, Wo % 4 == 0):
  // many wide loads in flight per wave, which the one-row-per-wave scalar loop lacked
  const float* ddn = a.dd + ((size_t)n * a.C + c0) * Ho * Wo;
  const size_t xn = ((size_t)n * a.C + c0) * H * W;
  const int va = max(oyA, 0), vb = min(oyB, Ho - 1), vrows = vb - va + 1;  // staged dd rows inside [0, Ho)
  {
    const int q4 = vrows * Wo / 4;  // float4s per channel
#pragma unroll 4
    for (int i = tid; i < C * q4; i += 256) {
      const int c = i / q4, o = (i - c * q4) * 4, r = o / Wo, ox = o - r * Wo;
      const float4 v = *reinterpret_cast<const float4*>(ddn + ((size_t)c * Ho + va) * Wo + o);
      float* d = sDD + (c * ODR + va - oyA + r) * ODW + PO + ox;
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
    // zero border: rows outside [0, Ho) and the PO columns on each side
    for (int i = tid; i < C * ODR; i += 256) {
      const int c = i / ODR, oy = oyA + i - c * ODR;
      float* d = sDD + i * ODW;
      if (oy < 0 || oy >= Ho) {
        for (int q = 0; q < ODW; ++q) d[q] = 0.f;
      } else {
        for (int q = 0; q < PO; ++q) d[q] = d[PO + Wo + q] = 0.f;
      }
    }
  }
  {
    const int q4 = NP / 4, w4 = W / 4;
#pragma unroll 4
    for (int i = tid; i < C * q4; i += 256) {
      const int c = i / q4, oq = i - c * q4, o = oq * 4, r = oq / w4, lo = (c * nrow + r) * PIN + (oq - r * w4) * 4;
      float4 v = xval4<PREBN>(a.x, xn + ((size_t)c * H + iy0) * W + o);
      if (PREBN) {
        const float m = sMean[c], iv = sInv[c];
        v.x = (v.x - m) * iv;
        v.y = (v.y - m) * iv;
        v.z = (v.z - m) * iv;
        v.w = (v.w - m) * iv;
      }
      v.x = fmaxf(v.x, 0.f);
      v.y = fmaxf(v.y, 0.f);
      v.z = fmaxf(v.z, 0.f);
      v.w = fmaxf(v.w, 0.f);
      *reinterpret_cast<float4*>(sIn + lo) = v;
    }
    if (accum) {
      const float* gsrc = a.gout + ((size_t)n * a.C + c0) * H * W;
#pragma unroll 4
      for (int i = tid; i < C * q4; i += 256) {
        const int c = i / q4, oq = i - c * q4, o = oq * 4, r = oq / w4;
        *reinterpret_cast<float4*>(sOld + (c * nrow + r) * PIN + (oq - r * w4) * 4) =
            *reinterpret_cast<const float4*>(gsrc + ((size_t)c * H + iy0) * W + o);
      }
    }
  }
  __syncthreads();
  KSTAMP(2);
  // input gradients of the band's own pixels
  float st1[C], st2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) st1[c] = st2[c] = 0.f;
  float* gn = a.gout + ((size_t)n * a.C + c0) * H * W;
  // The 4-pixel paths: stride 2 always, stride 1 through the tile map (widths of whole 2-quad cells);
  // other widths take the pixel-per-thread loop below
  const bool tiled = S == 1 && (W & 7) == 0;
  const bool vin = a.vin && (S == 2 || tiled);
  if (S == 1 && vin) {
    // stride 1: 4 consecutive input pixels of one row per thread (W % 4 == 0, as the staging
    // assumes): the taps' column offsets are shared, and the gradient leaves as one 16-byte store
    // per channel instead of four 4-byte ones
    // The staged dd row the 4 pixels meet through every column tap is dd columns ix .. ix + 3 + 2 PAD
    // (PO = PAD at stride 1): NQ aligned 16-byte quads from ix (ODW a multiple of 4), read as
    // ds_read_b128 per tap row instead of 4 K ds_read_b32 at a 4-float lane stride
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int NQ = (4 + 2 * PAD + 3) / 4;
    // work item = (channel, pixel quad), one per thread and pass, laid out by the tile map of
    // darts_plane_layout.h: every ds_read_b128 lane group holds 8 rows x 2 adjacent quads of one
    // channel, which tile_pitch makes conflict-free for the dd tap rows and the act(in) read alike
    // (in row-major quad order a lane group held half rows of 4 different rows, two of which
    // always overlapped: 2-3 LDS cycles per read instead of 1). Rows past a short band's end idle.
    const int npair = W >> 3, nrb = (nrow + kCellRows - 1) / kCellRows;
    for (int j = 4 * wave + tile_cell(lane); j < ((dbg & 1) ? 0 : C * nrb * npair); j += kBlockCells) {
      const TileItem it = tile_item(j, lane, nrb, npair);
      if (it.row >= nrow) continue;
      const int c = it.c, r = it.row, ix = 4 * it.quad, iy = iy0 + r;
      int srow[K];
#pragma unroll
      for (int k = 0; k < K; ++k) srow[k] = (iy + PAD - k * DIL - oyA) * ODW + ix;
      KEEP_WEIGHT_READS_LOCAL();
      const float* wk = sWt + c * KK;
      const float* dd = sDD + c * ODR * ODW;
      f4 ga = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        float v[4 * NQ];  // v[m] = dd column ix + m
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float4 t = *reinterpret_cast<const float4*>(dd + srow[ky] + 4 * q);
          v[4 * q] = t.x;
          v[4 * q + 1] = t.y;
          v[4 * q + 2] = t.z;
          v[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const float w = wk[ky * K + kx];
          const int o = 2 * PAD - kx * DIL;  // pixel ix + t meets dd column ix + t + o
          ga.x += w * v[o];
          ga.y += w * v[o + 1];
          ga.z += w * v[o + 2];
          ga.w += w * v[o + 3];
        }
      }
      const int li = (c * nrow + r) * PIN + ix;
      const f4 act = *reinterpret_cast<const f4*>(sIn + li);
      const f4 g = {act.x > 0.f ? ga.x : 0.f, act.y > 0.f ? ga.y : 0.f, act.z > 0.f ? ga.z : 0.f,
                    act.w > 0.f ? ga.w : 0.f};
      f4* dst = reinterpret_cast<f4*>(gn + ((size_t)c * H + iy) * W + ix);
      if (PREBN) {
        *dst = g;
        const float t1 = (g.x + g.y) + (g.z + g.w);
        const float t2 = (g.x * act.x + g.y * act.y) + (g.z * act.z + g.w * act.w);
#pragma unroll
        for (int cc = 0; cc < C; ++cc)  // select into the register arrays (no dynamic index)
          if (cc == c) {
            st1[cc] += t1;
            st2[cc] += t2;
          }
      } else {
        *dst = accum ? *reinterpret_cast<const f4*>(sOld + li) + g : g;
      }
    }
  }
  if constexpr (S == 2) {
    // stride 2: input pixel (iy, ix) meets tap (ky, kx) only when iy + PAD - ky*DIL and
    // ix + PAD - kx*DIL are both even. Threads walk the band class by class (row parity, column
    // parity; nrow, W even), so when a class spans whole waves (NPc % 64 == 0) the valid taps are
    // wave-uniform and the others are skipped by scalar branches instead of masked multiply-adds:
    // a quarter of the work (a dilated tap set is all-or-nothing per class).
    const int hw2 = W / 2, NPc = (nrow / 2) * hw2;
    for (int q = tid; q < ((dbg & 1) || !vin ? 0 : NP); q += 256) {
      const int cls = NPc % 64 == 0 ? __builtin_amdgcn_readfirstlane(q / NPc) : q / NPc;
      const int qq = q - cls * NPc, rr = qq / hw2, xx = qq - rr * hw2;
      const int r = 2 * rr + (cls >> 1), ix = 2 * xx + (cls & 1), iy = iy0 + r;
      const int iyc = iy0 + (cls >> 1), ixc = cls & 1;  // class representatives (parities only)
      int srow[K], scol[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        srow[k] = (((iy + PAD - k * DIL) >> 1) - oyA) * ODW;
        scol[k] = ((ix + PAD - k * DIL) >> 1) + PO;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        KEEP_WEIGHT_READS_LOCAL();
        const float* wk = sWt + c * KK;  // LDS broadcast reads
        const float* dd = sDD + c * ODR * ODW;
        float ga = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          if ((iyc + PAD - ky * DIL) & 1) continue;
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            if ((ixc + PAD - kx * DIL) & 1) continue;
            ga += wk[ky * K + kx] * dd[srow[ky] + scol[kx]];
          }
        }
        const int li = (c * nrow + r) * PIN + ix;
        const float act = sIn[li];
        const size_t gi = ((size_t)c * H + iy) * W + ix;
        const float g = act > 0.f ? ga : 0.f;
        if (PREBN) {
          gn[gi] = g;
          st1[c] += g;
          st2[c] += g * act;
        } else {
          gn[gi] = accum ? sOld[li] + g : g;
        }
      }
    }
  }
  for (int p = tid; p < ((dbg & 1) || vin ? 0 : NP); p += 256) {
    const int r = p / W, ix = p - r * W, iy = iy0 + r;
    int srow[K], scol[K];
    float mrow[K], mcol[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = iy + PAD - k * DIL, u = ix + PAD - k * DIL;
      srow[k] = ((t >> SH) - oyA) * ODW;
      scol[k] = (u >> SH) + PO;
      mrow[k] = (S == 1 || (t & 1) == 0) ? 1.f : 0.f;
      mcol[k] = (S == 1 || (u & 1) == 0) ? 1.f : 0.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      KEEP_WEIGHT_READS_LOCAL();
        const float* wk = sWt + c * KK;  // LDS broadcast reads
      const float* dd = sDD + c * ODR * ODW;
      float ga = 0.f;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        float rowacc = 0.f;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const float v = wk[ky * K + kx] * dd[srow[ky] + scol[kx]];
          rowacc += S == 1 ? v : mcol[kx] * v;
        }
        ga += S == 1 ? rowacc : mrow[ky] * rowacc;
      }
      const int li = (c * nrow + r) * PIN + ix;
      const float act = sIn[li];
      const size_t gi = ((size_t)c * H + iy) * W + ix;
      const float g = act > 0.f ? ga : 0.f;
      if (PREBN) {
        gn[gi] = g;
        st1[c] += g;
        st2[c] += g * act;  // g * y == g * relu(y)
      } else {
        gn[gi] = accum ? sOld[li] + g : g;
      }
    }
  }
  if (PREBN && a.red) {
    float st[2 * C];  // [sum g | sum g*y], reduce-scattered over the wave
#pragma unroll
    for (int c = 0; c < C; ++c) st[c] = st1[c], st[C + c] = st2[c];
    const float v = wave_reduce_scatter<2 * C>(st);
    if ((lane & (32 / C - 1)) == 0) atomicAdd(sRed + wave_scatter_index<2 * C>(lane), v);
  }
  KSTAMP(3);
  // depthwise weight gradients over the band: thread per (channel, tap, pixel part)
  if (a.gW && !(dbg & 2) && tiled) {
    // stride 1: job = (channel, ky, own row, column part). A 4-pixel quad of the input row (one
    // 16-byte LDS read) and the 4 + 2*PAD dd values it meets across all K column taps (registers)
    // feed 4*K multiply-adds: ~1.5 per LDS read against 0.5 for a pixel-by-pixel walk per tap.
    // Jobs are laid out in the cells of the tile map (wgrad_job: 8 rows x 2 interleaved column
    // parts per ds_read_b128 lane group), so both reads of every step are conflict-free - with one
    // lane per row the act(in) reads of 16 rows sat on 2 of the 16 bank slots (8-way) - and the
    // row is split further between cells until the jobs fill whole 16-cell passes. The K partial
    // sums are reduced across the lanes that share (channel, ky) before they touch sGW: one LDS
    // atomic per wave and weight when the wave's 4 cells share them, else one per cell (a
    // same-address ds_add_f32 per lane serialises 64-fold).
    constexpr int KP = K == 3 ? 4 : 8;  // K accumulators padded to a power of two (reduce-scatter)
    const int npair = W >> 3, nrb = (nrow + kCellRows - 1) / kCellRows;
    const int xp = wgrad_parts(C * K * nrb, npair), ncell = C * K * nrb * xp;
    const bool wave_job = ((nrb * xp) & 3) == 0;  // the 4 cells of a wave share (channel, ky)
    for (int u0 = 4 * wave; u0 < ncell; u0 += kBlockCells) {
      const int u = u0 + tile_cell(lane);
      const WgradJob jb = wgrad_job(u, lane, K, nrb, xp);
      float acc[KP];
#pragma unroll
      for (int kx = 0; kx < KP; ++kx) acc[kx] = 0.f;
      if (u < ncell && jb.row < nrow) {
        // dd columns ix .. ix + 3 + 2 PAD of the tap row (PO = PAD at stride 1), whole aligned quads
        const float* ddr = sDD + (jb.c * ODR + iy0 + jb.row + PAD - jb.ky * DIL - oyA) * ODW;
        const float* inr = sIn + (jb.c * nrow + jb.row) * PIN;
        for (int ix = 4 * jb.q0; ix < W; ix += 8 * xp) {
          const float4 v = *reinterpret_cast<const float4*>(inr + ix);
          constexpr int NQ = (4 + 2 * PAD + 3) / 4;
          float dseg[4 * NQ];  // dseg[m] = dd[ix - PAD + m]
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const float4 t = *reinterpret_cast<const float4*>(ddr + ix + 4 * q);
            dseg[4 * q] = t.x;
            dseg[4 * q + 1] = t.y;
            dseg[4 * q + 2] = t.z;
            dseg[4 * q + 3] = t.w;
          }
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            const int o = 2 * PAD - kx * DIL;  // in[ix + q] meets dd[ix + q + PAD - kx*DIL]
            acc[kx] += v.x * dseg[o] + v.y * dseg[o + 1] + v.z * dseg[o + 2] + v.w * dseg[o + 3];
          }
        }
      }
      float* gw = sGW + jb.c * KK + jb.ky * K;
      if (wave_job) {  // ncell is a multiple of 4 here: every cell of the wave is a job
        const float sum = wave_reduce_scatter<KP>(acc);
        const int kx = wave_scatter_index<KP>(lane);
        if ((lane & (64 / KP - 1)) == 0 && kx < K) atomicAdd(gw + kx, sum);
      } else {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          float v = acc[kx];  // the 16 lanes of a cell: lane bits 0, 1 and (2 with 3), (2 with 4)
          v += __shfl_xor(v, 1, 64);
          v += __shfl_xor(v, 2, 64);
          v += __shfl_xor(v, 12, 64);
          v += __shfl_xor(v, 20, 64);
          if ((lane & 27) == 0 && u < ncell) atomicAdd(gw + kx, v);
        }
      }
    }
  } else if (a.gW && !(dbg & 2)) {
    constexpr int JOBS = C * KK, T = JOBS >= 256 ? 1 : 256 / JOBS;
    for (int j = tid; j < JOBS * T; j += 256) {
      const int job = j / T, part = j - job * T;
      const int c = job / KK, tap = job - c * KK, ky = tap / K, kx = tap - ky * K;
      const float* dd = sDD + c * ODR * ODW;
      const float* in = sIn + c * nrow * PIN;
      float acc = 0.f;
      for (int r = 0; r < nrow; ++r) {
        const int t = iy0 + r + PAD - ky * DIL;
        if (S == 2 && (t & 1)) continue;
        const float* ddr = dd + ((t >> SH) - oyA) * ODW + PO;
        const float* inr = in + r * PIN;
        for (int ix = part * S + ((S == 2) ? ((PAD - kx * DIL) & 1) : 0); ix < W; ix += T * S)
          acc += inr[ix] * ddr[(ix + PAD - kx * DIL) >> SH];
      }
      atomicAdd(sGW + job, acc);
    }
  }
  KSTAMP(4);
  __syncthreads();
  if (PREBN && a.red && tid < 2 * C)  // red replica layout [sum g: a.C | sum g*y: a.C]
    atomicAdd(a.red + (bx % kRep) * 2 * a.C + (tid < C ? c0 + tid : a.C + c0 + tid - C), (double)sRed[tid]);
  if (a.gW)  // replica slot: the entry-local workgroup index (a mixed launch's grid is the entries' sum)
    for (int i = tid; i < C * KK; i += 256) atomicAdd(a.gW + (size_t)(bx % kRep) * a.gstride + c0 * KK + i, sGW[i]);
  KSTAMP(5);
}

template <int K, int DIL, int S, bool PREBN, int C>
__global__ void __launch_bounds__(256) dw_bwd_plane_kernel(DwBwdBatch bt, int nb, int dbg) {
  dw_bwd_plane_body<K, DIL, S, PREBN, C>(bt.e[blockIdx.y], blockIdx.x, nb, dbg);
}

// Mixed-variant depthwise backward: one launch for entries of different kernel size / dilation /
// stride / input BN that write DISTINCT outputs - a node's separable second stages (3x3 and 5x5,
// input BN), or a node's stage-1 separable and dilated convolutions each writing its own
// (masked) input-gradient buffer that the pool backward then sums into gx. Each entry carries
// its variant (dw_bwd_variant), band count and workgroup count.
#define DWB_CASE(KK, DD, SS, PB) \
  case dw_bwd_variant(KK, DD, SS, PB): dw_bwd_plane_body<KK, DD, SS, PB, C>(a, bx, a.nbands, 0); break;
template <int C>
__global__ void __launch_bounds__(256) dw_bwd_plane_multi_kernel(DwBwdBatch bt) {
  // 1-D grid of exactly the entries' workgroups: entry i owns [blk0, blk0 + nblk) (a
  // max-workgroups x entries grid started a workgroup, with its LDS, for every slot an entry
  // with fewer bands left empty)
  int ei = 0;
  for (int i = 1; i < bt.n; ++i)
    if ((int)blockIdx.x >= bt.e[i].blk0) ei = i;
  const DwBwdArgs a = bt.e[ei];  // copy: see dwpw_plane_multi_kernel
  const int bx = blockIdx.x - a.blk0;  // entry-local workgroup (band, group, replica slot)
  switch (a.variant) {
    DWB_CASE(3, 1, 1, true) DWB_CASE(5, 1, 1, true)
    DWB_CASE(3, 1, 1, false) DWB_CASE(3, 1, 2, false) DWB_CASE(5, 1, 1, false) DWB_CASE(5, 1, 2, false)
    DWB_CASE(3, 2, 1, false) DWB_CASE(3, 2, 2, false) DWB_CASE(5, 2, 1, false) DWB_CASE(5, 2, 2, false)
    default: break;
  }
}
#undef DWB_CASE

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
void launch_pool_bwd_multi(const PoolBwdBatch& b, hipStream_t st) {
  int maxblk = 0;
  size_t lds = 0;
  bool v4 = true;
  auto al = [](const void* p, uintptr_t m) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; };
  for (int i = 0; i < b.n; ++i) {
    const PoolBwdArgs& a = b.e[i];
    maxblk = std::max(maxblk, a.N * a.C);
    lds = std::max(lds, sizeof(float) * 2 * a.Ho * a.Wo + a.Ho * a.Wo + 16);
    v4 = v4 && (a.Ho * a.Wo) % 4 == 0 && (a.H * a.W) % 4 == 0 && a.W % 4 == 0 && al(a.za, 4 * sizeof(zt)) &&
         al(a.zm, 4 * sizeof(zt)) && al(a.amax, 4) && al(a.gx, 16);
    for (int e = 0; e < a.nsrc; ++e) {
      v4 = v4 && al(a.src[e].dout, 16);
      for (int j = 0; j < a.src[e].nextra; ++j) v4 = v4 && al(a.src[e].extra[j], 16);
    }
  }
  KSTAMP_ARM(kStampPoolBwd, st)
  if (v4) hipLaunchKernelGGL(pool_bwd_multi_kernel<true>, dim3(maxblk, b.n), dim3(256), lds, st, b);
  else hipLaunchKernelGGL(pool_bwd_multi_kernel<false>, dim3(maxblk, b.n), dim3(256), lds, st, b);
  KSTAMP_DISARM(st)
}

// LDS budget (KB) of one dw_bwd_plane band: the launchers cut an image into more bands until a
// band fits. With the stride-1 tile pitches a whole 32 x 32 plane of 4 channels takes 43 KB (3x3)
// to 47 KB (5x5, dilated): 40 cuts every such entry into two 16-row bands of 22-25 KB (6 resident
// workgroups per CU), 48 keeps them whole (3 per CU, no halo rows staged twice).
#ifndef KATIB_DWB_BAND_KB
#define KATIB_DWB_BAND_KB 48
#endif
constexpr int kDwbBandKB = KATIB_DWB_BAND_KB;
// LDS floats of one dw_bwd_plane band (nb bands per image)
static size_t dw_plane_floats(const DwBwdArgs& a, int K, int DIL, int S, int nb, bool accum, int C) {
  const int PAD = (K - 1) / 2 * DIL, PO = (PAD + S - 1) / S, sh = S == 2 ? 1 : 0, BRi = a.H / nb;
  auto fdiv = [sh](int v) { return v >= 0 ? v >> sh : -((-v + (1 << sh) - 1) >> sh); };
  const int ODR = fdiv(BRi - 1 + PAD) - fdiv(-PAD) + 2;  // +1: odd bands start at odd rows
  return (size_t)dwb_head_floats(C) + (size_t)C * ODR * plane_pitch(a.Wo + 2 * PO, S) +
         (size_t)C * BRi * plane_pitch(a.W, S) * (accum ? 2 : 1);
}

template <int K, int DIL, int S, int C>
static void launch_dw_bwd_plane_t(const DwBwdBatch& b, bool prebn, hipStream_t st) {
  const DwBwdArgs& a = b.e[0];
  bool accum = false;
  for (int i = 0; i < b.n; ++i) accum |= !prebn && !b.e[i].overwrite;
  // bands: as few as possible (less halo) while the launch still has ~4 workgroups per CU and a
  // band stays within kDwbBandKB of LDS
  int nb = 1;
  const int G = a.C / C;  // channel groups per image
  while (nb < 8 && a.H % (2 * nb) == 0 &&
         (dw_plane_floats(a, K, DIL, S, nb, accum, C) * 4 > kDwbBandKB * 1024 || a.N * nb * G * b.n < 1024))
    nb *= 2;
  const size_t lds = sizeof(float) * dw_plane_floats(a, K, DIL, S, nb, accum, C);
  dim3 grid(a.N * nb * G, b.n);
  constexpr int dbg = 0;  // timing probes
  if (prebn) hipLaunchKernelGGL((dw_bwd_plane_kernel<K, DIL, S, true, C>), grid, dim3(256), lds, st, b, nb, dbg);
  else hipLaunchKernelGGL((dw_bwd_plane_kernel<K, DIL, S, false, C>), grid, dim3(256), lds, st, b, nb, dbg);
}

static bool aligned16(const DwBwdBatch& b) {
  for (int i = 0; i < b.n; ++i)
    if (((uintptr_t)b.e[i].x | (uintptr_t)b.e[i].dd | (uintptr_t)b.e[i].gout) & 15) return false;
  return true;
}

// plane path: narrow layers whose spatial sizes divide exactly by the stride
static bool dw_plane_ok(const DwBwdBatch& b, int K, int DIL, int S) {
  const DwBwdArgs& a = b.e[0];
  return (a.C == 4 || a.C == 8 || (a.C % 16 == 0 && a.C <= kMaxC)) && a.H == a.Ho * S && a.W == a.Wo * S &&
         a.pad == (K - 1) / 2 * DIL && a.Wo % 4 == 0 && aligned16(b);
}

template <int K, int DIL, int S>
static void launch_dw_bwd_t(const DwBwdBatch& b, bool prebn, hipStream_t st) {
  const DwBwdArgs& a = b.e[0];
  if (dw_plane_ok(b, K, DIL, S)) {
    // wide layers run in channel groups of grp (4, 8 or 16) channels: 8 measured
    // 48.2 vs 50.8 ms per darts-gpu.yaml step against 16 (half the LDS per band: fewer, taller bands),
    // and 4 beats 8 on the round-4 kernels (B5 6.37 vs 6.44 ms, default 41.98 vs 42.20 ms,
    // profiles/darts_dwb_group_ab_r04.log)
    constexpr int grp = 4;
    if (a.C == 4 || grp == 4) return launch_dw_bwd_plane_t<K, DIL, S, 4>(b, prebn, st);
    if (a.C == 8 || grp == 8) return launch_dw_bwd_plane_t<K, DIL, S, 8>(b, prebn, st);
    return launch_dw_bwd_plane_t<K, DIL, S, 16>(b, prebn, st);
  }
  const int TR = 64 / a.Wo;
  const int r = (K - 1) / 2 * DIL, h = (r + S - 1) / S, OR = TR + 2 * h;
  const int IR = (TR - 1) * S + (K - 1) * DIL + 1;
  const int IW = (a.Wo - 1) * S + (K - 1) * DIL + 1;
  size_t lds = sizeof(float) * (a.chunk * OR * a.Wo + a.chunk * IR * IW + 4 * a.C + (a.gW ? a.C * K * K : 0));
  dim3 grid(per_edge_blocks(a.N * (a.Ho / TR), b.n), b.n);
  if (prebn) hipLaunchKernelGGL((dw_bwd_kernel<K, DIL, S, true>), grid, dim3(256), lds, st, b);
  else hipLaunchKernelGGL((dw_bwd_kernel<K, DIL, S, false>), grid, dim3(256), lds, st, b);
}

bool launch_dw_bwd_multi(DwBwdBatch b, hipStream_t st) {
  if (b.n < 1) return true;
  const DwBwdArgs& a0 = b.e[0];
  if (!(a0.C == 4 || a0.C == 8 || (a0.C % 16 == 0 && a0.C <= kMaxC)) || !aligned16(b)) return false;
  constexpr int grp = 4;
  const int C = (a0.C == 4 || grp == 4) ? 4 : 8;  // channel groups as launch_dw_bwd_t
  if (a0.C % C) return false;
  int total = 0;
  size_t lds = 0;
  for (int i = 0; i < b.n; ++i) {
    DwBwdArgs& a = b.e[i];
    const int K = dw_variant_k(a.variant), DIL = dw_variant_dil(a.variant), S = dw_variant_s(a.variant);
    const bool prebn = dw_variant_prebn(a.variant);
    // the plane kernel's layout (dw_plane_ok) and an overwriting (never accumulating) input BN-free entry
    if (a.C != a0.C || a.H != a.Ho * S || a.W != a.Wo * S || a.pad != (K - 1) / 2 * DIL || a.Wo % 4 ||
        (prebn && (DIL != 1 || S != 1)) || (!prebn && !a.overwrite))
      return false;
    int nb = 1;
    const int G = a.C / C;
    constexpr int min_wg = 512;
    while (nb < 8 && a.H % (2 * nb) == 0 &&
           (dw_plane_floats(a, K, DIL, S, nb, false, C) * 4 > kDwbBandKB * 1024 || a.N * nb * G * b.n < min_wg))
      nb *= 2;
    a.nbands = nb;
    a.nblk = a.N * nb * G;
    a.vin = S == 1 ? (vec_mask() >> (C == 4 ? 2 : 3)) & 1 : (vec_mask() >> 4) & 1;
    a.blk0 = total;  // the entries' workgroups back to back in a 1-D grid
    total += a.nblk;
    lds = std::max(lds, sizeof(float) * dw_plane_floats(a, K, DIL, S, nb, false, C));
  }
  KSTAMP_ARM(kStampDwBwd, st)
  if (C == 4) hipLaunchKernelGGL(dw_bwd_plane_multi_kernel<4>, dim3(total), dim3(256), lds, st, b);
  else hipLaunchKernelGGL(dw_bwd_plane_multi_kernel<8>, dim3(total), dim3(256), lds, st, b);
  KSTAMP_DISARM(st)
  return true;
}

void launch_dw_bwd(const DwBwdBatch& b, int K, int dil, int S, bool prebn, hipStream_t st) {
#define DISPATCH(KK, DD, SS) \
  if (K == KK && dil == DD && S == SS) return launch_dw_bwd_t<KK, DD, SS>(b, prebn, st);
  DISPATCH(3, 1, 1) DISPATCH(3, 1, 2) DISPATCH(5, 1, 1) DISPATCH(5, 1, 2)
  DISPATCH(3, 2, 1) DISPATCH(3, 2, 2) DISPATCH(5, 2, 1) DISPATCH(5, 2, 2)
#undef DISPATCH
}

}  // namespace katib_hip
