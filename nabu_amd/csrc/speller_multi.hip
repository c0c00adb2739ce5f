// speller_multi.hip — the Speller decoder over M encoded inputs, one attention mechanism each (AttentionWrapper with a
// list of mechanisms; include/nabu_hip.h, nabu_speller_multi_*).
//
// The decoder steps are a launch-bound chain (LABNOTES.md 6.5), so M mechanisms must not become M times the attention
// launches: a step's M mechanisms are ONE launch per pass, grid (B, S, M).  blockIdx.z selects the mechanism; the
// workgroup reads its memory's Te, E, slice count and pointers from a table that travels as the kernel argument, and
// carves its LDS by its OWN Te (the launch requests the largest).  What a pass needs from all frame slices of an
// utterance (softmax normaliser, dq, the gradient to the previous alignment, d conv kernel) is done by the slice that
// arrives last, inside the launch.  The contexts of all mechanisms live in one [B, sum E] buffer (row stride sum E,
// mechanism m at its column offset): it is the operand of the next step's layer-0 product and of the projection as it
// stands; the M queries are one product against the column-concatenated [U, M U] query kernels and the kernels read
// q_m at column m U of that [B, M U] result.  Arithmetic per mechanism is that of attn_fwd_kernel / attn_bwd_kernel
// (speller.hip, the general forms), which stay as they are for the one-memory decoder.
#include "common.h"
#include "gemm_args.h"
#include "speller_multi.h"
#include "speller_attn_dev.h"

namespace nabu {

namespace {

constexpr int MM = NABU_SPELLER_MAX_MEMORIES;

// ---------------------------------------------------------------------------
// forward: grid (B, Smax, M).  LDS (floats): conv kernel [ck_floats] | alp[Te] | sc[Te] | cf[Te F] | red[64] | part[4 AT]
template <bool KIND>
__global__ __launch_bounds__(AT) void attn_multi_fwd_kernel(MArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MMem &mm = p.m[blockIdx.z];
  const int b = blockIdx.x, sl = blockIdx.y, S = mm.S;
  if (sl >= S) return;                       // this mechanism has fewer slices than the launch's largest
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int Te = mm.Te, U = p.U, E = mm.E, F = p.F;
  constexpr int NW = AT / 64;
  float *base = smem + ck_floats(p.kind, p.K, F);
  float *alp = base, *sc = alp + Te, *cf = sc + Te, *red = cf + (KIND ? Te * F : 0);
  float *align = mm.align + (size_t)b * Te;
  const float *align_prev = mm.align_prev + (size_t)b * Te;
  float *cx = p.ctx + (size_t)b * p.SE + mm.coff;              // my columns of the shared context rows
  float *ctx = S > 1 ? mm.part + ((size_t)b * S + sl) * (E + 4) : cx;
  const bool fused = S > 1;
  __shared__ int last_flag;
  if (p.step >= p.dec_len[b]) {              // finished row: state frozen (by slice 0)
    if (sl != 0) return;
    const float *cp = p.ctx_prev + (size_t)b * p.SE + mm.coff;
    for (int t = tid; t < Te; t += AT) align[t] = align_prev[t];
    for (int e = tid; e < E; e += AT) cx[e] = cp[e];
    return;
  }
  const int nfull = min(max(mm.enc_len[b], 0), Te);
  const int per = (Te + S - 1) / S, lo = min(sl * per, nfull), n = min(lo + per, nfull);   // my frames [lo, n)
  const float *keys = mm.keys + (size_t)b * Te * U;
  const float *vals = mm.values + (size_t)b * Te * E;
  const float *q = p.q + (size_t)b * p.MU + (size_t)blockIdx.z * U;
  if (KIND) {
    for (int t = tid; t < Te; t += AT) alp[t] = align_prev[t];
    for (int i = tid; i < p.K * F; i += AT) smem[i] = mm.ck[i];
    __syncthreads();
    conv_features(p.K, F, Te, alp, cf, lo, n, smem);
    __syncthreads();
  }
  // windowed: only frames in [m - left - 1, m + right), m = first frame at which the cumulated previous alignment > 0.5
  int w_lo = 0, w_hi = Te;
  if (!KIND && p.kind == 2) {
    if (w == 0) {
      float carry = 0.f;
      int m = Te;
      for (int t0 = 0; t0 < Te && m == Te; t0 += 64) {
        const int t = t0 + lane;
        float c = t < Te ? align_prev[t] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float up = __shfl_up(c, o);
          if (lane >= o) c += up;
        }
        c += carry;
        const unsigned long long hit = __ballot(t < Te && c > 0.5f);
        if (hit) m = t0 + __ffsll((long long)hit) - 1;
        carry = __shfl(c, 63);
      }
      if (lane == 0) red[0] = __int_as_float(m);
    }
    __syncthreads();
    const int m = __float_as_int(red[0]);
    w_lo = max(m - p.K - 1, 0);
    w_hi = min(m + F, Te);
    __syncthreads();
  }
  // scores: waves over frames (4 in flight), lanes over 16-byte groups of units
  {
    const int U4 = U / 4;
    constexpr int FR = 4;
    const float4 *keys4 = reinterpret_cast<const float4 *>(keys);
    const float4 *q4 = reinterpret_cast<const float4 *>(q), *v4 = reinterpret_cast<const float4 *>(mm.v);
    for (int t0 = lo + w; t0 < n; t0 += FR * NW) {
      float s[FR];
#pragma unroll
      for (int i = 0; i < FR; ++i) s[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {            // U <= 1024
        const int u4 = lane + 64 * j;
        if (u4 >= U4) continue;
        const float4 qq = q4[u4], vv = v4[u4];
        float4 kx[FR];
#pragma unroll
        for (int i = 0; i < FR; ++i) kx[i] = keys4[(size_t)min(t0 + i * NW, n - 1) * U4 + u4];
#pragma unroll
        for (int i = 0; i < FR; ++i) {
          const int t = t0 + i * NW;
          float4 x = make_float4(kx[i].x + qq.x, kx[i].y + qq.y, kx[i].z + qq.z, kx[i].w + qq.w);
          if (KIND && t < n)
            for (int f = 0; f < F; ++f) {
              const float c = cf[t * F + f];
              const float4 wf = *reinterpret_cast<const float4 *>(mm.wf + (size_t)f * U + 4 * u4);
              x.x = fmaf(c, wf.x, x.x); x.y = fmaf(c, wf.y, x.y); x.z = fmaf(c, wf.z, x.z); x.w = fmaf(c, wf.w, x.w);
            }
          s[i] = fmaf(vv.x, tanhf_(x.x), s[i]);
          s[i] = fmaf(vv.y, tanhf_(x.y), s[i]);
          s[i] = fmaf(vv.z, tanhf_(x.z), s[i]);
          s[i] = fmaf(vv.w, tanhf_(x.w), s[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < FR; ++i) {
        const float tot = wave_sum(s[i]);
        if (lane == 0 && t0 + i * NW < n) sc[t0 + i * NW] = tot;
      }
    }
  }
  __syncthreads();
  if (!KIND && p.kind == 2) {
    for (int t = lo + tid; t < n; t += AT)
      if (t < w_lo || t >= w_hi) sc[t] = -INFINITY;
    __syncthreads();
  }
  // e[t] = exp(score - max) (softmax) or sigmoid(score); a slice keeps its local max and sum, the whole utterance normalises
  float mx = -3.0e38f;
  if (p.prob_fn == 0) {
    for (int t = lo + tid; t < n; t += AT) mx = fmaxf(mx, sc[t]);
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = red[0];
    for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red[i]);
    __syncthreads();
  }
  float z = 0.f;
  for (int t = lo + tid; t < n; t += AT) {
    const float e = p.prob_fn == 0 ? expf(sc[t] - mx) : 1.0f / (1.0f + expf(-sc[t]));
    sc[t] = e;
    if (fused) xst(align + t, e);
    z += e;
  }
  z = wave_sum(z);
  if (lane == 0) red[w] = z;
  __syncthreads();
  z = 0.f;
  for (int i = 0; i < NW; ++i) z += red[i];
  __syncthreads();
  if (fused) {
    if (tid == 0) { xst(ctx + E, mx); xst(ctx + E + 1, z); }
  } else {
    const float inv = p.prob_fn == 1 ? 1.0f : (z > 0.f ? 1.0f / z : 0.f);       // enc_len 0: alignment and context 0
    if (p.prob_fn == 2 && tid == 0 && mm.znorm) mm.znorm[b] = z;
    for (int t = tid; t < Te; t += AT) {
      const float a = t < n ? sc[t] * inv : 0.f;
      sc[t] = a;
      align[t] = a;
    }
    __syncthreads();
  }
  // context = weights^T . values over my frames: threads over 16-byte column groups, frames split over thread groups
  {
    const int E4 = E / 4;
    const int nsp = max(1, min(AT / max(E4, 1), 8));
    const float4 *vals4 = reinterpret_cast<const float4 *>(vals);
    float4 *part = reinterpret_cast<float4 *>(base + ((2 * Te + (KIND ? Te * F : 0) + 64 + 3) & ~3));
    for (int c0 = 0; c0 < E4; c0 += AT / nsp) {
      const int e4 = c0 + tid % (AT / nsp), pt = tid / (AT / nsp);
      if (e4 < E4 && pt < nsp) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = lo + pt; t < n; t += nsp) {
          const float4 a0 = vals4[(size_t)t * E4 + e4];
          const float w0 = sc[t];
          c.x = fmaf(w0, a0.x, c.x); c.y = fmaf(w0, a0.y, c.y); c.z = fmaf(w0, a0.z, c.z); c.w = fmaf(w0, a0.w, c.w);
        }
        part[pt * (AT / nsp) + (e4 - c0)] = c;
      }
      __syncthreads();
      if (tid < AT / nsp && c0 + tid < E4) {
        float4 c = part[tid];
        for (int i = 1; i < nsp; ++i) {
          const float4 o = part[i * (AT / nsp) + tid];
          c.x += o.x; c.y += o.y; c.z += o.z; c.w += o.w;
        }
        float *o = ctx + 4 * (c0 + tid);
        if (fused) { xst(o, c.x); xst(o + 1, c.y); xst(o + 2, c.z); xst(o + 3, c.w); }
        else       { o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w; }
      }
      __syncthreads();
    }
  }
  if (!fused) return;
  // ---- the slice that arrives last combines the utterance's slices (flash-style rescaling)
  if (!last_arriver(mm.tickets + b, (unsigned)S, &last_flag)) return;
  {
    float *fac = red;
    const float *pr = mm.part + (size_t)b * S * (E + 4);
    if (tid == 0) {
      float Mx = -3.0e38f, Z = 0.f;
      for (int i = 0; i < S; ++i) Mx = fmaxf(Mx, xld(pr + (size_t)i * (E + 4) + E));
      for (int i = 0; i < S; ++i) {
        const float f = p.prob_fn == 0 ? expf(xld(pr + (size_t)i * (E + 4) + E) - Mx) : 1.0f;
        fac[i] = f;
        Z += f * xld(pr + (size_t)i * (E + 4) + E + 1);
      }
      const float inv = p.prob_fn == 1 ? 1.0f : (Z > 0.f ? 1.0f / Z : 0.f);     // enc_len 0: alignment and context 0
      for (int i = 0; i < S; ++i) fac[i] *= inv;
      if (p.prob_fn == 2 && mm.znorm) mm.znorm[b] = Z;
    }
    __syncthreads();
    for (int t = tid; t < Te; t += AT) align[t] = t < nfull ? xld(align + t) * fac[t / per] : 0.f;
    for (int e = tid; e < E; e += AT) {
      float c = 0.f;
      for (int i = 0; i < S; ++i) c = fmaf(fac[i], xld(pr + (size_t)i * (E + 4) + e), c);
      cx[e] = c;
    }
  }
}

// ---------------------------------------------------------------------------
// backward: grid (B, Smax, M).  Workgroup (b, s, m) owns the frames [lo, hi) of utterance b in memory m: it
// ACCUMULATES into its rows of dkeys and into its partial rows dv_part [B S, U], dwf_part [B S, F, U]; the slice that
// arrives last sums dq and, for location-aware attention, turns the slices' d location features into the gradient to
// the previous alignment and adds its utterance's row of dck_part [B, K F].
// LDS (floats): conv kernel | alp[Te] | ds[Te] | cf[Te F] | red[NW U]
template <bool KIND>
__global__ __launch_bounds__(AT) void attn_multi_bwd_kernel(MArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MMem &mm = p.m[blockIdx.z];
  const int b = blockIdx.x, sl = blockIdx.y, S = mm.S;
  if (sl >= S) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int Te = mm.Te, U = p.U, E = mm.E, F = p.F;
  constexpr int NW = AT / 64;
  float *base = smem + ck_floats(p.kind, p.K, F);
  float *alp = base, *ds = alp + Te, *cf = ds + Te;
  float *red = base + ((2 * Te + (KIND ? Te * F : 0) + 3) & ~3);
  float *dq_part = mm.part + ((size_t)b * S + sl) * U;
  float *dq = p.dq + (size_t)b * p.MU + (size_t)blockIdx.z * U;
  float *dal_out = mm.dalign_out ? mm.dalign_out + (size_t)b * Te : nullptr;
  const float *dal_in = mm.dalign_in ? mm.dalign_in + (size_t)b * Te : nullptr;
  __shared__ int last_flag;
  if (p.step >= p.dec_len[b]) {              // finished row: no gradient of its own, d alignment passes through
    if (sl == 0) {
      for (int u = tid; u < U; u += AT) dq[u] = 0.f;
      if (dal_out)
        for (int t = tid; t < Te; t += AT) dal_out[t] = dal_in ? dal_in[t] : 0.f;
    }
    return;
  }
  const int n = min(max(mm.enc_len[b], 0), Te);
  const int per = (Te + S - 1) / S, lo = min(sl * per, n), hi = min(lo + per, n);
  float *dcf = mm.dcf_g + (size_t)b * Te * F;
  const float *keys = mm.keys + (size_t)b * Te * U;
  const float *vals = mm.values + (size_t)b * Te * E;
  const float *q = p.q + (size_t)b * p.MU + (size_t)blockIdx.z * U;
  const float *al = mm.align_c + (size_t)b * Te;
  const float *dctx = p.dctx + (size_t)b * p.SE + mm.coff;
  const float *cx = p.ctx + (size_t)b * p.SE + mm.coff;
  float *dkeys = mm.dkeys + (size_t)b * Te * U;
  if (KIND) {
    for (int t = tid; t < Te; t += AT) alp[t] = mm.align_prev[(size_t)b * Te + t];
    for (int i = tid; i < p.K * F; i += AT) smem[i] = mm.ck[i];
    __syncthreads();
    conv_features(p.K, F, Te, alp, cf, lo, hi, smem);
  }
  // d alignment[t] = dctx . values[t] (+ what arrives through the next step's location features)
  {
    const int E4 = E / 4;
    constexpr int FR = 4;
    const float4 *vals4 = reinterpret_cast<const float4 *>(vals);
    const float4 *dctx4 = reinterpret_cast<const float4 *>(dctx);
    for (int t0 = lo + w; t0 < hi; t0 += FR * NW) {
      float s[FR];
#pragma unroll
      for (int i = 0; i < FR; ++i) s[i] = 0.f;
      for (int e4 = lane; e4 < E4; e4 += 64) {
        const float4 dc = dctx4[e4];
        float4 vv[FR];
#pragma unroll
        for (int i = 0; i < FR; ++i) vv[i] = vals4[(size_t)min(t0 + i * NW, hi - 1) * E4 + e4];
#pragma unroll
        for (int i = 0; i < FR; ++i) {
          s[i] = fmaf(dc.x, vv[i].x, s[i]); s[i] = fmaf(dc.y, vv[i].y, s[i]);
          s[i] = fmaf(dc.z, vv[i].z, s[i]); s[i] = fmaf(dc.w, vv[i].w, s[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < FR; ++i) {
        const int t = t0 + i * NW;
        const float tot = wave_sum(s[i]);
        if (lane == 0 && t < hi) ds[t] = tot + (dal_in ? dal_in[t] : 0.f);
      }
    }
  }
  __syncthreads();
  // sum_t a[t] da[t] over ALL frames without visiting them: dctx . context + sum_t a[t] dalign_in[t]
  float r = 0.f;
  for (int e = tid; e < E; e += AT) r = fmaf(dctx[e], cx[e], r);
  if (dal_in)
    for (int t = tid; t < n; t += AT) r = fmaf(al[t], dal_in[t], r);
  r = wave_sum(r);
  if (lane == 0) red[w] = r;
  __syncthreads();
  r = 0.f;
  for (int i = 0; i < NW; ++i) r += red[i];
  __syncthreads();
  if (p.prob_fn == 0) {
    for (int t = lo + tid; t < hi; t += AT) ds[t] = al[t] * (ds[t] - r);
  } else if (p.prob_fn == 1) {
    for (int t = lo + tid; t < hi; t += AT) ds[t] = ds[t] * al[t] * (1.f - al[t]);
  } else {
    const float z = mm.znorm[b];
    for (int t = lo + tid; t < hi; t += AT) ds[t] = (ds[t] - r) * al[t] * (1.f - al[t] * z);
  }
  __syncthreads();
  // through v . tanh(keys + q + f): lanes own 16-byte groups of units, waves split the frames
  constexpr int MAXJ = 4, NF = 16;           // U <= 1024, F <= 16
  constexpr int FR = KIND ? 1 : 2;
  const int U4 = U / 4;
  float4 dq_l[MAXJ], dv_l[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) dq_l[j] = dv_l[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  {
    const float4 *keys4 = reinterpret_cast<const float4 *>(keys);
    float4 *dkeys4 = reinterpret_cast<float4 *>(dkeys);
    const float4 *q4 = reinterpret_cast<const float4 *>(q), *v4 = reinterpret_cast<const float4 *>(mm.v);
    for (int t0 = lo + w; t0 < hi; t0 += FR * NW) {
      float dcf_l[FR][KIND ? NF : 1];
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int f = 0; f < (KIND ? NF : 1); ++f) dcf_l[i][f] = 0.f;
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) {
        const int u4 = lane + 64 * j;
        if (u4 < U4) {
          const float4 qq = q4[u4], vv = v4[u4];
          float4 kx[FR], dk[FR];
#pragma unroll
          for (int i = 0; i < FR; ++i) {
            const size_t o = (size_t)min(t0 + i * NW, hi - 1) * U4 + u4;
            kx[i] = keys4[o];
            dk[i] = dkeys4[o];
          }
#pragma unroll
          for (int i = 0; i < FR; ++i) {
            const int t = t0 + i * NW;
            if (t < hi) {
              const float g = ds[t];
              float x[4] = {kx[i].x + qq.x, kx[i].y + qq.y, kx[i].z + qq.z, kx[i].w + qq.w};
              if (KIND)
                for (int f = 0; f < F; ++f) {
                  const float c = cf[t * F + f];
                  const float4 wf = *reinterpret_cast<const float4 *>(mm.wf + (size_t)f * U + 4 * u4);
                  x[0] = fmaf(c, wf.x, x[0]); x[1] = fmaf(c, wf.y, x[1]); x[2] = fmaf(c, wf.z, x[2]); x[3] = fmaf(c, wf.w, x[3]);
                }
              const float vvv[4] = {vv.x, vv.y, vv.z, vv.w};
              float d[4], th[4];
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                th[c] = tanhf_(x[c]);
                d[c] = g * vvv[c] * (1.f - th[c] * th[c]);
              }
              dq_l[j].x += d[0]; dq_l[j].y += d[1]; dq_l[j].z += d[2]; dq_l[j].w += d[3];
              dv_l[j].x = fmaf(g, th[0], dv_l[j].x); dv_l[j].y = fmaf(g, th[1], dv_l[j].y);
              dv_l[j].z = fmaf(g, th[2], dv_l[j].z); dv_l[j].w = fmaf(g, th[3], dv_l[j].w);
              dkeys4[(size_t)t * U4 + u4] = make_float4(dk[i].x + d[0], dk[i].y + d[1], dk[i].z + d[2], dk[i].w + d[3]);
              if (KIND) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                  if (f < F) {
                    const float4 wf = *reinterpret_cast<const float4 *>(mm.wf + (size_t)f * U + 4 * u4);
                    dcf_l[i][KIND ? f : 0] = fmaf(d[0], wf.x, fmaf(d[1], wf.y, fmaf(d[2], wf.z, fmaf(d[3], wf.w, dcf_l[i][KIND ? f : 0]))));
                  }
              }
            }
          }
        }
      }
      if (KIND) {
#pragma unroll
        for (int i = 0; i < FR; ++i)
#pragma unroll
          for (int f = 0; f < NF; ++f)
            if (f < F) {
              const float tot = wave_sum(dcf_l[i][KIND ? f : 0]);
              if (lane == 0 && t0 + i * NW < hi) xst(dcf + (t0 + i * NW) * F + f, tot);
            }
      }
    }
  }
  // cross-wave sums of dq and dv (fixed order)
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int u4 = lane + 64 * j;
    if (u4 < U4) *reinterpret_cast<float4 *>(red + (size_t)w * U + 4 * u4) = dq_l[j];
  }
  __syncthreads();
  for (int u = tid; u < U; u += AT) {
    float s = 0.f;
    for (int i = 0; i < NW; ++i) s += red[i * U + u];
    xst(dq_part + u, s);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int u4 = lane + 64 * j;
    if (u4 < U4) *reinterpret_cast<float4 *>(red + (size_t)w * U + 4 * u4) = dv_l[j];
  }
  __syncthreads();
  for (int u = tid; u < U; u += AT) {
    float s = 0.f;
    for (int i = 0; i < NW; ++i) s += red[i * U + u];
    mm.dv_part[((size_t)b * S + sl) * U + u] += s;
  }
  if (KIND) {
    // d conv_proj[f,u] += sum_t cf[t,f] d[t,u], d recomputed in a second pass over my frames
    for (int u = tid; u < U; u += AT) {
      float acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = 0.f;
      for (int t = lo; t < hi; ++t) {
        float x = keys[(size_t)t * U + u] + q[u];
        for (int f = 0; f < F; ++f) x = fmaf(cf[t * F + f], mm.wf[f * U + u], x);
        const float th = tanhf_(x);
        const float d = ds[t] * mm.v[u] * (1.f - th * th);
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (f < F) acc[f] = fmaf(cf[t * F + f], d, acc[f]);
      }
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < F) mm.dwf_part[(((size_t)b * S + sl) * F + f) * U + u] += acc[f];
    }
  }
  // ---- what needs every frame of the utterance: by the slice that arrives last
  if (!last_arriver(mm.tickets + b, (unsigned)S, &last_flag)) return;
  for (int u = tid; u < U; u += AT) {
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += xld(mm.part + ((size_t)b * S + i) * U + u);
    dq[u] = s;
  }
  if (!KIND) return;
  // d location features of all slices -> LDS (frames past the length carry no gradient); alp and the conv kernel are there
  float *dcs = cf;
  for (int i = tid; i < Te * F; i += AT) dcs[i] = i < n * F ? xld(dcf + i) : 0.f;
  __syncthreads();
  const int pb = (p.K - 1) / 2;
  // d previous alignment: out frame t receives dcf[t - d + pb, f] ck[d, f]; 16 threads per out frame
  for (int t0 = 0; t0 < Te; t0 += AT / 16) {
    const int t = t0 + (tid >> 4), qd = tid & 15;
    float s0 = 0.f;
    if (t < Te) {
      const int d0 = max(0, t + pb - (n - 1)), d1 = min(p.K, t + pb + 1);
      for (int d = d0 + qd; d < d1; d += 16) {
        const float *g = dcs + (t - d + pb) * F, *c = smem + d * F;
        for (int f = 0; f < F; ++f) s0 = fmaf(g[f], c[f], s0);
      }
    }
    s0 += __shfl_xor(s0, 1);
    s0 += __shfl_xor(s0, 2);
    s0 += __shfl_xor(s0, 4);
    s0 += __shfl_xor(s0, 8);
    if (t < Te && qd == 0) dal_out[t] = s0;
  }
  // d conv kernel[d,f] += sum_to a_prev[to + d - pb] dcf[to, f]
  for (int i = tid; i < p.K * F; i += AT) {
    const int d = i / F, f = i % F;
    float s0 = 0.f, s1 = 0.f;
    const int to0 = max(0, pb - d), to1 = min(n, Te + pb - d);
    const float *a = alp + d - pb, *g = dcs + f;
    int to = to0;
    for (; to + 1 < to1; to += 2) {
      s0 = fmaf(a[to], g[to * F], s0);
      s1 = fmaf(a[to + 1], g[(to + 1) * F], s1);
    }
    for (; to < to1; ++to) s0 = fmaf(a[to], g[to * F], s0);
    mm.dck_part[(size_t)b * p.K * F + i] += s0 + s1;
  }
}

// dst[r, c0 + c] = src[r, c] (column-concatenation of the query kernels)
__global__ __launch_bounds__(256) void put_cols_kernel(int R, int Cn, const float *__restrict__ src, float *__restrict__ dst,
                                                      int ldd, int c0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * Cn) return;
  dst[(size_t)(i / Cn) * ldd + c0 + i % Cn] = src[i];
}

// ---------------------------------------------------------------------------

static nabu_attn_desc mem_desc(const nabu_speller_multi_desc *d, int m) {
  nabu_attn_desc a = {sizeof(nabu_attn_desc), d->B, d->Te[m], d->E[m], d->U, d->kind, d->K, d->F, d->prob_fn};
  return a;
}

}  // namespace

int multi_attn_geo(const nabu_speller_multi_desc *d, MultiAttnGeo *g) {
  if (!d || d->size != sizeof(nabu_speller_multi_desc)) return fail(NABU_EINVAL, "speller_multi: bad descriptor size");
  if (d->M < 1 || d->M > MM) return fail(NABU_EUNSUP, "speller_multi: 1..%d encoded inputs", MM);
  if (d->B <= 0 || d->U <= 0 || d->C <= 1 || d->L <= 0) return fail(NABU_EINVAL, "speller_multi: bad dimensions");
  if (d->num_layers < 1 || d->num_layers > NABU_SPELLER_MAX_LAYERS)
    return fail(NABU_EUNSUP, "speller_multi: 1..%d layers", NABU_SPELLER_MAX_LAYERS);
  if (!(d->keep_prob > 0.f && d->keep_prob <= 1.f)) return fail(NABU_EINVAL, "speller_multi: keep_prob out of (0,1]");
  if (!(d->sample_prob >= 0.f && d->sample_prob <= 1.f)) return fail(NABU_EINVAL, "speller_multi: sample_prob out of [0,1]");
  g->M = d->M; g->SE = 0; g->MU = d->M * d->U; g->Smax = 1; g->lds_f = g->lds_b = 0;
  for (int m = 0; m < d->M; ++m) {
    const nabu_attn_desc a = mem_desc(d, m);
    const int S = nabu_attn_bwd_slices(&a);        // 0: the attention checks refused (dimensions, multiples of 4, LDS)
    if (S <= 0) return NABU_EUNSUP;                // (the message is theirs)
    g->S[m] = S;
    if (S > g->Smax) g->Smax = S;
    g->coff[m] = g->SE;
    g->SE += d->E[m];
    const size_t Te = d->Te[m], F = d->kind == 1 ? d->F : 0, ckf = ck_floats(d->kind, d->K, d->F);
    const size_t f = ckf + 2 * Te + Te * F + 64 + 4 + 4 * (size_t)AT;
    const size_t bw = ckf + 2 * Te + Te * F + 4 + (size_t)(AT / 64) * d->U;
    if (f > g->lds_f) g->lds_f = f;
    if (bw > g->lds_b) g->lds_b = bw;
  }
  g->lds_f *= sizeof(float);
  g->lds_b *= sizeof(float);
  return 0;
}

int put_cols(int R, int Cn, const float *src, float *dst, int ldd, int c0, hipStream_t s) {
  hipLaunchKernelGGL(put_cols_kernel, dim3((R * Cn + 255) / 256), dim3(256), 0, s, R, Cn, src, dst, ldd, c0);
  NABU_LAUNCH_CHECK();
  return 0;
}

size_t multi_attn_part_floats(int B, int Te, int E, int U, int kind, int K, int F, int prob_fn) {
  const nabu_attn_desc a = {sizeof(nabu_attn_desc), B, Te, E, U, kind, K, F, prob_fn};
  const int S = nabu_attn_bwd_slices(&a);
  return S > 0 ? (size_t)B * S * ((size_t)E + 4) : 0;
}

int multi_attn_launch(bool backward, const MultiAttnGeo &g, const MArgs &a, hipStream_t s) {
  const dim3 grid(a.B, g.Smax, g.M);
  if (backward) {
    if (a.kind == 1) return launch_lds(attn_multi_bwd_kernel<true>, grid, dim3(AT), g.lds_b, s, a);
    return launch_lds(attn_multi_bwd_kernel<false>, grid, dim3(AT), g.lds_b, s, a);
  }
  if (a.kind == 1) return launch_lds(attn_multi_fwd_kernel<true>, grid, dim3(AT), g.lds_f, s, a);
  return launch_lds(attn_multi_fwd_kernel<false>, grid, dim3(AT), g.lds_f, s, a);
}

int multi_attn_fwd(int M, int B, int U, int kind, int K, int F, int prob_fn, int step, const int32_t *dec_len, const float *q,
                   const float *ctx_prev, float *ctx, const MultiAttnMem *mems, hipStream_t s) {
  NABU_CHECK_ARG(M >= 1 && M <= MM && mems && dec_len && q && ctx_prev && ctx, "multi_attn_fwd: bad argument");
  nabu_speller_multi_desc d = {};
  d.size = sizeof(d); d.M = M; d.B = B; d.U = U; d.C = 2; d.L = 1; d.num_layers = 1;
  d.kind = kind; d.K = K; d.F = F; d.prob_fn = prob_fn; d.keep_prob = 1.f;
  for (int m = 0; m < M; ++m) { d.Te[m] = mems[m].Te; d.E[m] = mems[m].E; }
  MultiAttnGeo g;
  if (int e = multi_attn_geo(&d, &g)) return e;
  MArgs a = {};
  a.B = B; a.U = U; a.SE = g.SE; a.MU = g.MU; a.kind = kind; a.K = K; a.F = F; a.prob_fn = prob_fn; a.step = step;
  a.dec_len = dec_len; a.q = q; a.ctx_prev = ctx_prev; a.ctx = ctx;
  for (int m = 0; m < M; ++m) {
    MMem &x = a.m[m];
    const MultiAttnMem &y = mems[m];
    x.Te = y.Te; x.E = y.E; x.coff = g.coff[m]; x.S = g.S[m];
    x.enc_len = y.enc_len; x.keys = y.keys; x.values = y.values; x.v = y.v; x.ck = y.ck; x.wf = y.wf;
    x.align_prev = y.align_prev; x.align = y.align; x.znorm = y.znorm; x.part = y.part; x.tickets = y.tickets;
  }
  return multi_attn_launch(false, g, a, s);
}

}  // namespace nabu
