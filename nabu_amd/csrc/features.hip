// features.hip — fbank / MFCC features of a ragged batch of utterances (gfx950).
//
// Two launches per batch, whatever it holds:
//   feat_static_kernel   one workgroup per tile of FEAT_TILE consecutive frames of one utterance; a wave takes a frame
//                        at a time: samples straight from HBM (int16, pre-emphasis on the way in; neighbouring frames
//                        overlap by frame_len - frame_step samples, which the caches absorb), a real nfft-point
//                        transform as a complex nfft/2-point Stockham radix-2 transform in the wave's own LDS plus the
//                        usual split pass, power spectrum, energy, band sums, log (and DCT + lifter for MFCC);
//   feat_dynamic_kernel  one workgroup per utterance and group of 16 static columns: derivative columns, then mean and
//                        variance normalisation of its columns (two passes).
// Every sum has a fixed order that depends on the utterance alone (lane-strided partials, then a butterfly or a serial
// sum over 16 partials): no atomics, and an utterance's features are the same bits in any batch.
// The tables (twiddles, filter bands, DCT) are computed on the host in double precision (nabu_feat_tables_host).
#include <math.h>
#include <cmath>
#include <string.h>

#include <vector>

#include "common.h"

namespace nabu {
namespace {

constexpr int FEAT_TILE = 16;         // frames per workgroup of feat_static_kernel
constexpr int FEAT_MAX_FILT = 128;    // nfilt (one wave's log filter outputs sit in its transform buffer)
constexpr int DYN_COLS = 16;          // static columns per workgroup of feat_dynamic_kernel
constexpr int DYN_ROWS = 16;          // time lanes per column
// log(2^-52) rounded to fp32: what the reference's "replace an exact zero by finfo(float).eps" gives after the log
constexpr float LOG_EPS = -36.04365338911715f;

struct Layout {                       // byte offsets of the tables in the workspace
  size_t tw, band, weights, dct, total;
  int n_weights;
};

struct Bank {
  std::vector<int> start, len, off;
  std::vector<double> w;
};

int highfreq_of(const nabu_feat_desc *d) { return d->highfreq < 0 ? d->rate / 2 : d->highfreq; }

int check_desc(const nabu_feat_desc *d) {
  NABU_CHECK_ARG(d != nullptr, "nabu_feat: null descriptor");
  NABU_CHECK_ARG(d->size == sizeof(nabu_feat_desc), "nabu_feat: descriptor size %u, expected %zu", d->size,
                 sizeof(nabu_feat_desc));
  NABU_CHECK_ARG(d->rate > 0 && d->rate <= 384000, "nabu_feat: rate %d", d->rate);
  NABU_CHECK_ARG(d->winlen > 0 && d->winstep > 0 && d->winlen < 10 && d->winstep < 10,
                 "nabu_feat: winlen %g / winstep %g must be positive (seconds)", d->winlen, d->winstep);
  const long long fl = llround(d->winlen * d->rate), fs = llround(d->winstep * d->rate);   // half away from zero
  NABU_CHECK_ARG(fl >= 1 && fs >= 1, "nabu_feat: winlen / winstep shorter than one sample at rate %d", d->rate);
  NABU_CHECK_ARG(d->frame_len == fl && d->frame_step == fs,
                 "nabu_feat: frame_len %d / frame_step %d, but winlen*rate and winstep*rate round (half away from "
                 "zero) to %lld / %lld", d->frame_len, d->frame_step, fl, fs);
  NABU_CHECK_ARG(d->kind == NABU_FEAT_FBANK || d->kind == NABU_FEAT_MFCC, "nabu_feat: kind %d", d->kind);
  NABU_CHECK_ARG(d->nfilt >= 1 && d->nfilt <= FEAT_MAX_FILT, "nabu_feat: nfilt %d not in 1..%d", d->nfilt,
                 FEAT_MAX_FILT);
  if (d->kind == NABU_FEAT_MFCC)
    NABU_CHECK_ARG(d->numcep >= 1 && d->numcep <= d->nfilt, "nabu_feat: numcep %d not in 1..nfilt (%d)", d->numcep,
                   d->nfilt);
  NABU_CHECK_ARG((d->include_energy | 1) == 1 && (d->mvn | 1) == 1, "nabu_feat: include_energy and mvn are 0 or 1");
  NABU_CHECK_ARG(d->dynamic >= 0 && d->dynamic <= 2, "nabu_feat: dynamic %d (0 nodelta, 1 delta, 2 ddelta)",
                 d->dynamic);
  NABU_CHECK_ARG(std::isfinite(d->preemph) && std::isfinite(d->ceplifter), "nabu_feat: preemph / ceplifter not finite");
  const int hf = highfreq_of(d);
  NABU_CHECK_ARG(d->lowfreq >= 0 && d->lowfreq < hf && hf <= d->rate / 2,
                 "nabu_feat: need 0 <= lowfreq (%d) < highfreq (%d) <= rate/2 (%d)", d->lowfreq, hf, d->rate / 2);
  const int n = d->nfft;
  if (n < 256 || n > 2048 || (n & (n - 1)))
    return fail(NABU_EUNSUP, "nabu_feat: nfft %d is not a power of two in 256..2048", n);
  if (d->frame_len > n)
    return fail(NABU_EUNSUP, "nabu_feat: frame_len %d > nfft %d (the frame would be cropped)", d->frame_len, n);
  return 0;
}

int n_static(const nabu_feat_desc *d) {
  return (d->kind == NABU_FEAT_MFCC ? d->numcep : d->nfilt) + d->include_energy;
}

// snip + framing of one utterance.  Plain double arithmetic in the order the reference's Python evaluates it
// (no fused multiply-add: the truncations below sit on it).
int frames_of(const nabu_feat_desc *d, long long len, long long *kept_out) {
#pragma clang fp contract(off)
  const double wl = d->winlen * d->rate, ws = d->winstep * d->rate;
  const long long num = (long long)(((double)len - wl) / ws);       // trunc, as int()
  long long kept = (long long)((double)num * d->winstep * d->rate + wl);
  if (kept > len) kept = len;
  if (kept < 0) kept = 0;
  if (kept_out) *kept_out = kept;
  if (kept <= d->frame_len) return 1;
  return (int)(1 + (kept - d->frame_len + d->frame_step - 1) / d->frame_step);
}

double hz2mel(double hz) { return 2595.0 * log10(1.0 + hz / 700.0); }
double mel2hz(double mel) { return 700.0 * (pow(10.0, mel / 2595.0) - 1.0); }

void build_bank(const nabu_feat_desc *d, Bank *b) {
  const int nf = d->nfilt;
  const double lo = hz2mel(d->lowfreq), hi = hz2mel(highfreq_of(d));
  std::vector<double> bins(nf + 2);
  const double step = (hi - lo) / (nf + 1);
  for (int i = 0; i < nf + 2; ++i) {
    const double mel = i == nf + 1 ? hi : i * step + lo;              // numpy.linspace
    bins[i] = floor((d->nfft + 1) * mel2hz(mel) / d->rate);
  }
  b->start.resize(nf), b->len.resize(nf), b->off.resize(nf);
  b->w.clear();
  for (int j = 0; j < nf; ++j) {
    const int b0 = (int)bins[j], b1 = (int)bins[j + 1], b2 = (int)bins[j + 2];
    b->start[j] = b0, b->len[j] = b2 - b0, b->off[j] = (int)b->w.size();
    for (int i = b0; i < b1; ++i) b->w.push_back((i - bins[j]) / (bins[j + 1] - bins[j]));
    for (int i = b1; i < b2; ++i) b->w.push_back((bins[j + 2] - i) / (bins[j + 2] - bins[j + 1]));
  }
}

Layout layout_of(const nabu_feat_desc *d, int n_weights) {
  Layout l;
  l.n_weights = n_weights;
  l.tw = 0;
  l.band = l.tw + (size_t)(d->nfft / 2) * sizeof(float2);
  l.weights = l.band + (size_t)3 * d->nfilt * sizeof(int32_t);
  l.dct = align_up(l.weights + (size_t)n_weights * sizeof(float), 16);
  l.total = align_up(l.dct + (d->kind == NABU_FEAT_MFCC ? (size_t)d->numcep * d->nfilt * sizeof(float) : 0), 256);
  return l;
}

struct StaticArgs {
  const int16_t *samples;
  const int32_t *sample_off, *kept, *frame_off;
  const float2 *tw;
  const int32_t *band;       // start[nfilt], len[nfilt], off[nfilt]
  const float *weights, *dct;
  float *out;
  int frame_len, frame_step, nfft, nfilt, numcep, kind, include_energy, dim;
  float preemph;
};

// dynamic LDS: twiddles float2[nfft/2], then per wave two float2[nfft/2] transform buffers
__global__ __launch_bounds__(256) void feat_static_kernel(StaticArgs a) {
  extern __shared__ __attribute__((aligned(16))) char feat_smem[];
  const int M = a.nfft >> 1;
  float2 *tw = reinterpret_cast<float2 *>(feat_smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  float2 *bufA = tw + M + (size_t)wave * 2 * M, *bufB = bufA + M;
  for (int i = threadIdx.x; i < M; i += blockDim.x) tw[i] = a.tw[i];

  const int u = blockIdx.y;
  const int T = a.frame_off[u + 1] - a.frame_off[u];
  const int f0 = blockIdx.x * FEAT_TILE;
  if (f0 >= T) return;                                  // whole workgroup: no barrier is left behind
  const int16_t *s = a.samples + a.sample_off[u];
  const int kept = a.kept[u];
  float *out = a.out + (size_t)a.frame_off[u] * a.dim;
  const int nstat = (a.kind == NABU_FEAT_MFCC ? a.numcep : a.nfilt);
  const float inv_nfft = 1.0f / (float)a.nfft;

  for (int it = 0; it < FEAT_TILE; it += nwaves) {      // the same trip count for every wave: barriers inside
    const int f = f0 + it + wave;
    const bool live = f < T;
    // (1) the frame, pre-emphasised, as nfft/2 complex numbers (even sample, odd sample)
    const int base = f * a.frame_step;
    for (int n = lane; n < M; n += 64) {
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = 2 * n + h, pos = base + i;
        float x = 0.f;
        if (live && i < a.frame_len && pos < kept) {
          x = (float)s[pos];
          if (pos > 0) x -= a.preemph * (float)s[pos - 1];
        }
        v[h] = x;
      }
      bufA[n] = make_float2(v[0], v[1]);
    }
    // (2) Stockham radix-2 stages, ping-pong between the two buffers
    float2 *src = bufA, *dst = bufB;
    for (int p = 1; p < M; p <<= 1) {
      __syncthreads();
      const int tstride = M / p;                        // W_{2p}^k = W_nfft^{k * nfft/(2p)}
      for (int i = lane; i < (M >> 1); i += 64) {
        const int k = i & (p - 1), j = ((i - k) << 1) + k;
        const float2 w = tw[k * tstride], x0 = src[i], x1 = src[i + (M >> 1)];
        const float2 y = make_float2(w.x * x1.x - w.y * x1.y, w.x * x1.y + w.y * x1.x);
        dst[j] = make_float2(x0.x + y.x, x0.y + y.y);
        dst[j + p] = make_float2(x0.x - y.x, x0.y - y.y);
      }
      float2 *t = src;
      src = dst, dst = t;
    }
    __syncthreads();
    // (3) split pass: spectrum of the real frame from Z = src, power into dst (as floats, bins 0..M)
    float *pw = reinterpret_cast<float *>(dst);
    float esum = 0.f;
    for (int k = lane; k <= M; k += 64) {
      const float2 za = src[k & (M - 1)], zb = src[(M - k) & (M - 1)];
      const float er = 0.5f * (za.x + zb.x), ei = 0.5f * (za.y - zb.y);
      const float orr = 0.5f * (za.y + zb.y), oi = -0.5f * (za.x - zb.x);
      const float2 w = k < M ? tw[k] : make_float2(-1.f, 0.f);
      const float xr = er + (w.x * orr - w.y * oi), xi = ei + (w.x * oi + w.y * orr);
      const float pk = (xr * xr + xi * xi) * inv_nfft;
      pw[k] = pk;
      esum += pk;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) esum += __shfl_xor(esum, o);
    __syncthreads();
    // (4) band sums and logarithms
    float *logfb = reinterpret_cast<float *>(src);      // Z is spent
    for (int j = lane; j < a.nfilt; j += 64) {
      const int b0 = a.band[j], bl = a.band[a.nfilt + j];
      const float *w = a.weights + a.band[2 * a.nfilt + j];
      float acc = 0.f;
      for (int i = 0; i < bl; ++i) acc += w[i] * pw[b0 + i];
      const float lg = acc == 0.f ? LOG_EPS : logf(acc);
      if (a.kind == NABU_FEAT_FBANK) {
        if (live) out[(size_t)f * a.dim + j] = lg;
      } else {
        logfb[j] = lg;
      }
    }
    if (live && a.include_energy && lane == 0) out[(size_t)f * a.dim + nstat] = esum == 0.f ? LOG_EPS : logf(esum);
    if (a.kind == NABU_FEAT_MFCC) {
      __syncthreads();
      for (int n = lane; n < a.numcep; n += 64) {
        const float *dr = a.dct + (size_t)n * a.nfilt;
        float acc = 0.f;
        for (int j = 0; j < a.nfilt; ++j) acc += dr[j] * logfb[j];
        if (live) out[(size_t)f * a.dim + n] = acc;
      }
    }
    __syncthreads();                                    // the buffers are free for the next frame
  }
}

// index into a sequence of T >= 1 elements extended by reflection (... b a | a b ... y z | z y ...)
__device__ __forceinline__ int reflect(int i, int T) {
  while (i < 0 || i >= T) i = i < 0 ? -i - 1 : 2 * T - 1 - i;
  return i;
}

// blockDim = DYN_COLS x DYN_ROWS; x[t * dim + col] for one utterance
__global__ __launch_bounds__(DYN_COLS *DYN_ROWS) void feat_dynamic_kernel(float *out, const int32_t *frame_off, int ns,
                                                                           int dynamic, int mvn, int dim) {
  __shared__ float red[DYN_ROWS][DYN_COLS + 1];
  const int tx = threadIdx.x % DYN_COLS, ty = threadIdx.x / DYN_COLS;
  const int u = blockIdx.y, c = blockIdx.x * DYN_COLS + tx;
  const bool live = c < ns;
  const int T = frame_off[u + 1] - frame_off[u];
  float *x = out + (size_t)frame_off[u] * dim;
  for (int q = 1; q <= dynamic; ++q) {
    const int from = (q - 1) * ns + c, to = q * ns + c;
    if (live)
      for (int t = ty; t < T; t += DYN_ROWS) {
        const float p2 = x[(size_t)reflect(t + 2, T) * dim + from], p1 = x[(size_t)reflect(t + 1, T) * dim + from];
        const float m1 = x[(size_t)reflect(t - 1, T) * dim + from], m2 = x[(size_t)reflect(t - 2, T) * dim + from];
        x[(size_t)t * dim + to] = 2.f * (p2 - m2) + (p1 - m1);
      }
    __threadfence_block();
    __syncthreads();                                    // the next order reads what other time lanes wrote
  }
  if (!mvn) return;
  for (int q = 0; q <= dynamic; ++q) {
    const int col = q * ns + c;
    float acc = 0.f;
    if (live)
      for (int t = ty; t < T; t += DYN_ROWS) acc += x[(size_t)t * dim + col];
    red[ty][tx] = acc;
    __syncthreads();
    float mean = 0.f;
    for (int r = 0; r < DYN_ROWS; ++r) mean += red[r][tx];
    mean /= (float)T;
    __syncthreads();
    acc = 0.f;
    if (live)
      for (int t = ty; t < T; t += DYN_ROWS) {
        const float dv = x[(size_t)t * dim + col] - mean;
        acc += dv * dv;
      }
    red[ty][tx] = acc;
    __syncthreads();
    float var = 0.f;
    for (int r = 0; r < DYN_ROWS; ++r) var += red[r][tx];
    const float sd = sqrtf(var / (float)T);
    __syncthreads();
    if (live)
      for (int t = ty; t < T; t += DYN_ROWS) x[(size_t)t * dim + col] = (x[(size_t)t * dim + col] - mean) / sd;
  }
}

}  // namespace
}  // namespace nabu

using namespace nabu;

extern "C" int nabu_feat_dim(const nabu_feat_desc *d) {
  if (int rc = check_desc(d)) return rc;
  return n_static(d) * (1 + d->dynamic);
}

extern "C" int nabu_feat_num_frames(const nabu_feat_desc *d, long long n_samples) {
  if (int rc = check_desc(d)) return rc;
  NABU_CHECK_ARG(n_samples >= 1 && n_samples <= INT32_MAX, "nabu_feat_num_frames: %lld samples", n_samples);
  return frames_of(d, n_samples, nullptr);
}

extern "C" int nabu_feat_plan_host(const nabu_feat_desc *d, int n_utt, const int32_t *sample_offsets_host,
                                   int32_t *frame_offsets_host, int32_t *kept_host) {
  if (int rc = check_desc(d)) return rc;
  NABU_CHECK_ARG(n_utt >= 1 && sample_offsets_host && frame_offsets_host && kept_host,
                 "nabu_feat_plan_host: null pointer or n_utt %d < 1", n_utt);
  long long rows = 0;
  frame_offsets_host[0] = 0;
  for (int u = 0; u < n_utt; ++u) {
    const long long len = (long long)sample_offsets_host[u + 1] - sample_offsets_host[u];
    NABU_CHECK_ARG(sample_offsets_host[u] >= 0 && len >= 1, "nabu_feat_plan_host: utterance %d has %lld samples", u,
                   len);
    long long kept;
    rows += frames_of(d, len, &kept);
    NABU_CHECK_ARG(rows <= INT32_MAX / 512, "nabu_feat_plan_host: too many frames in one batch (%lld)", rows);
    kept_host[u] = (int32_t)kept;
    frame_offsets_host[u + 1] = (int32_t)rows;
  }
  return 0;
}

extern "C" size_t nabu_feat_ws_bytes(const nabu_feat_desc *d) {
  if (check_desc(d)) return 0;
  Bank b;
  build_bank(d, &b);
  return layout_of(d, (int)b.w.size()).total;
}

extern "C" int nabu_feat_tables_host(const nabu_feat_desc *d, void *ws_host, size_t ws_bytes) {
  if (int rc = check_desc(d)) return rc;
  NABU_CHECK_ARG(ws_host != nullptr, "nabu_feat_tables_host: null pointer");
  Bank b;
  build_bank(d, &b);
  const Layout l = layout_of(d, (int)b.w.size());
  if (ws_bytes < l.total) return fail(NABU_EWS, "nabu_feat_tables_host: %zu bytes, need %zu", ws_bytes, l.total);
  char *base = static_cast<char *>(ws_host);
  memset(base, 0, l.total);
  float2 *tw = reinterpret_cast<float2 *>(base + l.tw);
  for (int k = 0; k < d->nfft / 2; ++k) {
    const double ang = -2.0 * M_PI * k / d->nfft;
    tw[k] = make_float2((float)cos(ang), (float)sin(ang));
  }
  int32_t *band = reinterpret_cast<int32_t *>(base + l.band);
  for (int j = 0; j < d->nfilt; ++j)
    band[j] = b.start[j], band[d->nfilt + j] = b.len[j], band[2 * d->nfilt + j] = b.off[j];
  float *w = reinterpret_cast<float *>(base + l.weights);
  for (size_t i = 0; i < b.w.size(); ++i) w[i] = (float)b.w[i];
  if (d->kind == NABU_FEAT_MFCC) {
    float *dct = reinterpret_cast<float *>(base + l.dct);
    const int N = d->nfilt;
    const double L = d->ceplifter;
    for (int n = 0; n < d->numcep; ++n) {
      const double scale = n == 0 ? sqrt(1.0 / N) : sqrt(2.0 / N);
      const double lift = L > 0 ? 1.0 + (L / 2.0) * sin(M_PI * n / L) : 1.0;
      for (int j = 0; j < N; ++j) dct[(size_t)n * N + j] = (float)(lift * scale * cos(M_PI * n * (2 * j + 1) / (2.0 * N)));
    }
  }
  return 0;
}

extern "C" int nabu_feat_compute(const nabu_feat_desc *d, int n_utt, int max_frames, const int16_t *samples,
                                 const int32_t *sample_offsets, const int32_t *kept, const int32_t *frame_offsets,
                                 float *out, const void *ws, size_t ws_bytes, nabu_stream_t stream) {
  if (int rc = check_desc(d)) return rc;
  NABU_CHECK_ARG(samples && sample_offsets && kept && frame_offsets && out && ws, "nabu_feat_compute: null pointer");
  NABU_CHECK_ARG(n_utt >= 1 && n_utt <= 65535, "nabu_feat_compute: n_utt %d not in 1..65535", n_utt);
  NABU_CHECK_ARG(max_frames >= 1, "nabu_feat_compute: max_frames %d", max_frames);
  NABU_CHECK_ARG(((uintptr_t)ws & 15) == 0, "nabu_feat_compute: ws must be 16-byte aligned");
  Bank b;
  build_bank(d, &b);
  const Layout l = layout_of(d, (int)b.w.size());
  if (ws_bytes < l.total) return fail(NABU_EWS, "nabu_feat_compute: workspace %zu bytes, need %zu", ws_bytes, l.total);
  const char *base = static_cast<const char *>(ws);
  StaticArgs a;
  a.samples = samples, a.sample_off = sample_offsets, a.kept = kept, a.frame_off = frame_offsets;
  a.tw = reinterpret_cast<const float2 *>(base + l.tw);
  a.band = reinterpret_cast<const int32_t *>(base + l.band);
  a.weights = reinterpret_cast<const float *>(base + l.weights);
  a.dct = reinterpret_cast<const float *>(base + l.dct);
  a.out = out;
  a.frame_len = d->frame_len, a.frame_step = d->frame_step, a.nfft = d->nfft, a.nfilt = d->nfilt;
  a.numcep = d->numcep, a.kind = d->kind, a.include_energy = d->include_energy;
  a.dim = n_static(d) * (1 + d->dynamic);
  a.preemph = d->preemph;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 4 waves per workgroup (2 at nfft 2048): twiddles 4*nfft bytes + 8*nfft bytes per wave, at most 40 KiB
  const int waves = d->nfft > 1024 ? 2 : 4;
  const size_t lds = (size_t)(d->nfft / 2) * sizeof(float2) * (1 + 2 * waves);
  const dim3 grid((max_frames + FEAT_TILE - 1) / FEAT_TILE, n_utt);
  hipLaunchKernelGGL(feat_static_kernel, grid, dim3(64 * waves), lds, s, a);
  NABU_LAUNCH_CHECK();
  if (d->dynamic > 0 || d->mvn) {
    const int ns = n_static(d);
    hipLaunchKernelGGL(feat_dynamic_kernel, dim3((ns + DYN_COLS - 1) / DYN_COLS, n_utt), dim3(DYN_COLS * DYN_ROWS), 0,
                       s, out, frame_offsets, ns, d->dynamic, d->mvn, a.dim);
    NABU_LAUNCH_CHECK();
  }
  return 0;
}
