// pkc — the sinc filter bank of the SincNet architecture (reference neural_networks.py:2146-2283,
// SincConv): the first layer's convolution weights are not a parameter tensor but N band-pass
// filters generated before every forward from two learned vectors, low_hz_ and band_hz_.
//
//   low  = min_low_hz / sr + |low_hz_|            high = low + min_band_hz / sr + |band_hz_|
//   lp(f)[k] = 2 f sinc(2 pi (f n_[k]) sr)        sinc = sin(x) / x on the left half, 1 at the
//   bp = lp(high) - lp(low)                       centre, the right half the flip of the left
//   filters = bp / max_k(bp) * window_
//
// Forward: fp32 in the reference's operation order, every product and difference rounded on its
// own (no contraction into fma), precise sinf.  One workgroup per filter: the left half and the
// centre go through LDS, the first maximum is found by a fixed tree, the taps are mirrored on the
// way out.
//
// Backward: dW (the convolution's weight gradient) -> d low_hz_, d band_hz_.  The filter bank is
// tiny (N x K = 128 x 129 at full size) and its gradient is a cancelling sum of cosines at
// arguments up to ~200 rad, so the backward re-evaluates the formula in fp64 from the two
// parameters (the maximum is taken at the index the forward saved) and rounds once at the end.
// One workgroup per filter, per-thread partial sums in tap order and a fixed tree over the
// threads: no atomics, equal inputs give bit-identical outputs.
#include "pkc_common.h"

namespace pkc {
namespace {

constexpr int SINC_THREADS = 256;
constexpr int SINC_MAX_K = 4033;                       // the longest filter pkc_conv1d_fwd takes
constexpr int SINC_HALF = (SINC_MAX_K - 1) / 2 + 1;    // left half + centre
constexpr int NONE = 0x7fffffff;                       // no tap seen yet (threads past the half)

// lp(f) at a left-half tap: 2 f sin(x) / x with x = ((2 pi) (f n)) sr, each step rounded to fp32
__device__ __forceinline__ float lowpass_tap(float f, float n, float sr) {
  const float x = __fmul_rn(__fmul_rn(6.283185307179586f, __fmul_rn(f, n)), sr);
  return __fmul_rn(__fmul_rn(2.f, f), __fdiv_rn(sinf(x), x));
}

__global__ __launch_bounds__(SINC_THREADS) void sinc_fwd_kernel(pkc_sinc_args a, float c_low,
                                                                float c_band) {
  __shared__ float bp[SINC_HALF];
  __shared__ float rv[SINC_THREADS];
  __shared__ int ri[SINC_THREADS];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int K = a.K, h = (K - 1) / 2;
  const float low = __fadd_rn(c_low, fabsf(a.low_hz[i]));
  const float high = __fadd_rn(__fadd_rn(low, c_band), fabsf(a.band_hz[i]));
  float best = 0.f;
  int bi = NONE;
  for (int j = tid; j <= h; j += SINC_THREADS) {
    float v;
    if (j < h) {
      const float n = a.n_[j];
      v = __fsub_rn(lowpass_tap(high, n, a.sr), lowpass_tap(low, n, a.sr));
    } else {
      v = __fsub_rn(__fmul_rn(2.f, high), __fmul_rn(2.f, low));     // sinc = 1 at the centre
    }
    bp[j] = v;
    // ascending j, so the first maximum stays; as torch.max, a NaN beats numbers (the first one)
    if (bi == NONE || (best == best && (v != v || v > best))) { best = v; bi = j; }
  }
  rv[tid] = best;
  ri[tid] = bi;
  __syncthreads();
  for (int o = SINC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const float v0 = rv[tid], v1 = rv[tid + o];
      const int i0 = ri[tid], i1 = ri[tid + o];
      const bool n0 = v0 != v0, n1 = v1 != v1;
      bool take;                                                     // the other entry wins
      if (i1 == NONE) take = false;
      else if (i0 == NONE) take = true;
      else if (n0 || n1) take = n1 && (!n0 || i1 < i0);
      else take = v1 > v0 || (v1 == v0 && i1 < i0);
      if (take) { rv[tid] = v1; ri[tid] = i1; }
    }
    __syncthreads();
  }
  const float mx = rv[0];
  if (tid == 0) {
    a.max_[i] = mx;
    a.max_idx[i] = ri[0];
  }
  float* out = a.filters + (int64_t)i * K;
  for (int k = tid; k < K; k += SINC_THREADS) {
    const int j = k <= h ? k : K - 1 - k;
    out[k] = __fmul_rn(__fdiv_rn(bp[j], mx), a.window[k]);
  }
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = SINC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(SINC_THREADS) void sinc_bwd_kernel(pkc_sinc_args a, double c_low,
                                                                double c_band) {
  __shared__ double red[SINC_THREADS];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int K = a.K, h = (K - 1) / 2;
  const double TWO_PI = 6.283185307179586;
  const double pl = (double)a.low_hz[i], pb = (double)a.band_hz[i], sr = (double)a.sr;
  const double low = c_low + fabs(pl);
  const double high = low + c_band + fabs(pb);
  const float* dW = a.dW + (int64_t)i * K;
  // per left-half tap j (the right half is a flip of computed values: its gradient belongs to the
  // mirrored tap): g = dW[j] w[j] + dW[K-1-j] w[K-1-j];  sums of g bp, g dbp/dlow, g dbp/dhigh
  double s_bp = 0.0, s_lo = 0.0, s_hi = 0.0;
  for (int j = tid; j <= h; j += SINC_THREADS) {
    double g = (double)dW[j] * (double)a.window[j];
    if (j < h) {
      g += (double)dW[K - 1 - j] * (double)a.window[K - 1 - j];
      const double n = (double)a.n_[j];
      const double x1 = TWO_PI * (low * n) * sr, x2 = TWO_PI * (high * n) * sr;
      s_bp += g * (2.0 * high * (sin(x2) / x2) - 2.0 * low * (sin(x1) / x1));
      s_lo -= g * 2.0 * cos(x1);            // d lp(f)[j] / df = 2 cos(x_j)
      s_hi += g * 2.0 * cos(x2);
    } else {
      s_bp += g * (2.0 * high - 2.0 * low);
      s_lo -= g * 2.0;
      s_hi += g * 2.0;
    }
  }
  s_bp = block_sum_d(s_bp, red);
  s_lo = block_sum_d(s_lo, red);
  s_hi = block_sum_d(s_hi, red);
  if (tid == 0) {
    int m = a.max_idx[i];
    if (m < 0 || m > h) m = h;
    double mx, m_lo, m_hi;                  // the maximum and its derivatives at the saved index
    if (m < h) {
      const double n = (double)a.n_[m];
      const double x1 = TWO_PI * (low * n) * sr, x2 = TWO_PI * (high * n) * sr;
      mx = 2.0 * high * (sin(x2) / x2) - 2.0 * low * (sin(x1) / x1);
      m_lo = -2.0 * cos(x1);
      m_hi = 2.0 * cos(x2);
    } else {
      mx = 2.0 * high - 2.0 * low;
      m_lo = -2.0;
      m_hi = 2.0;
    }
    const double dmax = -s_bp / (mx * mx);
    const double dlow = s_lo / mx + dmax * m_lo;
    const double dhigh = s_hi / mx + dmax * m_hi;
    // high = low + ... : low_hz_ reaches both; the gradient of |.| at 0 is 0, as torch.abs has it
    const double sl = pl > 0.0 ? 1.0 : pl < 0.0 ? -1.0 : 0.0;
    const double sb = pb > 0.0 ? 1.0 : pb < 0.0 ? -1.0 : 0.0;
    a.dlow[i] = sl == 0.0 ? 0.f : (float)(sl * (dlow + dhigh));
    a.dband[i] = sb == 0.0 ? 0.f : (float)(sb * dhigh);
  }
}

int sinc_check(const pkc_sinc_args* a, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null args", who);
  PKC_CHECK_ARG(a->N > 0 && a->N <= 65535, "%s: N %d outside 1 .. 65535", who, a->N);
  PKC_CHECK_ARG(a->K >= 1 && a->K <= SINC_MAX_K, "%s: K %d outside 1 .. %d", who, a->K, SINC_MAX_K);
  PKC_CHECK_ARG(a->K % 2 == 1, "%s: K %d is even (SincConv makes the length odd, "
                "neural_networks.py:2193-2194)", who, a->K);
  PKC_CHECK_ARG(a->sr > 0.f, "%s: sample rate %g", who, (double)a->sr);
  PKC_CHECK_ARG(a->min_low_hz >= 0.f && a->min_band_hz >= 0.f, "%s: negative min_low_hz / "
                "min_band_hz", who);
  return PKC_OK;
}

}  // namespace
}  // namespace pkc

using namespace pkc;

extern "C" int pkc_sinc_ok(const pkc_sinc_args* a) {
  return sinc_check(a, "pkc_sinc_ok") == PKC_OK ? 1 : 0;
}

extern "C" int pkc_sinc_filters_fwd(const pkc_sinc_args* a, void* stream) {
  if (int rc = sinc_check(a, "pkc_sinc_filters_fwd")) return rc;
  PKC_CHECK_ARG(a->low_hz && a->band_hz && a->n_ && a->window && a->filters && a->max_ && a->max_idx,
                "pkc_sinc_filters_fwd: null pointer");
  // min_low_hz / sr is a Python float in the reference, rounded to fp32 when added to the tensor
  const float c_low = (float)((double)a->min_low_hz / (double)a->sr);
  const float c_band = (float)((double)a->min_band_hz / (double)a->sr);
  hipLaunchKernelGGL(sinc_fwd_kernel, dim3((unsigned)a->N), dim3(SINC_THREADS), 0, S(stream), *a,
                     c_low, c_band);
  PKC_LAUNCH_CHECK("pkc_sinc_filters_fwd");
  return PKC_OK;
}

extern "C" int pkc_sinc_filters_bwd(const pkc_sinc_args* a, void* stream) {
  if (int rc = sinc_check(a, "pkc_sinc_filters_bwd")) return rc;
  PKC_CHECK_ARG(a->low_hz && a->band_hz && a->n_ && a->window && a->max_idx && a->dW && a->dlow &&
                a->dband, "pkc_sinc_filters_bwd: null pointer");
  hipLaunchKernelGGL(sinc_bwd_kernel, dim3((unsigned)a->N), dim3(SINC_THREADS), 0, S(stream), *a,
                     (double)a->min_low_hz / (double)a->sr, (double)a->min_band_hz / (double)a->sr);
  PKC_LAUNCH_CHECK("pkc_sinc_filters_bwd");
  return PKC_OK;
}
