// pkc_conv.hip — the CNN architecture's layer (neural_networks.py:2017-2029):
//   x = drop(act(norm(max_pool1d(conv1d(x), pool))))  over (B, C, L)
// as four launches per layer and direction (include/pkc.h, "Conv1d + max-pool layer"):
//   pkc_conv1d_fwd   : implicit GEMM on the exact-fp32 MFMA, bias + max-pool in the epilogue
//   pkc_conv_post_fwd: LayerNorm (C, L affine) / BatchNorm / none, activation, dropout
//   pkc_conv_post_bwd: their backward over the consumers' gradient slabs
//   pkc_conv1d_bwd   : dX (the same implicit GEMM over the un-pooled gradient), dW / dbias as
//                      per-sample-group partial slabs summed in slab order (no atomics)
//
// Tiles.  v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and
// D[4 (l >> 4) + r][l & 15], r = 0..3.  A workgroup (4 waves) computes 64 positions x 64 output
// channels of one sample: wave w owns positions 16 w .. 16 w + 15 (the A rows) and four
// 16-channel accumulators (the B columns).  The contraction index kk = c * len + k runs over
// input channels and filter taps together, so K = C_in * len needs no multiple of anything: the
// lanes past the end feed zeros.  A fragments come from an LDS strip x[b, c, p0 .. p0 + 63 + len - 1]
// (A[i][kk] = strip[c][i + k]): no im2col tensor exists anywhere.
#include <algorithm>

#include "pkc_common.h"
#include "pkc_ops.h"

namespace pkc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TP = 64;            // positions per workgroup
constexpr int TC = 64;            // output channels per workgroup
constexpr int STRIP = 8192;       // floats of the input strip in LDS
constexpr int CSLD = TP + 1;      // padded row of the epilogue tile

// value at conv position l of the un-pooled gradient: dz[l / pool] where the forward's first
// maximum sat at l, else 0 (positions in the dropped pool tail get 0)
__device__ __forceinline__ float unpool(const float* __restrict__ dz, const uint8_t* __restrict__ off,
                                        int64_t row, int l, int pool, int L_out) {
  if (l < 0) return 0.f;
  const int lp = l / pool;
  if (lp >= L_out) return 0.f;
  return off[row + lp] == (uint8_t)(l - lp * pool) ? dz[row + lp] : 0.f;
}

// MODE 0: z = pool(conv(x) + bias), offsets.   MODE 1: dX = conv_transpose(unpool(dz)).
// Output channels OC (fwd: C_out, dX: C_in), reduction channels RC (fwd: C_in, dX: C_out).
template <int MODE>
__global__ __launch_bounds__(256) void conv_gemm_kernel(pkc_conv1d_args a, int ntiles, int rct) {
  __shared__ float strip[STRIP];
  __shared__ float cs[TC * CSLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  const int oc0 = blockIdx.y * TC;
  const int len = a.len, pool = a.pool, L_in = a.L_in;
  const int L_conv = L_in - len + 1, L_out = L_conv / pool;
  const int OC = MODE == 0 ? a.C_out : a.C_in, RC = MODE == 0 ? a.C_in : a.C_out;
  const int PT = TP / pool;                          // pooled outputs per tile (MODE 0)
  const int p0 = MODE == 0 ? tile * PT * pool : tile * TP;
  const int SW = TP + len - 1;
  const int li = lane & 15, lk = lane >> 4;

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int ntl = (OC - oc0 + 15) / 16;                    // live 16-channel tiles of this workgroup
  ntl = ntl > 4 ? 4 : ntl;

  for (int rc0 = 0; rc0 < RC; rc0 += rct) {
    const int nrc = min(rct, RC - rc0);
    __syncthreads();
    for (int i = tid; i < nrc * SW; i += 256) {
      const int c = i / SW, s = i - c * SW;
      float v;
      if (MODE == 0) {
        const int p = p0 + s;
        v = p < L_in ? a.x[(int64_t)b * a.ldx + (int64_t)(rc0 + c) * L_in + p] : 0.f;
      } else {
        v = unpool(a.dz, a.off, ((int64_t)b * a.C_out + rc0 + c) * L_out, p0 + s - (len - 1), pool,
                   L_out);
      }
      strip[c * SW + s] = v;
    }
    __syncthreads();
    const int K = nrc * len;
    int c = 0, k = lk;                               // this lane's (channel, tap) of kk = kk0 + lk
    while (k >= len) { k -= len; ++c; }
    for (int kk0 = 0; kk0 < K; kk0 += 4) {
      const bool live = kk0 + lk < K;
      const float av = live ? strip[c * SW + 16 * w + li + k] : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < ntl) {
          const int oc = oc0 + 16 * t + li;
          float bv = 0.f;
          if (live && oc < OC) {
            bv = MODE == 0 ? a.W[((int64_t)oc * RC + rc0 + c) * len + k]
                           : a.W[((int64_t)(rc0 + c) * OC + oc) * len + (len - 1 - k)];
          }
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
        }
      }
      k += 4;
      while (k >= len) { k -= len; ++c; }
    }
  }
  // D[4 lk + r][li] of tile t: position 16 w + 4 lk + r, channel 16 t + li
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int oc = oc0 + 16 * t + li;
    const float bias = (MODE == 0 && t < ntl && oc < OC) ? a.bias[oc] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) cs[(16 * t + li) * CSLD + 16 * w + 4 * lk + r] = acc[t][r] + bias;
  }
  __syncthreads();
  if (MODE == 0) {
    const int lp0 = tile * PT;
    for (int i = tid; i < TC * PT; i += 256) {
      const int cl = i / PT, pl = i - cl * PT;
      const int oc = oc0 + cl, lp = lp0 + pl;
      if (oc >= OC || lp >= L_out) continue;
      const float* wv = cs + cl * CSLD + pl * pool;
      float best = wv[0];
      int bi = 0;
      for (int j = 1; j < pool; ++j) {               // first maximum; a NaN wins, as F.max_pool1d
        const float v = wv[j];
        if (v > best || (v != v && best == best)) { best = v; bi = j; }
      }
      const int64_t o = ((int64_t)b * OC + oc) * L_out + lp;
      a.z[o] = best;
      a.off[o] = (uint8_t)bi;
    }
  } else {
    for (int i = tid; i < TC * TP; i += 256) {
      const int cl = i / TP, s = i - cl * TP;
      const int oc = oc0 + cl, p = p0 + s;
      if (oc < OC && p < L_in) a.dx[(int64_t)b * a.lddx + (int64_t)oc * L_in + p] = cs[cl * CSLD + s];
    }
  }
}

// dW[co][n] (n = ci * len + k) partial of one sample group: sum_{b in group} sum_l
// unpool(dz)[b, co, l] * x[b, ci, l + k].  Workgroup: 64 co x 64 n; wave w owns co 16 w .. + 15
// (A rows, contraction over l) and four 16-wide n accumulators.  blockIdx.x == 0 also sums the
// bias gradient of its channels.  Slab s of `work`: C_out * Ktot dW partials, then C_out dbias.
__global__ __launch_bounds__(256) void conv_dw_kernel(pkc_conv1d_args a, float* __restrict__ work,
                                                       int bper) {
  __shared__ float ds[TC * CSLD];
  __shared__ float xs[STRIP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int len = a.len, pool = a.pool, L_in = a.L_in;
  const int L_conv = L_in - len + 1, L_out = L_conv / pool, Le = L_out * pool;
  const int Ktot = a.C_in * len;
  const int n0 = blockIdx.x * 64, co0 = blockIdx.y * TC, slab = blockIdx.z;
  const int ci_lo = n0 / len, ci_hi = min(Ktot - 1, n0 + 63) / len;
  const int nch = ci_hi - ci_lo + 1;
  const int XW = TP + len - 1;
  int boff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + li;
    boff[t] = n < Ktot ? (n / len - ci_lo) * XW + n % len : -1;
  }
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;
  const int b_end = min(a.B, (slab + 1) * bper);
  for (int b = slab * bper; b < b_end; ++b) {
    for (int l0 = 0; l0 < Le; l0 += TP) {
      __syncthreads();
      for (int i = tid; i < TC * TP; i += 256) {
        const int cl = i / TP, j = i - cl * TP;
        const int co = co0 + cl;
        ds[cl * CSLD + j] = co < a.C_out
            ? unpool(a.dz, a.off, ((int64_t)b * a.C_out + co) * L_out, l0 + j, pool, L_out) : 0.f;
      }
      for (int i = tid; i < nch * XW; i += 256) {
        const int c = i / XW, j = i - c * XW;
        const int p = l0 + j;
        xs[i] = p < L_in ? a.x[(int64_t)b * a.ldx + (int64_t)(ci_lo + c) * L_in + p] : 0.f;
      }
      __syncthreads();
      for (int k4 = 0; k4 < TP; k4 += 4) {
        const float av = ds[(16 * w + li) * CSLD + k4 + lk];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float bv = boff[t] >= 0 ? xs[boff[t] + k4 + lk] : 0.f;
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
        }
      }
      if (blockIdx.x == 0 && tid < TC) {
        float s = 0.f;
        for (int j = 0; j < TP; ++j) s += ds[tid * CSLD + j];
        dbacc += s;
      }
    }
  }
  float* out = work + (int64_t)slab * ((int64_t)a.C_out * Ktot + a.C_out);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * w + 4 * lk + r;
      if (co < a.C_out && n < Ktot) out[(int64_t)co * Ktot + n] = acc[t][r];
    }
  }
  if (blockIdx.x == 0 && tid < TC && co0 + tid < a.C_out)
    out[(int64_t)a.C_out * Ktot + co0 + tid] = dbacc;
}

// the partial slabs into dW and dbias, slab order (pkc_ops.h slabsum_body)
__global__ __launch_bounds__(256) void conv_dw_sum_kernel(int ns, int nW, int nb, const float* work,
                                                           float* dW, float* db, int wblocks) {
  const int64_t stride = (int64_t)nW + nb;
  if ((int)blockIdx.x < wblocks) slabsum_body(ns, nW, work, stride, dW, (int64_t)blockIdx.x * 1024, false);
  else slabsum_body(ns, nb, work + nW, stride, db, (int64_t)(blockIdx.x - wblocks) * 1024, false);
}

// ------------------------------------------------------------------ norm / act / dropout
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

struct DropCtx {
  bool on;
  float scale;
  uint32_t thr, key;
};

__device__ __forceinline__ DropCtx drop_ctx(const pkc_conv_post_args& a) {
  DropCtx d;
  d.on = a.drop_p > 0.f;
  d.scale = d.on ? 1.f / (1.f - a.drop_p) : 1.f;
  d.thr = d.on ? (uint32_t)((double)(1.f - a.drop_p) * 4294967296.0) : 0u;
  const int64_t step = a.step_ctr ? *a.step_ctr : 0;
  d.key = hash_seed(a.seed, (uint64_t)a.stream_id, (uint64_t)step);
  return d;
}

__device__ __forceinline__ void post_store(const pkc_conv_post_args& a, const DropCtx& d, int64_t idx,
                                           float pre) {
  float o = act_fwd(a.act, pre);
  if (d.on) {
    uint8_t k;
    if (a.keep_in) k = a.keep_in[idx];
    else k = hash_drop(d.key, (uint32_t)idx) < d.thr;
    if (a.keep) a.keep[idx] = k;
    o = k ? o * d.scale : 0.f;
  }
  if (a.out) a.out[idx] = o;
  if (a.out_bf16) reinterpret_cast<__bf16*>(a.out_bf16)[idx] = (__bf16)o;
}

// grid (C, splits): channel c = blockIdx.x.  BatchNorm in training needs every (b, l) of its
// channel in one workgroup (splits == 1).
__global__ __launch_bounds__(256) void conv_post_fwd_kernel(pkc_conv_post_args a) {
  __shared__ double red[256];
  const int c = blockIdx.x, C = a.C, L = a.L, B = a.B;
  const int tid = threadIdx.x;
  const DropCtx d = drop_ctx(a);
  const int64_t n = (int64_t)B * L;
  if (a.norm == PKC_CONV_NORM_LN) {
    const int lane = tid & 63;
    for (int b = blockIdx.y * 4 + (tid >> 6); b < B; b += gridDim.y * 4) {
      const int64_t row = ((int64_t)b * C + c) * L;
      float s = 0.f;
      for (int l = lane; l < L; l += 64) s += a.z[row + l];
      const float mean = warp_sum(s) / (float)L;
      float q = 0.f;
      for (int l = lane; l < L; l += 64) { const float t = a.z[row + l] - mean; q += t * t; }
      const float sd = sqrtf(warp_sum(q) / (float)(L - 1));    // unbiased, as torch.std
      const float r = 1.f / (sd + a.eps);
      if (lane == 0 && a.ln_stat) {
        a.ln_stat[2 * ((int64_t)b * C + c)] = r;
        a.ln_stat[2 * ((int64_t)b * C + c) + 1] = sd;
      }
      for (int l = lane; l < L; l += 64) {
        const float xh = (a.z[row + l] - mean) * r;
        if (a.xhat) a.xhat[row + l] = xh;
        post_store(a, d, row + l, a.gamma[(int64_t)c * L + l] * xh + a.beta[(int64_t)c * L + l]);
      }
    }
    return;
  }
  float mean = 0.f, invstd = 1.f, g = 1.f, be = 0.f;
  if (a.norm == PKC_NORM_BN_TRAIN) {
    double s = 0.0;
    for (int64_t i = tid; i < n; i += 256) s += a.z[((i / L) * C + c) * L + i % L];
    const double m = block_sum_d(s, red) / (double)n;
    double q = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
      const double t = (double)a.z[((i / L) * C + c) * L + i % L] - m;
      q += t * t;
    }
    const double var = block_sum_d(q, red) / (double)n;
    mean = (float)m;
    invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    if (tid == 0) {
      a.save_mean[c] = mean;
      a.save_invstd[c] = invstd;
      const double unb = n > 1 ? var * (double)n / (double)(n - 1) : var;
      a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
      a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (float)unb;
    }
  } else if (a.norm == PKC_NORM_BN_EVAL) {
    mean = a.running_mean[c];
    invstd = 1.f / sqrtf(a.running_var[c] + a.eps);
  }
  const bool bn = a.norm != PKC_NORM_NONE;
  if (bn) { g = a.gamma[c]; be = a.beta[c]; }
  for (int64_t i = (int64_t)blockIdx.y * 256 + tid; i < n; i += (int64_t)gridDim.y * 256) {
    const int64_t idx = ((i / L) * C + c) * L + i % L;
    const float z = a.z[idx];
    if (!bn) { post_store(a, d, idx, z); continue; }
    const float xh = (z - mean) * invstd;
    if (a.xhat) a.xhat[idx] = xh;
    post_store(a, d, idx, xh * g + be);
  }
}

// dL/d(activation input) at flat index idx: the consumers' slabs summed in slab order, through
// dropout and the activation (pre: the activation's input, recomputed by the caller)
__device__ __forceinline__ float post_g(const pkc_conv_post_args& a, float scale, int64_t idx,
                                        float pre) {
  float dy = a.gslab[idx];
  for (int s = 1; s < a.nslab; ++s) dy += a.gslab[(int64_t)s * a.slab_stride + idx];
  if (a.drop_p > 0.f) dy = a.keep[idx] ? dy * scale : 0.f;
  return dy * act_bwd(a.act, pre, act_fwd(a.act, pre));
}

__global__ __launch_bounds__(256) void conv_post_bwd_kernel(pkc_conv_post_args a) {
  __shared__ double red[256];
  const int c = blockIdx.x, C = a.C, L = a.L, B = a.B;
  const int tid = threadIdx.x;
  const float scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  const int64_t n = (int64_t)B * L;
  if (a.norm == PKC_NORM_NONE) {
    for (int64_t i = (int64_t)blockIdx.y * 256 + tid; i < n; i += (int64_t)gridDim.y * 256) {
      const int64_t idx = ((i / L) * C + c) * L + i % L;
      a.dz[idx] = post_g(a, scale, idx, a.z[idx]);
    }
    return;
  }
  if (a.norm == PKC_CONV_NORM_LN) {
    // y = gamma (x - mean) / (sd + eps) + beta with the unbiased sd: with dxh = g gamma,
    // dx = r (dxh - mean(dxh)) - xhat sum(dxh xhat) / ((L - 1) sd), r = 1 / (sd + eps)
    const int lane = tid & 63;
    for (int b = tid >> 6; b < B; b += 4) {
      const int64_t row = ((int64_t)b * C + c) * L;
      float s1 = 0.f, sx = 0.f;
      for (int l = lane; l < L; l += 64) {
        const float xh = a.xhat[row + l], ga = a.gamma[(int64_t)c * L + l];
        const float dxh = post_g(a, scale, row + l, ga * xh + a.beta[(int64_t)c * L + l]) * ga;
        s1 += dxh;
        sx += dxh * xh;
      }
      s1 = warp_sum(s1);
      sx = warp_sum(sx);
      const float r = a.ln_stat[2 * ((int64_t)b * C + c)], sd = a.ln_stat[2 * ((int64_t)b * C + c) + 1];
      // a row constant along L (a zero-padded frame: conv output == bias everywhere) has sd == 0:
      // torch masks std == 0 to 0 in std_backward, as pkc_norm.hip does
      const float m1 = s1 / (float)L, kx = sd > 0.f ? sx / ((float)(L - 1) * sd) : 0.f;
      for (int l = lane; l < L; l += 64) {
        const float xh = a.xhat[row + l], ga = a.gamma[(int64_t)c * L + l];
        const float dxh = post_g(a, scale, row + l, ga * xh + a.beta[(int64_t)c * L + l]) * ga;
        a.dz[row + l] = r * (dxh - m1) - xh * kx;
      }
    }
    for (int l = tid; l < L; l += 256) {             // affine gradients: over the samples, in order
      const float ga = a.gamma[(int64_t)c * L + l], be = a.beta[(int64_t)c * L + l];
      float dg = 0.f, db = 0.f;
      for (int b = 0; b < B; ++b) {
        const int64_t idx = ((int64_t)b * C + c) * L + l;
        const float xh = a.xhat[idx];
        const float g = post_g(a, scale, idx, ga * xh + be);
        dg += g * xh;
        db += g;
      }
      a.dgamma[(int64_t)c * L + l] = dg;
      a.dbeta[(int64_t)c * L + l] = db;
    }
    return;
  }
  // BatchNorm, training statistics
  const float ga = a.gamma[c], be = a.beta[c], invstd = a.save_invstd[c];
  double sg = 0.0, sgx = 0.0;
  for (int64_t i = tid; i < n; i += 256) {
    const int64_t idx = ((i / L) * C + c) * L + i % L;
    const float xh = a.xhat[idx];
    const float g = post_g(a, scale, idx, xh * ga + be);
    sg += g;
    sgx += (double)g * xh;
  }
  const double dbeta = block_sum_d(sg, red);
  const double dgamma = block_sum_d(sgx, red);
  if (tid == 0) {
    a.dgamma[c] = (float)dgamma;
    a.dbeta[c] = (float)dbeta;
  }
  const float mb = (float)(dbeta / (double)n), mg = (float)(dgamma / (double)n);
  for (int64_t i = tid; i < n; i += 256) {
    const int64_t idx = ((i / L) * C + c) * L + i % L;
    const float xh = a.xhat[idx];
    const float g = post_g(a, scale, idx, xh * ga + be);
    a.dz[idx] = ga * invstd * (g - mb - xh * mg);
  }
}

int conv_check(const pkc_conv1d_args* a, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null args", who);
  PKC_CHECK_ARG(a->B > 0 && a->C_in > 0 && a->C_out > 0 && a->len > 0 && a->pool > 0 && a->L_in > 0,
                "%s: non-positive dimension", who);
  PKC_CHECK_ARG(a->L_in - a->len + 1 >= a->pool, "%s: no pooled output (L_in %d, len %d, pool %d)",
                who, a->L_in, a->len, a->pool);
  PKC_CHECK_ARG(a->pool <= TP, "%s: pool %d > %d", who, a->pool, TP);
  PKC_CHECK_ARG(TP + a->len - 1 <= STRIP / 2, "%s: filter length %d too long", who, a->len);
  PKC_CHECK_ARG(a->ldx >= (int64_t)a->C_in * a->L_in, "%s: ldx < C_in * L_in", who);
  PKC_CHECK_ARG((int64_t)a->B * ((int64_t)a->L_in + 1) < (int64_t)1 << 31 &&
                (int64_t)a->B * a->ldx < (int64_t)1 << 40, "%s: batch too large", who);
  return PKC_OK;
}

constexpr int DW_SLABS = 64;
int dw_slabs(const pkc_conv1d_args* a, int* bper) {
  *bper = (a->B + DW_SLABS - 1) / DW_SLABS;
  return (a->B + *bper - 1) / *bper;
}

}  // namespace
}  // namespace pkc

using namespace pkc;

extern "C" int pkc_conv1d_ok(const pkc_conv1d_args* a) {
  return conv_check(a, "pkc_conv1d_ok") == PKC_OK ? 1 : 0;
}

extern "C" int pkc_conv1d_fwd(const pkc_conv1d_args* a, void* stream) {
  if (int e = conv_check(a, "pkc_conv1d_fwd")) return e;
  PKC_CHECK_ARG(a->x && a->W && a->bias && a->z && a->off, "pkc_conv1d_fwd: null pointer");
  const int SW = TP + a->len - 1;
  const int L_out = (a->L_in - a->len + 1) / a->pool, PT = TP / a->pool;
  const int ntiles = (L_out + PT - 1) / PT;
  const int rct = std::min(a->C_in, STRIP / SW);
  dim3 grid((unsigned)(a->B * ntiles), (unsigned)((a->C_out + TC - 1) / TC));
  hipLaunchKernelGGL(conv_gemm_kernel<0>, grid, dim3(256), 0, S(stream), *a, ntiles, rct);
  PKC_LAUNCH_CHECK("pkc_conv1d_fwd");
  return PKC_OK;
}

// The slab count of a call depends on its B and is not monotone in it (B = 130: 44 slabs, B = 128:
// 64), and a caller sizes the buffer once for its largest batch: the size is that of DW_SLABS
// slabs whatever B is, so one buffer serves every row count.
extern "C" int64_t pkc_conv1d_bwd_work_size(const pkc_conv1d_args* a) {
  if (conv_check(a, "pkc_conv1d_bwd_work_size") != PKC_OK) return -1;
  return (int64_t)DW_SLABS * ((int64_t)a->C_out * a->C_in * a->len + a->C_out);
}

extern "C" int pkc_conv1d_bwd(const pkc_conv1d_args* a, float* work, void* stream) {
  if (int e = conv_check(a, "pkc_conv1d_bwd")) return e;
  PKC_CHECK_ARG(a->x && a->W && a->dz && a->off && a->dW && a->dbias && work,
                "pkc_conv1d_bwd: null pointer");
  PKC_CHECK_ARG(a->dx == nullptr || a->lddx >= (int64_t)a->C_in * a->L_in,
                "pkc_conv1d_bwd: lddx < C_in * L_in");
  const int SW = TP + a->len - 1;
  if (a->dx) {
    const int ntiles = (a->L_in + TP - 1) / TP;
    const int rct = std::min(a->C_out, STRIP / SW);
    dim3 grid((unsigned)(a->B * ntiles), (unsigned)((a->C_in + TC - 1) / TC));
    hipLaunchKernelGGL(conv_gemm_kernel<1>, grid, dim3(256), 0, S(stream), *a, ntiles, rct);
    PKC_LAUNCH_CHECK("pkc_conv1d_bwd dX");
  }
  const int Ktot = a->C_in * a->len;
  // channels one 64-wide n tile can touch, times the strip width, must fit the LDS strip
  const int nch = std::min(a->C_in, 63 / a->len + 2);
  PKC_CHECK_ARG((int64_t)nch * SW <= STRIP, "pkc_conv1d_bwd: filter length %d too long", a->len);
  int bper;
  const int ns = dw_slabs(a, &bper);
  dim3 grid((unsigned)((Ktot + 63) / 64), (unsigned)((a->C_out + TC - 1) / TC), (unsigned)ns);
  hipLaunchKernelGGL(conv_dw_kernel, grid, dim3(256), 0, S(stream), *a, work, bper);
  PKC_LAUNCH_CHECK("pkc_conv1d_bwd dW");
  const int nW = a->C_out * Ktot, wblocks = (nW + 1023) / 1024, bblocks = (a->C_out + 1023) / 1024;
  hipLaunchKernelGGL(conv_dw_sum_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(256), 0, S(stream),
                     ns, nW, a->C_out, work, a->dW, a->dbias, wblocks);
  PKC_LAUNCH_CHECK("pkc_conv1d_bwd slab sum");
  return PKC_OK;
}

static int post_check(const pkc_conv_post_args* a, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null args", who);
  PKC_CHECK_ARG(a->B > 0 && a->C > 0 && a->L > 0, "%s: non-positive dimension", who);
  PKC_CHECK_ARG(a->norm == PKC_NORM_NONE || a->norm == PKC_NORM_BN_TRAIN ||
                a->norm == PKC_NORM_BN_EVAL || a->norm == PKC_CONV_NORM_LN, "%s: norm %d", who, a->norm);
  PKC_CHECK_ARG(a->z, "%s: null z", who);
  PKC_CHECK_ARG(a->norm == PKC_NORM_NONE || (a->gamma && a->beta), "%s: null gamma / beta", who);
  PKC_CHECK_ARG(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: drop_p %g", who, (double)a->drop_p);
  PKC_CHECK_ARG((int64_t)a->B * a->C * a->L < (int64_t)1 << 32, "%s: more than 2^32 elements", who);
  return PKC_OK;
}

extern "C" int pkc_conv_post_fwd(const pkc_conv_post_args* a, void* stream) {
  if (int e = post_check(a, "pkc_conv_post_fwd")) return e;
  PKC_CHECK_ARG(a->out || a->out_bf16, "pkc_conv_post_fwd: no output");
  if (a->norm == PKC_NORM_BN_TRAIN)
    PKC_CHECK_ARG(a->running_mean && a->running_var && a->save_mean && a->save_invstd && a->xhat,
                  "pkc_conv_post_fwd: BatchNorm training buffers missing");
  if (a->norm == PKC_NORM_BN_EVAL)
    PKC_CHECK_ARG(a->running_mean && a->running_var, "pkc_conv_post_fwd: running statistics missing");
  const int64_t n = (int64_t)a->B * a->L;
  int splits = 1;
  if (a->norm == PKC_CONV_NORM_LN) splits = std::max(1, std::min(64, (a->B + 3) / 4));
  else if (a->norm != PKC_NORM_BN_TRAIN) splits = (int)std::max<int64_t>(1, std::min<int64_t>(64, n / 1024));
  hipLaunchKernelGGL(conv_post_fwd_kernel, dim3((unsigned)a->C, (unsigned)splits), dim3(256), 0,
                     S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_conv_post_fwd");
  return PKC_OK;
}

extern "C" int pkc_conv_post_bwd(const pkc_conv_post_args* a, void* stream) {
  if (int e = post_check(a, "pkc_conv_post_bwd")) return e;
  PKC_CHECK_ARG(a->norm != PKC_NORM_BN_EVAL, "pkc_conv_post_bwd: BatchNorm in eval mode");
  PKC_CHECK_ARG(a->gslab && a->nslab >= 1 && a->dz, "pkc_conv_post_bwd: null gradient / dz");
  PKC_CHECK_ARG(a->drop_p == 0.f || a->keep, "pkc_conv_post_bwd: dropout without its keep mask");
  if (a->norm != PKC_NORM_NONE)
    PKC_CHECK_ARG(a->xhat && a->dgamma && a->dbeta, "pkc_conv_post_bwd: xhat / dgamma / dbeta missing");
  if (a->norm == PKC_NORM_BN_TRAIN) PKC_CHECK_ARG(a->save_invstd, "pkc_conv_post_bwd: save_invstd missing");
  if (a->norm == PKC_CONV_NORM_LN) PKC_CHECK_ARG(a->ln_stat, "pkc_conv_post_bwd: ln_stat missing");
  const int64_t n = (int64_t)a->B * a->L;
  const int splits = a->norm == PKC_NORM_NONE
      ? (int)std::max<int64_t>(1, std::min<int64_t>(64, n / 1024)) : 1;
  hipLaunchKernelGGL(conv_post_bwd_kernel, dim3((unsigned)a->C, (unsigned)splits), dim3(256), 0,
                     S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_conv_post_bwd");
  return PKC_OK;
}
