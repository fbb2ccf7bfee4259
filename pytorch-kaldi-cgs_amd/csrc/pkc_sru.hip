// pkc_sru.hip — the Simple Recurrent Unit (Lei et al., "Simple Recurrent Units for Highly
// Parallelizable Recurrence", EMNLP 2018; the v2 cell with the highway scaling alpha): the time loop
// of a whole layer, both directions, as ONE launch.
//
// The SRU has no matrix product inside its recurrence: all weights act in the (T*B)-row projection
// U = X weight (a plain matmul, outside this file) and what stays serial is elementwise over T per
// (sentence b, column j).  So one thread owns a (b, j) pair and walks all T steps with its state
// c in a register; consecutive lanes own consecutive j, so every load and store of a wave is one
// contiguous run (k = 4: 16 bytes per lane).  The direction is a property of the column
// (j / d: 1 walks t = T-1 .. 0), so a bidirectional layer is the same launch.  No grid
// synchronisation, no co-residency condition, no per-step launches, for every shape.
//
// Few wavefronts exist at the sizes this runs at (B = 8, n_out = 1100: 138), so latency is hidden
// by instruction-level parallelism, not occupancy: none of the loads of a step (u, x, c for the
// backward, dy) depends on the carried state, so they are issued a block of UNR steps ahead of
// their use, the next block's loads in flight while the current block's serial chain runs.
//
// Backward: the same walk the other way with the carry dc; the gates are recomputed from u and
// c_{t-1} (nothing but c is saved).  d weight_c and d bias are summed over T in registers, the
// per-(b, j) sums go to `work`, and a second small kernel adds them over b in fixed order: no
// atomics anywhere, reruns are bit-identical, and a bidirectional call equals two one-direction
// calls bit for bit (a column's results depend on its own operands only).
#include "pkc_common.h"

namespace pkc {
namespace {

constexpr int UNR = 4;         // steps per block of loads in flight

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// g: identity, relu or tanh (the only activations of the cell)
__device__ __forceinline__ float g_fwd(int act, float c) {
  return act == PKC_ACT_TANH ? tanhf(c) : act == PKC_ACT_RELU ? (c > 0.f ? c : 0.f) : c;
}

struct Geo {
  int T, B, n_out, j, b, rev;
  __device__ __forceinline__ int time(int s) const { return rev ? T - 1 - s : s; }
  __device__ __forceinline__ int64_t col(int t) const {            // (T, B, n_out) element
    return ((int64_t)t * B + b) * n_out + j;
  }
};

__device__ __forceinline__ bool geo(const pkc_sru_args& a, Geo* g) {
  g->T = a.T; g->B = a.B; g->n_out = a.ndir * a.d;
  g->j = blockIdx.x * blockDim.x + threadIdx.x;
  g->b = blockIdx.y;
  g->rev = g->j >= a.d;
  return g->j < g->n_out;
}

template <int K>
__device__ __forceinline__ void load_u(const float* u, int64_t col, float* v) {
  if constexpr (K == 4) {
    const float4 q = *reinterpret_cast<const float4*>(u + col * 4);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = u[col * 3]; v[1] = u[col * 3 + 1]; v[2] = u[col * 3 + 2]; v[3] = 0.f;
  }
}

// the mask scale m_c[b, j] of this thread: keep / (1 - p) in training with p > 0, else 1
__device__ __forceinline__ float mask_c(const pkc_sru_args& a, const Geo& g, bool draw) {
  if (!(a.train && a.drop_p > 0.f)) return 1.f;
  const uint32_t e = (uint32_t)g.b * (uint32_t)g.n_out + (uint32_t)g.j;
  uint8_t k;
  if (!draw) {
    k = a.keep[e];
  } else {
    if (a.keep_in) {
      k = a.keep_in[e];
    } else {
      const uint32_t thr = (uint32_t)((double)(1.f - a.drop_p) * 4294967296.0);
      const int64_t step = a.step_ctr ? *a.step_ctr : 0;
      k = hash_drop(hash_seed(a.seed, (uint64_t)a.stream_id, (uint64_t)step), e) < thr;
    }
    a.keep[e] = k;
  }
  return k ? 1.f / (1.f - a.drop_p) : 0.f;
}

// ------------------------------------------------------------------------------- forward
struct FwdIn { float u[4]; float x; };

template <int K>
__device__ __forceinline__ void fwd_load(const pkc_sru_args& a, const Geo& g, int s0, bool hw,
                                         FwdIn* in) {
#pragma unroll
  for (int i = 0; i < UNR; ++i) {
    const int s = s0 + i < g.T ? s0 + i : g.T - 1;      // clamped: unconditional loads
    const int t = g.time(s);
    load_u<K>(a.u, g.col(t), in[i].u);
    in[i].x = hw ? a.x[((int64_t)t * g.B + g.b) * a.ldx + g.j] : 0.f;
  }
}

template <int K>
__global__ __launch_bounds__(64) void sru_fwd(pkc_sru_args a) {
  Geo g;
  if (!geo(a, &g)) return;
  const bool hw = K == 3 && a.skip;                      // highway term alpha * x
  const float vf = a.weight_c[g.j], vr = a.weight_c[g.n_out + g.j];
  const float bf = a.bias[g.j], br = a.bias[g.n_out + g.j];
  const float mc = mask_c(a, g, true);
  float c = 0.f;
  FwdIn cur[UNR], nxt[UNR];
  fwd_load<K>(a, g, 0, hw, cur);
  for (int s0 = 0; s0 < g.T; s0 += UNR) {
    fwd_load<K>(a, g, s0 + UNR, hw, nxt);          // (clamped past the end: never out of bounds)
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      if (s0 + i < g.T) {
        const float* u = cur[i].u;
        const float f = sigm(u[1] + vf * c + bf);
        const float r = sigm(u[2] + vr * c + br);
        c = f * c + (1.f - f) * u[0];
        const float xp = K == 4 ? u[3] : a.alpha * cur[i].x;
        const float h = r * g_fwd(a.act, c) * mc + (1.f - r) * xp;
        const int64_t o = g.col(g.time(s0 + i));
        a.cs[o] = c;
        a.y[o] = h;
      }
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i) cur[i] = nxt[i];
  }
}

// ------------------------------------------------------------------------------- backward
struct BwdIn { float u[4]; float x, c, cp, dy; };

// block of the steps s0, s0-1, .., s0-UNR+1 (the walk runs s = T-1 .. 0)
template <int K>
__device__ __forceinline__ void bwd_load(const pkc_sru_args& a, const Geo& g, int s0, bool hw,
                                         BwdIn* in) {
  const int ns = a.dy_nslab > 0 ? a.dy_nslab : 1;
#pragma unroll
  for (int i = 0; i < UNR; ++i) {
    const int s = s0 - i > 0 ? s0 - i : 0;
    const int t = g.time(s);
    const int64_t o = g.col(t);
    load_u<K>(a.u, o, in[i].u);
    in[i].x = hw ? a.x[((int64_t)t * g.B + g.b) * a.ldx + g.j] : 0.f;
    in[i].c = a.cs[o];
    const float cp = a.cs[g.col(g.time(s > 0 ? s - 1 : 0))];
    in[i].cp = s > 0 ? cp : 0.f;
    float dy = 0.f;
    for (int z = 0; z < ns; ++z) dy += a.dy[(int64_t)z * a.dy_slab_stride + o];
    in[i].dy = dy;
  }
}

template <int K>
__global__ __launch_bounds__(64) void sru_bwd(pkc_sru_args a) {
  Geo g;
  if (!geo(a, &g)) return;
  const bool hw = K == 3 && a.skip;
  const float vf = a.weight_c[g.j], vr = a.weight_c[g.n_out + g.j];
  const float bf = a.bias[g.j], br = a.bias[g.n_out + g.j];
  const float mc = mask_c(a, g, false);
  float dc = 0.f, dvf = 0.f, dvr = 0.f, dbf = 0.f, dbr = 0.f;
  BwdIn cur[UNR], nxt[UNR];
  bwd_load<K>(a, g, g.T - 1, hw, cur);
  for (int s0 = g.T - 1; s0 >= 0; s0 -= UNR) {
    bwd_load<K>(a, g, s0 - UNR, hw, nxt);          // (clamped past the end: never out of bounds)
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      if (s0 - i >= 0) {
        const BwdIn& q = cur[i];
        const float cp = q.cp, c = q.c, dh = q.dy;
        const float f = sigm(q.u[1] + vf * cp + bf);
        const float r = sigm(q.u[2] + vr * cp + br);
        float gc, gp;
        if (a.act == PKC_ACT_TANH) { gc = tanhf(c); gp = 1.f - gc * gc; }
        else if (a.act == PKC_ACT_RELU) { gc = c > 0.f ? c : 0.f; gp = c > 0.f ? 1.f : 0.f; }
        else { gc = c; gp = 1.f; }
        const float xp = K == 4 ? q.u[3] : a.alpha * q.x;
        const float dr = dh * (gc * mc - xp);
        const float dxp = dh * (1.f - r);
        dc += dh * r * mc * gp;
        const float du0 = dc * (1.f - f);
        const float daf = dc * (cp - q.u[0]) * f * (1.f - f);
        const float dar = dr * r * (1.f - r);
        dvf += daf * cp; dvr += dar * cp; dbf += daf; dbr += dar;
        dc = dc * f + daf * vf + dar * vr;
        const int64_t o = g.col(g.time(s0 - i));
        if constexpr (K == 4) {
          *reinterpret_cast<float4*>(a.du + o * 4) = make_float4(du0, daf, dar, dxp);
        } else {
          a.du[o * 3] = du0; a.du[o * 3 + 1] = daf; a.du[o * 3 + 2] = dar;
          if (hw) a.dxh[o] = a.alpha * dxp;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i) cur[i] = nxt[i];
  }
  float* w = a.work + (int64_t)g.b * 4 * g.n_out + g.j;          // (B, 4, n_out)
  w[0] = dvf; w[g.n_out] = dvr; w[2 * g.n_out] = dbf; w[3 * g.n_out] = dbr;
}

// [dv_f | dv_r] and [db_f | db_r]: the per-sentence sums of `work` added in b order
__global__ __launch_bounds__(256) void sru_reduce_b(pkc_sru_args a) {
  const int n_out = a.ndir * a.d;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;           // q * n_out + j, q < 4
  if (i >= 4 * n_out) return;
  float v = 0.f;
  for (int b = 0; b < a.B; ++b) v += a.work[(int64_t)b * 4 * n_out + i];
  if (i < 2 * n_out) a.dwc[i] = v;
  else a.dbias[i - 2 * n_out] = v;
}

// ------------------------------------------------------------------------------- input side
// xt = x * m_x with m_x[b, i] = keep / (1 - p), ONE mask for all t; keep (B, n_in) is written
__global__ __launch_bounds__(256) void sru_mask_x(int T, int B, int n_in, const float* x, int64_t ldx,
                                                  float drop_p, uint64_t seed, const int64_t* step_ctr,
                                                  int64_t stream_id, const uint8_t* keep_in,
                                                  uint8_t* keep, float* xt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)T * B * n_in) return;
  const int i = (int)(e % n_in);
  const int64_t row = e / n_in;
  const int b = (int)(row % B);
  const uint32_t m = (uint32_t)b * (uint32_t)n_in + (uint32_t)i;
  uint8_t k;
  if (keep_in) {
    k = keep_in[m];
  } else {
    const uint32_t thr = (uint32_t)((double)(1.f - drop_p) * 4294967296.0);
    const int64_t step = step_ctr ? *step_ctr : 0;
    k = hash_drop(hash_seed(seed, (uint64_t)stream_id, (uint64_t)step), m) < thr;
  }
  if (row < B) keep[m] = k;                                       // the t = 0 rows write the mask
  xt[e] = k ? x[row * ldx + i] * (1.f / (1.f - drop_p)) : 0.f;
}

// dx = m_x * sum_s slab_s + dxh, ONE slab
__global__ __launch_bounds__(256) void sru_dx(int64_t rows, int B, int n_in, const float* slabs,
                                              int nslab, int64_t slab_stride, const uint8_t* keep,
                                              float drop_p, const float* dxh, float* dx) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * n_in) return;
  float v = 0.f;
  for (int z = 0; z < nslab; ++z) v += slabs[(int64_t)z * slab_stride + e];
  if (keep) {
    const int i = (int)(e % n_in), b = (int)((e / n_in) % B);
    v = keep[(int64_t)b * n_in + i] ? v * (1.f / (1.f - drop_p)) : 0.f;
  }
  if (dxh) v += dxh[e];
  dx[e] = v;
}

int check(const pkc_sru_args* a, bool bwd, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  PKC_CHECK_ARG(a->T > 0 && a->B > 0 && a->d > 0, "%s: T=%d B=%d d=%d", who, a->T, a->B, a->d);
  PKC_CHECK_ARG(a->B <= 65535, "%s: B=%d > 65535", who, a->B);
  PKC_CHECK_ARG(a->ndir == 1 || a->ndir == 2, "%s: ndir=%d", who, a->ndir);
  PKC_CHECK_ARG(a->k == 3 || a->k == 4, "%s: k=%d (3 or 4)", who, a->k);
  const int64_t n_out = (int64_t)a->ndir * a->d;
  PKC_CHECK_ARG((int64_t)a->B * n_out < (int64_t)1 << 31 && (int64_t)a->T * a->B * n_out * 4 <
                (int64_t)1 << 40, "%s: T*B*n_out too large", who);
  PKC_CHECK_ARG(a->act == PKC_ACT_LINEAR || a->act == PKC_ACT_RELU || a->act == PKC_ACT_TANH,
                "%s: activation %d (linear, relu or tanh)", who, a->act);
  PKC_CHECK_ARG(a->k == 3 || a->skip, "%s: k=4 without the skip term", who);
  PKC_CHECK_ARG(!(a->k == 3 && a->skip) || a->n_in == n_out,
                "%s: k=3 with the skip term needs n_in == n_out (n_in=%d, n_out=%d)", who, a->n_in,
                (int)n_out);
  PKC_CHECK_ARG(!(a->k == 4) || a->n_in != n_out, "%s: k=4 with n_in == n_out = %d", who, (int)n_out);
  PKC_CHECK_ARG(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", who,
                (double)a->drop_p);
  PKC_CHECK_ARG(a->u && a->weight_c && a->bias && a->cs && a->y,
                "%s: null u / weight_c / bias / cs / y", who);
  PKC_CHECK_ARG(a->k == 3 || (reinterpret_cast<uintptr_t>(a->u) & 15) == 0,
                "%s: u is not 16-byte aligned", who);
  if (a->k == 3 && a->skip)
    PKC_CHECK_ARG(a->x && a->ldx >= n_out, "%s: null x or ldx=%lld < n_out (k=3 skip term)", who,
                  (long long)a->ldx);
  PKC_CHECK_ARG(!(a->train && a->drop_p > 0.f) || a->keep, "%s: null keep (dropout)", who);
  if (bwd) {
    PKC_CHECK_ARG(a->dy && a->du && a->dwc && a->dbias && a->work,
                  "%s: null dy / du / dwc / dbias / work", who);
    PKC_CHECK_ARG(a->k == 3 || (reinterpret_cast<uintptr_t>(a->du) & 15) == 0,
                  "%s: du is not 16-byte aligned", who);
    PKC_CHECK_ARG(!(a->k == 3 && a->skip) || a->dxh, "%s: null dxh (k=3 skip term)", who);
    PKC_CHECK_ARG(a->dy_nslab <= 1 || a->dy_slab_stride > 0, "%s: dy slab stride", who);
  }
  return PKC_OK;
}

}  // namespace
}  // namespace pkc

using namespace pkc;

extern "C" int pkc_sru_fwd(const pkc_sru_args* a, void* stream) {
  if (int e = check(a, false, "pkc_sru_fwd")) return e;
  const dim3 grid((a->ndir * a->d + 63) / 64, a->B);
  if (a->k == 4) hipLaunchKernelGGL(sru_fwd<4>, grid, dim3(64), 0, S(stream), *a);
  else hipLaunchKernelGGL(sru_fwd<3>, grid, dim3(64), 0, S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_sru_fwd");
  return PKC_OK;
}

extern "C" int pkc_sru_bwd(const pkc_sru_args* a, void* stream) {
  if (int e = check(a, true, "pkc_sru_bwd")) return e;
  const int n_out = a->ndir * a->d;
  const dim3 grid((n_out + 63) / 64, a->B);
  if (a->k == 4) hipLaunchKernelGGL(sru_bwd<4>, grid, dim3(64), 0, S(stream), *a);
  else hipLaunchKernelGGL(sru_bwd<3>, grid, dim3(64), 0, S(stream), *a);
  hipLaunchKernelGGL(sru_reduce_b, dim3((4 * n_out + 255) / 256), dim3(256), 0, S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_sru_bwd");
  return PKC_OK;
}

extern "C" int pkc_sru_mask_x(int T, int B, int n_in, const float* x, int64_t ldx, float drop_p,
                              uint64_t seed, const int64_t* step_ctr, int64_t stream_id,
                              const uint8_t* keep_in, uint8_t* keep, float* xt, void* stream) {
  PKC_CHECK_ARG(T > 0 && B > 0 && n_in > 0 && ldx >= n_in, "pkc_sru_mask_x: T=%d B=%d n_in=%d ldx=%lld",
                T, B, n_in, (long long)ldx);
  PKC_CHECK_ARG((int64_t)B * n_in < (int64_t)1 << 31 && (int64_t)T * B * n_in < (int64_t)1 << 38,
                "pkc_sru_mask_x: T*B*n_in too large");
  PKC_CHECK_ARG(drop_p > 0.f && drop_p < 1.f, "pkc_sru_mask_x: drop_p=%g outside (0, 1)",
                (double)drop_p);
  PKC_CHECK_ARG(x && keep && xt, "pkc_sru_mask_x: null x / keep / xt");
  const int64_t n = (int64_t)T * B * n_in;
  hipLaunchKernelGGL(sru_mask_x, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), T, B, n_in,
                     x, ldx, drop_p, seed, step_ctr, stream_id, keep_in, keep, xt);
  PKC_LAUNCH_CHECK("pkc_sru_mask_x");
  return PKC_OK;
}

extern "C" int pkc_sru_dx(int T, int B, int n_in, const float* slabs, int nslab, int64_t slab_stride,
                          const uint8_t* keep, float drop_p, const float* dxh, float* dx,
                          void* stream) {
  PKC_CHECK_ARG(T > 0 && B > 0 && n_in > 0, "pkc_sru_dx: T=%d B=%d n_in=%d", T, B, n_in);
  PKC_CHECK_ARG((int64_t)T * B * n_in < (int64_t)1 << 38, "pkc_sru_dx: T*B*n_in too large");
  PKC_CHECK_ARG(slabs && dx && nslab >= 1, "pkc_sru_dx: null slabs / dx or nslab=%d", nslab);
  PKC_CHECK_ARG(nslab == 1 || slab_stride > 0, "pkc_sru_dx: slab stride");
  PKC_CHECK_ARG(!keep || (drop_p > 0.f && drop_p < 1.f), "pkc_sru_dx: drop_p=%g outside (0, 1)",
                (double)drop_p);
  const int64_t n = (int64_t)T * B * n_in;
  hipLaunchKernelGGL(sru_dx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), (int64_t)T * B,
                     B, n_in, slabs, nslab, slab_stride, keep, drop_p, dxh, dx);
  PKC_LAUNCH_CHECK("pkc_sru_dx");
  return PKC_OK;
}
