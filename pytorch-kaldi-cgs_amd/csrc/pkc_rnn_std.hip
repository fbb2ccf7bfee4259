// pkc_rnn_std.hip — the time loops of the standard-cell recurrent layers: the reference's LSTM_cudnn,
// GRU_cudnn and RNN_cudnn (neural_networks.py:364-465), i.e. torch.nn.LSTM / GRU / RNN.
//
// What differs from the cells of pkc_rnn_impl.h:
//   * each direction of a bidirectional layer has its own weights (weight_ih/_hh/bias_*_l{k}_reverse),
//     so the directions are separate operands: direction d is blockIdx.z of every step launch, reads
//     its own pre-activations, its own weight_hh and its own time index (t or T-1-t) and writes its
//     half of the (T, B, ndir*H) output.  A 16-row tile holds rows of one direction only;
//   * weights are packed as torch packs them, (G*H, H) with gate rows i,f,g,o (LSTM) / r,z,n (GRU),
//     and the pre-activations are the one packed projection's output, (T, B, G*H);
//   * the GRU is torch's cell, n = tanh(a_n + r * (U_n h + b_hn)): all three recurrent products read
//     h_{t-1}, so a step is ONE launch (three accumulators per wave over one read of h_{t-1});
//   * no BatchNorm, no recurrent dropout; inverted dropout acts on the layer OUTPUT (between
//     layers) and is fused into the step epilogue's write of y and the BPTT's read of dy.
//
// A step is one launch of 16-row x 16-unit tiles; the 4 (H >= 512: 8) waves of a workgroup split
// the contraction into contiguous strips per lane group, every lane streams its strip of one
// h_{t-1} row and of one weight row per gate into exact-fp32 v_mfma_f32_16x16x4_f32 chains, the
// waves' partial tiles are summed in LDS in a fixed order and the cell update runs on the finished
// tile.  BPTT: dh_{t-1} = dR_t U over the packed G*H contraction (B operand from a transposed copy
// made once per pass), with the gate gradients of step t-1 in the same launch's epilogue.  No
// atomics anywhere: reruns are bit-identical, and a bidirectional run equals two uni-directional
// runs bit for bit.
#include "pkc_common.h"

#include <initializer_list>

namespace pkc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int std_gates(int cell) {
  return cell == PKC_STD_LSTM ? 4 : cell == PKC_STD_GRU ? 3 : 1;
}
// gate-gradient slabs per row: the GRU keeps the recurrent-side gradient of n (r * da_n) beside
// the input-side one (da_n): [r, z, n_rec, n_in]
__host__ __device__ constexpr int std_dgates(int cell) { return cell == PKC_STD_GRU ? 4 : std_gates(cell); }

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// v[0..3] = row[k .. k+3] where ok and inside [0, kmax), else 0 (clamped, unconditional loads);
// vw: 4: 16-byte loads (kmax % 4 == 0 and 16-byte aligned rows, so a group is wholly in or out),
// 2: 8-byte pairs (kmax even, 8-byte aligned rows: H = 550), 1: element loads
__device__ __forceinline__ void load4(const float* row, bool ok, int k, int kmax, int vw, float* v) {
  if (vw == 4) {
    const bool in = ok && k < kmax;
    const float4 x = *reinterpret_cast<const float4*>(row + (in ? k : 0));
    v[0] = in ? x.x : 0.f; v[1] = in ? x.y : 0.f; v[2] = in ? x.z : 0.f; v[3] = in ? x.w : 0.f;
  } else if (vw == 2) {
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      const bool in = ok && k + i < kmax;
      const float2 x = *reinterpret_cast<const float2*>(row + (in ? k + i : 0));
      v[i] = in ? x.x : 0.f; v[i + 1] = in ? x.y : 0.f;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool in = ok && k + i < kmax;
      const float x = row[in ? k + i : 0];
      v[i] = in ? x : 0.f;
    }
  }
}

// per-lane strip of a contraction of length K split over 4 * NW lane groups (a multiple of 4)
__host__ __device__ constexpr int strip_of(int K, int NW) {
  return ((K + 4 * NW - 1) / (4 * NW) + 3) / 4 * 4;
}

constexpr int RED_LD = 17;     // padded row of the 16 x 16 partial tiles in LDS

struct StdIdx {
  int T, B, H, D, G, GD;
  int64_t BH;
  __device__ __forceinline__ int64_t state(int d, int slot, int r, int j) const {   // (ndir, T+1, B, H)
    return ((int64_t)d * (T + 1) + slot) * BH + (int64_t)r * H + j;
  }
  __device__ __forceinline__ int64_t row(int d, int tt, int r) const {              // (ndir, T, B) row
    return ((int64_t)d * T + tt) * B + r;
  }
  __device__ __forceinline__ int64_t out(int d, int tt, int r, int j) const {       // (T, B, ndir*H)
    return ((int64_t)tt * B + r) * D + (int64_t)d * H + j;
  }
};
__device__ __forceinline__ StdIdx mkidx(const pkc_rnn_std_args& a) {
  StdIdx x;
  x.T = a.T; x.B = a.B; x.H = a.H; x.D = a.ndir * a.H;
  x.G = std_gates(a.cell); x.GD = std_dgates(a.cell);
  x.BH = (int64_t)a.B * a.H;
  return x;
}
// slots of the (T+1)-deep state arrays: the forward direction keeps the state after time tt at
// tt + 1 (h_{t-1} at tt), the reverse direction at tt (its h_{t-1}, the state after tt + 1, at
// tt + 1): in both, the h_{t-1} rows of all T steps are T consecutive slots in natural time order,
// which is what the weight_hh gradient matmul contracts with the (natural-time) gate gradients
__device__ __forceinline__ int slot_prev(int d, int tt) { return d ? tt + 1 : tt; }
__device__ __forceinline__ int slot_out(int d, int tt) { return d ? tt : tt + 1; }

// ------------------------------------------------------------------------------- forward step
// step s of both directions: direction d handles time tt = d ? T-1-s : s
template <int CELL, int NW>
__global__ __launch_bounds__(64 * NW) void std_fwd_step(pkc_rnn_std_args a, int s, int vec) {
  constexpr int G = std_gates(CELL);
  __shared__ float red[NW * G * 16 * RED_LD];
  const StdIdx ix = mkidx(a);
  const int H = a.H, B = a.B, d = blockIdx.z;
  const int tt = d ? a.T - 1 - s : s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int u0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const int sp = slot_prev(d, tt), so = slot_out(d, tt);
  if (s > 0) {
    f32x4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int S = strip_of(H, NW);
    const int kb = (w * 4 + q) * S;
    const int ra = r0 + c, u = u0 + c;
    const bool rok = ra < B, uok = u < H;
    const float* ph = a.hs + ix.state(d, sp, rok ? ra : 0, 0);
    const float* pu = a.U[d] + (int64_t)(uok ? u : 0) * H;
    for (int s0 = 0; s0 < S; s0 += 4) {
      float va[4], vu[G][4];
      load4(ph, rok, kb + s0, H, vec, va);
#pragma unroll
      for (int g = 0; g < G; ++g) load4(pu + (int64_t)g * H * H, uok, kb + s0, H, vec, vu[g]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int g = 0; g < G; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[i], vu[g][i], acc[g], 0, 0, 0);
      }
    }
    // C layout: column lane & 15, rows 4 (lane >> 4) + i
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[((w * G + g) * 16 + 4 * q + i) * RED_LD + c] = acc[g][i];
    }
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, ul = threadIdx.x & 15;
  const int r = r0 + rl, j = u0 + ul;
  if (r >= B || j >= H) return;
  float up[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float v = 0.f;
    if (s > 0) {
      const float* p = red + (g * 16 + rl) * RED_LD + ul;
      constexpr int P = G * 16 * RED_LD;
      v = (p[0] + p[P]) + (p[2 * P] + p[3 * P]);
      if constexpr (NW == 8) v += (p[4 * P] + p[5 * P]) + (p[6 * P] + p[7 * P]);
    }
    if (a.bhh[d]) v += a.bhh[d][g * H + j];
    up[g] = v;
  }
  const int64_t rw = ix.row(d, tt, r);
  const float* wp = a.wpre[d] + ((int64_t)tt * B + r) * (G * H) + j;
  float* gt = a.gates + rw * (G * H) + j;
  const int64_t ip = ix.state(d, sp, r, j), io = ix.state(d, so, r, j);
  float hp = 0.f;
  if (s > 0) hp = a.hs[ip];
  else a.hs[ip] = 0.f;               // the zero initial state, read by the weight_hh gradient
  float h;
  if constexpr (CELL == PKC_STD_LSTM) {
    float cp = 0.f;
    if (s > 0) cp = a.cs[ip];
    else a.cs[ip] = 0.f;
    const float ig = sigm(wp[0] + up[0]);
    const float fg = sigm(wp[H] + up[1]);
    const float gg = tanhf(wp[2 * H] + up[2]);
    const float og = sigm(wp[3 * H] + up[3]);
    const float cn = fg * cp + ig * gg;
    h = og * tanhf(cn);
    a.cs[io] = cn;
    gt[0] = ig; gt[H] = fg; gt[2 * H] = gg; gt[3 * H] = og;
  } else if constexpr (CELL == PKC_STD_GRU) {
    const float rg = sigm(wp[0] + up[0]);
    const float zg = sigm(wp[H] + up[1]);
    const float ng = tanhf(wp[2 * H] + rg * up[2]);
    h = (1.f - zg) * ng + zg * hp;
    a.un[rw * H + j] = up[2];
    gt[0] = rg; gt[H] = zg; gt[2 * H] = ng;
  } else {
    h = act_fwd(a.act, wp[0] + up[0]);
  }
  a.hs[io] = h;
  const int64_t oi = ix.out(d, tt, r, j);
  if (a.train && a.drop_p > 0.f) {
    uint8_t k;
    if (a.keep_in) {
      k = a.keep_in[oi];
    } else {
      const uint32_t thr = (uint32_t)((double)(1.f - a.drop_p) * 4294967296.0);
      const int64_t step = a.step_ctr ? *a.step_ctr : 0;
      k = hash_drop(hash_seed(a.seed, (uint64_t)a.stream_id, (uint64_t)step), (uint32_t)oi) < thr;
    }
    a.keep[oi] = k;
    h = k ? h * (1.f / (1.f - a.drop_p)) : 0.f;
  }
  a.y[oi] = h;
}

// ------------------------------------------------------------------------------- backward
// ut[d][k][jj] = U[d][jj][k], jj < G*H: the B operand of the BPTT products
__global__ __launch_bounds__(256) void std_transpose_u(pkc_rnn_std_args a) {
  __shared__ float tl[32][33];
  const int H = a.H, GH = std_gates(a.cell) * a.H, d = blockIdx.z;
  const float* U = a.U[d];
  float* ut = a.ut + (int64_t)d * H * GH;
  const int j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i, k = k0 + tx;
    tl[i][tx] = (j < GH && k < H) ? U[(int64_t)j * H + k] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, j = j0 + tx;
    if (k < H && j < GH) ut[(int64_t)k * GH + j] = tl[tx][i];
  }
}

// BPTT of step s (time tt): dh = dR_{next step} U (s < T-1), g = dL/dy_tt + dh + carry, then the
// gate gradients of this step into dgates and the carries of the next (earlier) step into work
template <int CELL, int NW>
__global__ __launch_bounds__(64 * NW) void std_bwd_step(pkc_rnn_std_args a, int s, int vec) {
  constexpr int G = std_gates(CELL), GD = std_dgates(CELL);
  __shared__ float red[NW * 16 * RED_LD];
  const StdIdx ix = mkidx(a);
  const int H = a.H, B = a.B, T = a.T, d = blockIdx.z, GH = G * H;
  const int tt = d ? T - 1 - s : s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const bool rec = s < T - 1;
  if (rec) {
    const int tn = d ? tt - 1 : tt + 1;            // the time of step s + 1
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int S = strip_of(GH, NW);
    const int kb = (w * 4 + q) * S;
    const int ra = r0 + c, k = k0 + c;
    const bool rok = ra < B, kok = k < H;
    const float* pa = a.dgates + ix.row(d, tn, rok ? ra : 0) * (GD * H);
    const float* pb = a.ut + ((int64_t)d * H + (kok ? k : 0)) * GH;
    for (int s0 = 0; s0 < S; s0 += 4) {
      float va[4], vb[4];
      load4(pa, rok, kb + s0, GH, vec, va);
      load4(pb, kok, kb + s0, GH, vec, vb);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[i], vb[i], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(w * 16 + 4 * q + i) * RED_LD + c] = acc[i];
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, kl = threadIdx.x & 15;
  const int r = r0 + rl, k = k0 + kl;
  if (r >= B || k >= H) return;
  float* carry = a.work + (int64_t)d * 2 * ix.BH + (int64_t)r * H + k;
  const int64_t oi = ix.out(d, tt, r, k);
  float g = 0.f;
  {
    const int ns = a.dy_nslab > 0 ? a.dy_nslab : 1;
    for (int z = 0; z < ns; ++z) g += a.dy[(int64_t)z * a.dy_slab_stride + oi];
    if (a.train && a.drop_p > 0.f) g = a.keep[oi] ? g * (1.f / (1.f - a.drop_p)) : 0.f;
  }
  if (rec) {
    const float* p = red + rl * RED_LD + kl;
    constexpr int P = 16 * RED_LD;
    float v = (p[0] + p[P]) + (p[2 * P] + p[3 * P]);
    if constexpr (NW == 8) v += (p[4 * P] + p[5 * P]) + (p[6 * P] + p[7 * P]);
    g += v;
    if constexpr (CELL == PKC_STD_GRU) g += carry[0];      // z_{t+1} * g_{t+1}
  }
  const int64_t rw = ix.row(d, tt, r);
  const float* gt = a.gates + rw * GH + k;
  float* dg = a.dgates + rw * (GD * H) + k;
  const int64_t ip = ix.state(d, slot_prev(d, tt), r, k), io = ix.state(d, slot_out(d, tt), r, k);
  if constexpr (CELL == PKC_STD_LSTM) {
    const float ig = gt[0], fg = gt[H], gg = gt[2 * H], og = gt[3 * H];
    const float cn = a.cs[io], cp = a.cs[ip];
    const float tc = tanhf(cn);
    float dc = g * og * (1.f - tc * tc);
    if (rec) dc += carry[ix.BH];                            // dc_{t+1} * f_{t+1}
    dg[0] = dc * gg * ig * (1.f - ig);
    dg[H] = dc * cp * fg * (1.f - fg);
    dg[2 * H] = dc * ig * (1.f - gg * gg);
    dg[3 * H] = g * tc * og * (1.f - og);
    carry[ix.BH] = dc * fg;
  } else if constexpr (CELL == PKC_STD_GRU) {
    const float rg = gt[0], zg = gt[H], ng = gt[2 * H];
    const float hp = a.hs[ip], un = a.un[rw * H + k];
    const float dan = g * (1.f - zg) * (1.f - ng * ng);
    dg[0] = dan * un * rg * (1.f - rg);
    dg[H] = g * (hp - ng) * zg * (1.f - zg);
    dg[2 * H] = rg * dan;                                   // recurrent side: dU_n, db_hn, dh_{t-1}
    dg[3 * H] = dan;                                        // input side: dW_in, db_in, dx
    carry[0] = g * zg;
  } else {
    dg[0] = g * act_bwd_out(a.act, a.hs[io]);
  }
}

template <int CELL>
int fwd_loop(const pkc_rnn_std_args* a, int vec, hipStream_t st) {
  const dim3 grid((a->H + 15) / 16, (a->B + 15) / 16, a->ndir);
  for (int s = 0; s < a->T; ++s) {
    if (a->H >= 512) hipLaunchKernelGGL((std_fwd_step<CELL, 8>), grid, dim3(512), 0, st, *a, s, vec);
    else hipLaunchKernelGGL((std_fwd_step<CELL, 4>), grid, dim3(256), 0, st, *a, s, vec);
  }
  PKC_LAUNCH_CHECK("pkc_rnn_std_fwd step");
  return PKC_OK;
}

template <int CELL>
int bwd_loop(const pkc_rnn_std_args* a, int vec, hipStream_t st) {
  const int GH = std_gates(CELL) * a->H;
  const dim3 tg((a->H + 31) / 32, (GH + 31) / 32, a->ndir);
  hipLaunchKernelGGL(std_transpose_u, tg, dim3(256), 0, st, *a);
  const dim3 grid((a->H + 15) / 16, (a->B + 15) / 16, a->ndir);
  for (int s = a->T - 1; s >= 0; --s) {
    if (GH >= 1024) hipLaunchKernelGGL((std_bwd_step<CELL, 8>), grid, dim3(512), 0, st, *a, s, vec);
    else hipLaunchKernelGGL((std_bwd_step<CELL, 4>), grid, dim3(256), 0, st, *a, s, vec);
  }
  PKC_LAUNCH_CHECK("pkc_rnn_std_bwd step");
  return PKC_OK;
}

// widest load the strips take: every row starts a multiple of H floats after its base pointer
int load_width(int H, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  if (H % 4 == 0 && (bits & 15) == 0) return 4;
  if (H % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

int check(const pkc_rnn_std_args* a, bool bwd, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  PKC_CHECK_ARG(a->cell == PKC_STD_LSTM || a->cell == PKC_STD_GRU || a->cell == PKC_STD_RNN,
                "%s: cell %d", who, a->cell);
  PKC_CHECK_ARG(a->T > 0 && a->B > 0 && a->H > 0, "%s: T=%d B=%d H=%d", who, a->T, a->B, a->H);
  PKC_CHECK_ARG(a->H <= 2048, "%s: H=%d > 2048", who, a->H);
  PKC_CHECK_ARG(a->ndir == 1 || a->ndir == 2, "%s: ndir=%d", who, a->ndir);
  PKC_CHECK_ARG((int64_t)a->T * a->B * std_dgates(a->cell) * a->H * a->ndir < (int64_t)1 << 40,
                "%s: T*B*H too large", who);
  PKC_CHECK_ARG(a->cell != PKC_STD_RNN || a->act == PKC_ACT_TANH || a->act == PKC_ACT_RELU,
                "%s: RNN nonlinearity %d (tanh or relu)", who, a->act);
  PKC_CHECK_ARG(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", who,
                (double)a->drop_p);
  for (int d = 0; d < a->ndir; ++d)
    PKC_CHECK_ARG(a->wpre[d] && a->U[d], "%s: null wpre / U of direction %d", who, d);
  PKC_CHECK_ARG(a->hs && a->gates && a->y, "%s: null hs / gates / y", who);
  PKC_CHECK_ARG(a->cell != PKC_STD_LSTM || a->cs, "%s: LSTM needs cs", who);
  PKC_CHECK_ARG(a->cell != PKC_STD_GRU || a->un, "%s: GRU needs un", who);
  PKC_CHECK_ARG(!(a->train && a->drop_p > 0.f) || a->keep, "%s: dropout needs keep", who);
  if (bwd) {
    PKC_CHECK_ARG(a->dy && a->dgates && a->ut && a->work, "%s: null dy / dgates / ut / work", who);
    PKC_CHECK_ARG(a->dy_nslab <= 1 || a->dy_slab_stride > 0, "%s: dy slab stride", who);
  }
  return PKC_OK;
}

}  // namespace
}  // namespace pkc

using namespace pkc;

extern "C" int pkc_rnn_std_fwd(const pkc_rnn_std_args* a, void* stream) {
  if (int e = check(a, false, "pkc_rnn_std_fwd")) return e;
  const int vec = load_width(a->H, {a->hs, a->U[0], a->U[a->ndir - 1]});
  hipStream_t st = S(stream);
  switch (a->cell) {
    case PKC_STD_LSTM: return fwd_loop<PKC_STD_LSTM>(a, vec, st);
    case PKC_STD_GRU: return fwd_loop<PKC_STD_GRU>(a, vec, st);
    default: return fwd_loop<PKC_STD_RNN>(a, vec, st);
  }
}

extern "C" int pkc_rnn_std_bwd(const pkc_rnn_std_args* a, void* stream) {
  if (int e = check(a, true, "pkc_rnn_std_bwd")) return e;
  const int vec = load_width(a->H, {a->dgates, a->ut});
  hipStream_t st = S(stream);
  switch (a->cell) {
    case PKC_STD_LSTM: return bwd_loop<PKC_STD_LSTM>(a, vec, st);
    case PKC_STD_GRU: return bwd_loop<PKC_STD_GRU>(a, vec, st);
    default: return bwd_loop<PKC_STD_RNN>(a, vec, st);
  }
}
