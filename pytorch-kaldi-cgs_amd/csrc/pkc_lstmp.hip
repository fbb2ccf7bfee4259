// pkc_lstmp.hip — the time loops of the projected LSTM (LSTMP; Sak et al., Interspeech 2014):
// LSTM_cudnn with proj_size = P, i.e. torch.nn.LSTM(..., proj_size=P), 0 < P < H.
//
// The cell is the LSTM of pkc_rnn_std.hip up to h~_t = o tanh(c_t) (H wide); the layer output and
// the recurrent state are h_t = weight_hr h~_t (P wide, no bias).  weight_hh is (4H, P).  The two
// products of a step depend on each other, so a step is TWO launches of 16-row x 16-column tiles,
// both directions in blockIdx.z:
//   forward   lstmp_cell_step  U h_{t-1} over P (skipped at step 0) -> gates, cs, ht
//             lstmp_proj_step  weight_hr h~_t over H -> hs, and with the inter-layer dropout, y
//   backward  lstmp_bwd_hp     dhp_t = sum dy slabs (dropout applied) + dgates_{next} U over 4H
//             lstmp_bwd_cell   dh~_t = dhp_t weight_hr over P -> dgates_t and the dc f carry
// The waves of a workgroup (4; contraction >= 256: 8) split the contraction into contiguous strips
// per lane group, every lane streams its strip of one row of each operand into exact-fp32
// v_mfma_f32_16x16x4_f32 chains, the waves' partial tiles are summed in LDS in a fixed order.
// weight_hh . weight_hr is never folded into one (4H, H) matrix: that would undo the saving and
// change the rounding torch has.  No atomics, no waits: reruns are bit-identical, and a
// bidirectional run equals two uni-directional runs bit for bit.
#include "pkc_common.h"

#include <initializer_list>

namespace pkc {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// v[0..3] = row[k .. k+3] where ok and inside [0, kmax), else 0 (clamped, unconditional loads);
// VW: 4: 16-byte loads (kmax % 4 == 0 and 16-byte aligned rows, so a group is wholly in or out),
// 2: 8-byte pairs (kmax even, 8-byte aligned rows), 1: element loads
template <int VW>
__device__ __forceinline__ void load4(const float* row, bool ok, int k, int kmax, float* v) {
  if constexpr (VW == 4) {
    const bool in = ok && k < kmax;
    const float4 x = *reinterpret_cast<const float4*>(row + (in ? k : 0));
    v[0] = in ? x.x : 0.f; v[1] = in ? x.y : 0.f; v[2] = in ? x.z : 0.f; v[3] = in ? x.w : 0.f;
  } else if constexpr (VW == 2) {
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

// One lane's strip [kb, kb + S) of G products that share the A row: acc[g] += pa[k] * pb[g * gs + k]
// in k order.  An iteration issues the (unconditional, clamped) loads of D groups of 4 and then
// their MFMAs, so D * (1 + G) loads are in flight per wait; groups past the strip's end load
// nothing new and are skipped (a wave-uniform test), so the sum order is that of a plain k loop.
// The load width is a template parameter: the loop body has no branch on it.
template <int VW, int G, int D>
__device__ __forceinline__ void strip_dot(const float* pa, bool aok, const float* pb, bool bok,
                                          int64_t gs, int kb, int S, int K, f32x4* acc) {
  for (int s0 = 0; s0 < S; s0 += 4 * D) {
    float va[D][4], vb[D][G][4];
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const bool in = s0 + 4 * u < S;
      load4<VW>(pa, aok && in, kb + s0 + 4 * u, K, va[u]);
#pragma unroll
      for (int g = 0; g < G; ++g) load4<VW>(pb + g * gs, bok && in, kb + s0 + 4 * u, K, vb[u][g]);
    }
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (s0 + 4 * u < S) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int g = 0; g < G; ++g)
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[u][i], vb[u][g][i], acc[g], 0, 0, 0);
        }
      }
    }
  }
}
template <int G, int D>
__device__ __forceinline__ void strip_dot_vec(int vec, const float* pa, bool aok, const float* pb,
                                              bool bok, int64_t gs, int kb, int S, int K, f32x4* acc) {
  if (vec == 4) strip_dot<4, G, D>(pa, aok, pb, bok, gs, kb, S, K, acc);
  else if (vec == 2) strip_dot<2, G, D>(pa, aok, pb, bok, gs, kb, S, K, acc);
  else strip_dot<1, G, D>(pa, aok, pb, bok, gs, kb, S, K, acc);
}

// the finished element (rl, cl) of tile g: the NW waves' partial tiles in fixed order
template <int NW, int G>
__device__ __forceinline__ float red_sum(const float* red, int g, int rl, int cl) {
  const float* p = red + (g * 16 + rl) * RED_LD + cl;
  constexpr int S = G * 16 * RED_LD;
  float v = (p[0] + p[S]) + (p[2 * S] + p[3 * S]);
  if constexpr (NW == 8) v += (p[4 * S] + p[5 * S]) + (p[6 * S] + p[7 * S]);
  return v;
}

struct PIdx {
  int T, B, H, P, D;
  __device__ __forceinline__ int64_t hstate(int d, int slot, int r) const {   // (ndir, T+1, B, P) row
    return (((int64_t)d * (T + 1) + slot) * B + r) * P;
  }
  __device__ __forceinline__ int64_t cstate(int d, int slot, int r) const {   // (ndir, T+1, B, H) row
    return (((int64_t)d * (T + 1) + slot) * B + r) * H;
  }
  __device__ __forceinline__ int64_t row(int d, int tt, int r) const {        // (ndir, T, B) row
    return ((int64_t)d * T + tt) * B + r;
  }
  __device__ __forceinline__ int64_t out(int d, int tt, int r, int p) const { // (T, B, ndir*P)
    return ((int64_t)tt * B + r) * D + (int64_t)d * P + p;
  }
};
__device__ __forceinline__ PIdx mkidx(const pkc_lstmp_args& a) {
  PIdx x;
  x.T = a.T; x.B = a.B; x.H = a.H; x.P = a.P; x.D = a.ndir * a.P;
  return x;
}
// slots of the (T+1)-deep state arrays, as pkc_rnn_std_args: the forward direction keeps the state
// after time tt at tt + 1, the reverse direction at tt, so that the h_{t-1} rows of all T steps
// are T consecutive slots in natural time order (what the weight_hh gradient contracts with)
__device__ __forceinline__ int slot_prev(int d, int tt) { return d ? tt + 1 : tt; }
__device__ __forceinline__ int slot_out(int d, int tt) { return d ? tt : tt + 1; }

// ------------------------------------------------------------------------------- forward
// cell update of step s: direction d handles time tt = d ? T-1-s : s.  Tiles of 16 rows x 16 units
template <int NW>
__global__ __launch_bounds__(64 * NW) void lstmp_cell_step(pkc_lstmp_args a, int s, int vec) {
  __shared__ float red[NW * 4 * 16 * RED_LD];
  const PIdx ix = mkidx(a);
  const int H = a.H, B = a.B, P = a.P, d = blockIdx.z;
  const int tt = d ? a.T - 1 - s : s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int u0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const int sp = slot_prev(d, tt), so = slot_out(d, tt);
  if (s > 0) {
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int S = strip_of(P, NW);
    const int kb = (w * 4 + q) * S;
    const int ra = r0 + c, u = u0 + c;
    const bool rok = ra < B, uok = u < H;
    const float* ph = a.hs + ix.hstate(d, sp, rok ? ra : 0);
    const float* pu = a.U[d] + (int64_t)(uok ? u : 0) * P;
    strip_dot_vec<4, 2>(vec, ph, rok, pu, uok, (int64_t)H * P, kb, S, P, acc);
    // C layout: column lane & 15, rows 4 (lane >> 4) + i
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[((w * 4 + g) * 16 + 4 * q + i) * RED_LD + c] = acc[g][i];
    }
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, ul = threadIdx.x & 15;
  const int r = r0 + rl, j = u0 + ul;
  if (r >= B || j >= H) return;
  float up[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v = 0.f;
    if (s > 0) v = red_sum<NW, 4>(red, g, rl, ul);
    if (a.bhh[d]) v += a.bhh[d][g * H + j];
    up[g] = v;
  }
  const int64_t rw = ix.row(d, tt, r);
  const float* wp = a.wpre[d] + ((int64_t)tt * B + r) * (4 * H) + j;
  float* gt = a.gates + rw * (4 * H) + j;
  const int64_t ip = ix.cstate(d, sp, r) + j, io = ix.cstate(d, so, r) + j;
  float cp = 0.f;
  if (s > 0) cp = a.cs[ip];
  else a.cs[ip] = 0.f;
  const float ig = sigm(wp[0] + up[0]);
  const float fg = sigm(wp[H] + up[1]);
  const float gg = tanhf(wp[2 * H] + up[2]);
  const float og = sigm(wp[3 * H] + up[3]);
  const float cn = fg * cp + ig * gg;
  a.cs[io] = cn;
  gt[0] = ig; gt[H] = fg; gt[2 * H] = gg; gt[3 * H] = og;
  a.ht[rw * H + j] = og * tanhf(cn);
}

// projection of step s: h_t = weight_hr h~_t.  Tiles of 16 rows x 16 projected units
template <int NW>
__global__ __launch_bounds__(64 * NW) void lstmp_proj_step(pkc_lstmp_args a, int s, int vec) {
  __shared__ float red[NW * 16 * RED_LD];
  const PIdx ix = mkidx(a);
  const int H = a.H, B = a.B, P = a.P, d = blockIdx.z;
  const int tt = d ? a.T - 1 - s : s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int p0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int S = strip_of(H, NW);
    const int kb = (w * 4 + q) * S;
    const int ra = r0 + c, p = p0 + c;
    const bool rok = ra < B, pok = p < P;
    const float* pa = a.ht + ix.row(d, tt, rok ? ra : 0) * H;
    const float* pb = a.Whr[d] + (int64_t)(pok ? p : 0) * H;
    strip_dot_vec<1, 4>(vec, pa, rok, pb, pok, 0, kb, S, H, &acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(w * 16 + 4 * q + i) * RED_LD + c] = acc[i];
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, pl = threadIdx.x & 15;
  const int r = r0 + rl, p = p0 + pl;
  if (r >= B || p >= P) return;
  float h = red_sum<NW, 1>(red, 0, rl, pl);
  if (s == 0) a.hs[ix.hstate(d, slot_prev(d, tt), r) + p] = 0.f;   // the zero initial state, read
  a.hs[ix.hstate(d, slot_out(d, tt), r) + p] = h;                  // by the weight_hh gradient
  const int64_t oi = ix.out(d, tt, r, p);
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
// dst[d][c][r] = src[d][r][c] for a (rows, cols) matrix per direction: the B operands of the BPTT
__global__ __launch_bounds__(256) void lstmp_transpose(const float* s0, const float* s1, float* dst,
                                                       int rows, int cols) {
  __shared__ float tl[32][33];
  const int d = blockIdx.z;
  const float* src = d ? s1 : s0;
  float* out = dst + (int64_t)d * rows * cols;
  const int j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int j = j0 + i, k = k0 + tx;
    tl[i][tx] = (j < rows && k < cols) ? src[(int64_t)j * cols + k] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, j = j0 + tx;
    if (k < cols && j < rows) out[(int64_t)k * rows + j] = tl[tx][i];
  }
}

// (A) of BPTT step s (time tt): dhp = sum of the dy slabs (dropout applied) + dgates_{next step} U
// over the packed 4H contraction (not at the first BPTT step, s = T-1)
template <int NW>
__global__ __launch_bounds__(64 * NW) void lstmp_bwd_hp(pkc_lstmp_args a, int s, int vec) {
  __shared__ float red[NW * 16 * RED_LD];
  const PIdx ix = mkidx(a);
  const int H = a.H, B = a.B, P = a.P, T = a.T, d = blockIdx.z, GH = 4 * H;
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
    const bool rok = ra < B, kok = k < P;
    const float* pa = a.dgates + ix.row(d, tn, rok ? ra : 0) * GH;
    const float* pb = a.ut + ((int64_t)d * P + (kok ? k : 0)) * GH;
    strip_dot_vec<1, 8>(vec, pa, rok, pb, kok, 0, kb, S, GH, &acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(w * 16 + 4 * q + i) * RED_LD + c] = acc[i];
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, kl = threadIdx.x & 15;
  const int r = r0 + rl, k = k0 + kl;
  if (r >= B || k >= P) return;
  const int64_t oi = ix.out(d, tt, r, k);
  float g = 0.f;
  const int ns = a.dy_nslab > 0 ? a.dy_nslab : 1;
  for (int z = 0; z < ns; ++z) g += a.dy[(int64_t)z * a.dy_slab_stride + oi];
  if (a.train && a.drop_p > 0.f) g = a.keep[oi] ? g * (1.f / (1.f - a.drop_p)) : 0.f;
  if (rec) g += red_sum<NW, 1>(red, 0, rl, kl);
  a.dhp[ix.row(d, tt, r) * P + k] = g;
}

// (B) of BPTT step s: dh~ = dhp weight_hr over P, then the gate gradients of this step into dgates
// and the dc f carry of the next (earlier) step into work
template <int NW>
__global__ __launch_bounds__(64 * NW) void lstmp_bwd_cell(pkc_lstmp_args a, int s, int vec) {
  __shared__ float red[NW * 16 * RED_LD];
  const PIdx ix = mkidx(a);
  const int H = a.H, B = a.B, P = a.P, T = a.T, d = blockIdx.z;
  const int tt = d ? T - 1 - s : s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int j0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int S = strip_of(P, NW);
    const int kb = (w * 4 + q) * S;
    const int ra = r0 + c, j = j0 + c;
    const bool rok = ra < B, jok = j < H;
    const float* pa = a.dhp + ix.row(d, tt, rok ? ra : 0) * P;
    const float* pb = a.wt + ((int64_t)d * H + (jok ? j : 0)) * P;
    strip_dot_vec<1, 2>(vec, pa, rok, pb, jok, 0, kb, S, P, &acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(w * 16 + 4 * q + i) * RED_LD + c] = acc[i];
    __syncthreads();
  }
  if (threadIdx.x >= 256) return;
  const int rl = threadIdx.x >> 4, jl = threadIdx.x & 15;
  const int r = r0 + rl, j = j0 + jl;
  if (r >= B || j >= H) return;
  const float g = red_sum<NW, 1>(red, 0, rl, jl);
  float* carry = a.work + ((int64_t)d * B + r) * H + j;
  const int64_t rw = ix.row(d, tt, r);
  const float* gt = a.gates + rw * (4 * H) + j;
  float* dg = a.dgates + rw * (4 * H) + j;
  const float ig = gt[0], fg = gt[H], gg = gt[2 * H], og = gt[3 * H];
  const float cn = a.cs[ix.cstate(d, slot_out(d, tt), r) + j];
  const float cp = a.cs[ix.cstate(d, slot_prev(d, tt), r) + j];
  const float tc = tanhf(cn);
  float dc = g * og * (1.f - tc * tc);
  if (s < T - 1) dc += carry[0];                            // dc_{t+1} * f_{t+1}
  dg[0] = dc * gg * ig * (1.f - ig);
  dg[H] = dc * cp * fg * (1.f - fg);
  dg[2 * H] = dc * ig * (1.f - gg * gg);
  dg[3 * H] = g * tc * og * (1.f - og);
  carry[0] = dc * fg;
}

// 8 waves where a lane's strip of the contraction would otherwise exceed 16 elements
bool wide(int K) { return K >= 256; }

// widest load the strips take: every row starts a multiple of K floats after its base pointer
int load_width(int K, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  if (K % 4 == 0 && (bits & 15) == 0) return 4;
  if (K % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

int check(const pkc_lstmp_args* a, bool bwd, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  PKC_CHECK_ARG(a->T > 0 && a->B > 0 && a->H > 0, "%s: T=%d B=%d H=%d", who, a->T, a->B, a->H);
  PKC_CHECK_ARG(a->H <= 2048, "%s: H=%d > 2048", who, a->H);
  PKC_CHECK_ARG(a->P > 0 && a->P < a->H, "%s: P=%d outside (0, H=%d)", who, a->P, a->H);
  PKC_CHECK_ARG(a->ndir == 1 || a->ndir == 2, "%s: ndir=%d", who, a->ndir);
  PKC_CHECK_ARG((int64_t)a->T * a->B * 4 * a->H * a->ndir < (int64_t)1 << 40,
                "%s: T*B*H too large", who);
  PKC_CHECK_ARG(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: drop_p=%g outside [0, 1)", who,
                (double)a->drop_p);
  for (int d = 0; d < a->ndir; ++d)
    PKC_CHECK_ARG(a->wpre[d] && a->U[d] && a->Whr[d], "%s: null wpre / U / Whr of direction %d",
                  who, d);
  PKC_CHECK_ARG(a->hs && a->cs && a->gates && a->ht && a->y, "%s: null hs / cs / gates / ht / y", who);
  PKC_CHECK_ARG(!(a->train && a->drop_p > 0.f) || a->keep, "%s: null keep (dropout needs it)", who);
  if (bwd) {
    PKC_CHECK_ARG(a->dy && a->dgates && a->dhp && a->ut && a->wt && a->work,
                  "%s: null dy / dgates / dhp / ut / wt / work", who);
    PKC_CHECK_ARG(a->dy_nslab <= 1 || a->dy_slab_stride > 0, "%s: dy slab stride", who);
  }
  return PKC_OK;
}

#define LSTMP_LAUNCH(kern, K, grid, ...)                                                   \
  do {                                                                                     \
    if (wide(K)) hipLaunchKernelGGL((kern<8>), grid, dim3(512), 0, st, __VA_ARGS__);       \
    else hipLaunchKernelGGL((kern<4>), grid, dim3(256), 0, st, __VA_ARGS__);               \
  } while (0)

}  // namespace
}  // namespace pkc

using namespace pkc;

extern "C" int pkc_lstmp_fwd(const pkc_lstmp_args* a, void* stream) {
  if (int e = check(a, false, "pkc_lstmp_fwd")) return e;
  const int H = a->H, P = a->P, last = a->ndir - 1;
  const int vp = load_width(P, {a->hs, a->U[0], a->U[last]});
  const int vh = load_width(H, {a->ht, a->Whr[0], a->Whr[last]});
  hipStream_t st = S(stream);
  const dim3 gc((H + 15) / 16, (a->B + 15) / 16, a->ndir), gp((P + 15) / 16, (a->B + 15) / 16, a->ndir);
  for (int s = 0; s < a->T; ++s) {
    LSTMP_LAUNCH(lstmp_cell_step, P, gc, *a, s, vp);
    LSTMP_LAUNCH(lstmp_proj_step, H, gp, *a, s, vh);
  }
  PKC_LAUNCH_CHECK("pkc_lstmp_fwd step");
  return PKC_OK;
}

extern "C" int pkc_lstmp_bwd(const pkc_lstmp_args* a, void* stream) {
  if (int e = check(a, true, "pkc_lstmp_bwd")) return e;
  const int H = a->H, P = a->P, GH = 4 * a->H, last = a->ndir - 1;
  const int vg = load_width(GH, {a->dgates, a->ut});
  const int vp = load_width(P, {a->dhp, a->wt});
  hipStream_t st = S(stream);
  // ut[d][k][jj] = U[d][jj][k] (P, 4H);  wt[d][j][p] = Whr[d][p][j] (H, P)
  hipLaunchKernelGGL(lstmp_transpose, dim3((P + 31) / 32, (GH + 31) / 32, a->ndir), dim3(256), 0, st,
                     a->U[0], a->U[last], a->ut, GH, P);
  hipLaunchKernelGGL(lstmp_transpose, dim3((H + 31) / 32, (P + 31) / 32, a->ndir), dim3(256), 0, st,
                     a->Whr[0], a->Whr[last], a->wt, P, H);
  const dim3 ga((P + 15) / 16, (a->B + 15) / 16, a->ndir), gb((H + 15) / 16, (a->B + 15) / 16, a->ndir);
  for (int s = a->T - 1; s >= 0; --s) {
    LSTMP_LAUNCH(lstmp_bwd_hp, GH, ga, *a, s, vg);
    LSTMP_LAUNCH(lstmp_bwd_cell, P, gb, *a, s, vp);
  }
  PKC_LAUNCH_CHECK("pkc_lstmp_bwd step");
  return PKC_OK;
}
