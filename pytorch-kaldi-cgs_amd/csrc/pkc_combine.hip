// pkc — the [model] tensor operations on produced outputs (utils.py:2014-2043: concatenate, mult,
// sum, mult_constant, sum_constant, avg) as one elementwise launch forward and one backward.
//
// Memory-bound streams: every thread moves one 16-byte group (float4) when every pointer, leading
// dimension, slab stride and width allows it, one float otherwise; both forms do the same fp32
// operations in the same order, so their results are bit-identical.  No atomics, no reductions
// across threads: reruns are bit-identical.
#include "pkc_common.h"

// one rounding per stated operation: nothing here may be contracted into an fma
#pragma clang fp contract(off)

namespace pkc {

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

template <int V>
__device__ __forceinline__ void cb_load(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void cb_store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}
template <int V>
__device__ __forceinline__ void cb_store_bf16(__bf16* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    bf16x4_t h;
    h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
    *reinterpret_cast<bf16x4_t*>(p) = h;
  } else {
    *p = (__bf16)v[0];
  }
}

// (row, first column) of work item i of a matrix with nv items per row; 32-bit division whenever
// the item count allows it
__device__ __forceinline__ void cb_rc(size_t i, size_t nv, bool small, size_t* r, int* cv) {
  if (small) {
    const uint32_t q = (uint32_t)i / (uint32_t)nv;
    *r = q;
    *cv = (int)((uint32_t)i - q * (uint32_t)nv);
  } else {
    const size_t q = i / nv;
    *r = q;
    *cv = (int)(i - q * nv);
  }
}

template <int V>
__global__ void __launch_bounds__(256) combine_fwd_kernel(pkc_combine_args a) {
  const int N = a.op == PKC_COMBINE_CONCAT ? a.Na + a.Nb : a.Na;
  const size_t nv = (size_t)(N / V), total = (size_t)a.M * nv;
  const bool small = total <= 0xffffffffull;
  __bf16* oh = reinterpret_cast<__bf16*>(a.out_bf16);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    size_t r;
    int cv;
    cb_rc(i, nv, small, &r, &cv);
    const int c = cv * V;
    float x[V], y[V], o[V];
    if (a.op == PKC_COMBINE_CONCAT) {
      if (c < a.Na) cb_load<V>(a.a + r * (size_t)a.lda + c, o);
      else cb_load<V>(a.b + r * (size_t)a.ldb + (c - a.Na), o);
    } else {
      cb_load<V>(a.a + r * (size_t)a.lda + c, x);
      if (a.op <= PKC_COMBINE_AVG) cb_load<V>(a.b + r * (size_t)a.ldb + c, y);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        switch (a.op) {
          case PKC_COMBINE_SUM: o[k] = x[k] + y[k]; break;
          case PKC_COMBINE_MULT: o[k] = x[k] * y[k]; break;
          case PKC_COMBINE_AVG: { const float t = x[k] + y[k]; o[k] = t * 0.5f; break; }
          case PKC_COMBINE_SUM_CONST: o[k] = x[k] + a.c; break;
          default: o[k] = x[k] * a.c; break;
        }
      }
    }
    const size_t at = r * (size_t)N + c;
    cb_store<V>(a.out + at, o);
    if (oh) cb_store_bf16<V>(oh + at, o);
  }
}

template <int V>
__global__ void __launch_bounds__(256) combine_bwd_kernel(pkc_combine_args a) {
  const int N = a.op == PKC_COMBINE_CONCAT ? a.Na + a.Nb : a.Na;
  const size_t nv = (size_t)(N / V), total = (size_t)a.M * nv;
  const bool small = total <= 0xffffffffull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    size_t r;
    int cv;
    cb_rc(i, nv, small, &r, &cv);
    const int c = cv * V;
    const size_t at = r * (size_t)N + c;
    float g[V], t[V], o[V];
    cb_load<V>(a.gslab + at, g);
    for (int s = 1; s < a.nslab; ++s) {           // slab order, left to right
      cb_load<V>(a.gslab + (size_t)s * (size_t)a.slab_stride + at, t);
#pragma unroll
      for (int k = 0; k < V; ++k) g[k] = g[k] + t[k];
    }
    switch (a.op) {
      case PKC_COMBINE_CONCAT:
        if (c < a.Na) {
          if (a.da) cb_store<V>(a.da + r * (size_t)a.Na + c, g);
        } else if (a.db) {
          cb_store<V>(a.db + r * (size_t)a.Nb + (c - a.Na), g);
        }
        break;
      case PKC_COMBINE_SUM:
      case PKC_COMBINE_SUM_CONST:
        if (a.da) cb_store<V>(a.da + at, g);
        if (a.db) cb_store<V>(a.db + at, g);
        break;
      case PKC_COMBINE_AVG:
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = g[k] * 0.5f;
        if (a.da) cb_store<V>(a.da + at, o);
        if (a.db) cb_store<V>(a.db + at, o);
        break;
      case PKC_COMBINE_MULT:
        if (a.da) {
          cb_load<V>(a.b + r * (size_t)a.ldb + c, t);
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = g[k] * t[k];
          cb_store<V>(a.da + at, o);
        }
        if (a.db) {
          cb_load<V>(a.a + r * (size_t)a.lda + c, t);
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = g[k] * t[k];
          cb_store<V>(a.db + at, o);
        }
        break;
      default:                                    // PKC_COMBINE_MULT_CONST
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = g[k] * a.c;
        if (a.da) cb_store<V>(a.da + at, o);
        break;
    }
  }
}

static inline bool cb_al(const void* p) { return ((uintptr_t)p % 16) == 0; }
static inline bool cb_binary(int op) { return op <= PKC_COMBINE_AVG; }

// argument checks shared by pkc_combine_ok and the entry points (0: fine, error string set else)
static int combine_check(const pkc_combine_args* a, bool bwd, const char* who) {
  PKC_CHECK_ARG(a, "%s: null arguments", who);
  PKC_CHECK_ARG(a->op >= PKC_COMBINE_CONCAT && a->op <= PKC_COMBINE_MULT_CONST,
                "%s: unknown operation %d", who, a->op);
  PKC_CHECK_ARG(a->M >= 1 && a->Na >= 1, "%s: M = %d, Na = %d (both >= 1)", who, a->M, a->Na);
  if (cb_binary(a->op)) {
    PKC_CHECK_ARG(a->Nb >= 1, "%s: Nb = %d (>= 1)", who, a->Nb);
    PKC_CHECK_ARG(a->op == PKC_COMBINE_CONCAT || a->Na == a->Nb,
                  "%s: operand widths %d and %d differ", who, a->Na, a->Nb);
    PKC_CHECK_ARG((int64_t)a->Na + a->Nb <= 0x7fffffff, "%s: concatenated width overflows", who);
  } else {
    PKC_CHECK_ARG(a->Nb == 0 || a->Nb == a->Na,
                  "%s: Nb = %d beside Na = %d for a constant operand", who, a->Nb, a->Na);
  }
  // which operands the pass reads
  const bool rd_a = !bwd || (a->op == PKC_COMBINE_MULT && a->db);
  const bool rd_b = cb_binary(a->op) && (!bwd || (a->op == PKC_COMBINE_MULT && a->da));
  PKC_CHECK_ARG(!rd_a || (a->a && a->lda >= a->Na), "%s: null a or lda %lld below Na = %d", who,
                (long long)a->lda, a->Na);
  PKC_CHECK_ARG(!rd_b || (a->b && a->ldb >= a->Nb), "%s: null b or ldb %lld below Nb = %d", who,
                (long long)a->ldb, a->Nb);
  if (!bwd) {
    PKC_CHECK_ARG(a->out, "%s: null out", who);
    return PKC_OK;
  }
  const int N = a->op == PKC_COMBINE_CONCAT ? a->Na + a->Nb : a->Na;
  PKC_CHECK_ARG(a->nslab >= 1, "%s: nslab = %d (>= 1)", who, a->nslab);
  PKC_CHECK_ARG(a->gslab, "%s: null gslab", who);
  PKC_CHECK_ARG(a->nslab == 1 || a->slab_stride >= (int64_t)a->M * N,
                "%s: slab_stride %lld below M * N = %lld", who, (long long)a->slab_stride,
                (long long)a->M * N);
  PKC_CHECK_ARG(a->da || a->db, "%s: both da and db null", who);
  PKC_CHECK_ARG(cb_binary(a->op) || (a->da && !a->db),
                "%s: a constant operand takes da only", who);
  return PKC_OK;
}

static bool combine_vec(const pkc_combine_args* a, bool bwd) {
  const bool cat = a->op == PKC_COMBINE_CONCAT, bin = cb_binary(a->op);
  if (a->Na % 4 || (cat && a->Nb % 4)) return false;
  if (!bwd)
    return cb_al(a->a) && a->lda % 4 == 0 && (!bin || (cb_al(a->b) && a->ldb % 4 == 0)) &&
           cb_al(a->out) && cb_al(a->out_bf16);
  const bool mul = a->op == PKC_COMBINE_MULT;
  return cb_al(a->gslab) && (a->nslab == 1 || a->slab_stride % 4 == 0) && cb_al(a->da) &&
         cb_al(a->db) && (!(mul && a->db) || (cb_al(a->a) && a->lda % 4 == 0)) &&
         (!(mul && a->da) || (cb_al(a->b) && a->ldb % 4 == 0));
}

// 256 threads, one item each up to 2048 workgroups (8 per CU), grid-stride beyond
static dim3 combine_grid(const pkc_combine_args* a, int V) {
  const int N = a->op == PKC_COMBINE_CONCAT ? a->Na + a->Nb : a->Na;
  const uint64_t items = (uint64_t)a->M * (uint64_t)(N / V);
  uint64_t blocks = (items + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  return dim3((unsigned)blocks);
}

}  // namespace pkc

extern "C" int pkc_combine_ok(const pkc_combine_args* a, int backward) {
  return pkc::combine_check(a, backward != 0, "pkc_combine_ok") == PKC_OK ? 1 : 0;
}

extern "C" int pkc_combine_fwd(const pkc_combine_args* a, void* stream) {
  using namespace pkc;
  const int rc = combine_check(a, false, "pkc_combine_fwd");
  if (rc != PKC_OK) return rc;
  if (combine_vec(a, false))
    hipLaunchKernelGGL(combine_fwd_kernel<4>, combine_grid(a, 4), dim3(256), 0, S(stream), *a);
  else
    hipLaunchKernelGGL(combine_fwd_kernel<1>, combine_grid(a, 1), dim3(256), 0, S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_combine_fwd");
  return PKC_OK;
}

extern "C" int pkc_combine_bwd(const pkc_combine_args* a, void* stream) {
  using namespace pkc;
  const int rc = combine_check(a, true, "pkc_combine_bwd");
  if (rc != PKC_OK) return rc;
  if (combine_vec(a, true))
    hipLaunchKernelGGL(combine_bwd_kernel<4>, combine_grid(a, 4), dim3(256), 0, S(stream), *a);
  else
    hipLaunchKernelGGL(combine_bwd_kernel<1>, combine_grid(a, 1), dim3(256), 0, S(stream), *a);
  PKC_LAUNCH_CHECK("pkc_combine_bwd");
  return PKC_OK;
}
