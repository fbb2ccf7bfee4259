// pkc_feat_transform.hip — splice-feats and transform-feats of the fMLLR feature pipe, on the GPU.
//
// Kaldi's steps/nnet/make_fmllr_feats.sh dumps the features every *_fmllr cfg trains on through
//   apply-cmvn | splice-feats --left-context=3 --right-context=3 | transform-feats final.mat |
//   transform-feats --utt2spk=ark:U ark:trans.ark
// The two tools are restated here from Kaldi's published feat/feature-functions.cc SpliceFrames and
// featbin/transform-feats.cc (Kaldi is third-party and absent: parity UNPINNED against Kaldi itself):
//   splice:    spl[j*D + d] = in[clamp(t + j - L, first frame, last frame of the utterance)][d],
//              j = 0..L+R (past frame first)
//   transform: out[o] = (sum_k A[o][k] * spl[k]) + b[o]   (AddMatMat, then AddVecToRows; a linear
//              matrix has no b), with K = D*(L+R+1) and A the utterance's own Dout x K matrix.
// One launch does both, so a spliced matrix never reaches HBM in front of a transform.
//
// A workgroup of 256 threads takes one tile of the host-built tile table: up to `tile rows`
// consecutive output rows that are consecutive frames of ONE utterance (so one matrix).  It stages
// the tile + L + R source frames in LDS, already clamped; the spliced row of tile row i is then the
// K contiguous floats from frames[i*D], and nothing is spliced in memory.  The matrix is staged in
// LDS transposed ([k][o], o padded to a multiple of 4) in chunks of at most 64 outputs x KC columns;
// a thread owns 4 consecutive outputs of 4 consecutive rows (16 accumulators): per k one 16-byte LDS
// read of the matrix and 4 broadcast reads of the frames feed 16 FMAs, and a row's 4 outputs leave
// as one 16-byte store when Dout % 4 == 0.
//
// Numerics: fp32 everywhere.  Each output element is one thread's fmaf chain over k = 0..K-1 in
// ascending order starting from 0.0f (the accumulators live across the matrix chunks), then one
// addition of b: equal inputs give equal bits whatever the tiling or the row order, and a row never
// reads another utterance.  No atomics.
#include "pkc_common.h"

namespace pkc {

constexpr int FT_THREADS = 256;
constexpr int FT_RB = 4;                 // rows per thread
constexpr int FT_OC = 64;                // outputs per matrix chunk (a multiple of 4)
constexpr int FT_FRAME_FLOATS = 8192;    // LDS budget of the staged frames (32 KB)
constexpr int FT_MAT_FLOATS = 6144;      // LDS budget of one matrix chunk (24 KB)
constexpr int FT_TILE_MAX = 128;
constexpr int FT_MAX_K = 4096, FT_MAX_DOUT = 512, FT_MAX_CTX = 64;

struct FtGeom {
  int K, Dp, OC, KC, tile;
  size_t lds;
};

// The launch geometry of a shape (tile == 0: unsupported, the reason in `why`).
static FtGeom ft_geom(int D, int L, int R, int Dout, int has_mat, const char** why) {
  FtGeom g = {};
  *why = nullptr;
  if (D < 1 || L < 0 || R < 0 || L > FT_MAX_CTX || R > FT_MAX_CTX) {
    *why = "needs D >= 1 and 0 <= left / right context <= 64";
    return g;
  }
  const int64_t K64 = (int64_t)D * (L + R + 1);
  if (K64 > FT_MAX_K) {
    *why = "spliced width K = D * (left + right + 1) is above 4096";
    return g;
  }
  g.K = (int)K64;
  if (has_mat ? (Dout < 1 || Dout > FT_MAX_DOUT) : Dout != g.K) {
    *why = has_mat ? "needs 1 <= Dout <= 512" : "a splice without a transform writes Dout = K columns";
    return g;
  }
  int tile = FT_FRAME_FLOATS / D - L - R;           // >= 1: (1 + L + R) * D = K <= 4096
  tile = tile < FT_TILE_MAX ? tile : FT_TILE_MAX;
  if (has_mat) {
    g.Dp = (Dout + 3) & ~3;
    g.OC = g.Dp < FT_OC ? g.Dp : FT_OC;
    g.KC = FT_MAT_FLOATS / g.OC;                    // >= 96
    g.KC = g.KC < g.K ? g.KC : g.K;
    const int groups = FT_THREADS / (g.OC / 4);     // one work item per thread and matrix chunk
    tile = tile < groups * FT_RB ? tile : groups * FT_RB;
  }
  g.tile = tile;
  g.lds = sizeof(float) * ((size_t)(tile + L + R) * D + (has_mat ? (size_t)g.KC * g.OC : 0));
  return g;
}

// frames (LDS): (n + L + R) x D, row i = source frame clamp(s0 + i - L) of the tile's utterance.
__device__ __forceinline__ void ft_stage_frames(float* frames, const float* __restrict__ in, int D,
                                                int L, int nctx, int64_t s0, int64_t b, int64_t e) {
  for (int i = threadIdx.x; i < nctx * D; i += FT_THREADS) {
    const int fr = i / D, d = i - fr * D;
    int64_t f = s0 + fr - L;
    f = f < b ? b : (f > e ? e : f);
    frames[i] = in[f * D + d];
  }
}

__global__ __launch_bounds__(FT_THREADS) void feat_transform_kernel(
    const float* __restrict__ in, int D, int L, int R, int64_t Nout,
    const int32_t* __restrict__ srow, const int32_t* __restrict__ urow,
    const int32_t* __restrict__ ubeg, const int32_t* __restrict__ uend, int n_utts,
    const int32_t* __restrict__ umat, const float* __restrict__ mats, int n_mats, int Dout,
    int affine, const int32_t* __restrict__ tiles, int tile_rows, int OC, int KC,
    float* __restrict__ out) {
  extern __shared__ float4 lds4[];
  const int K = D * (L + R + 1);
  const int64_t row0 = tiles[2 * blockIdx.x];
  int n = tiles[2 * blockIdx.x + 1];
  n = n < tile_rows ? n : tile_rows;
  if (row0 < 0 || n < 1 || row0 + n > Nout) return;          // a tile outside the output: nothing
  const int u = urow[row0];
  if (u < 0 || u >= n_utts) return;
  const int64_t s0 = srow[row0], b = ubeg[u], e = (int64_t)uend[u] - 1;
  if (e < b) return;
  float* At = reinterpret_cast<float*>(lds4);                 // 16-byte aligned: KC * OC floats
  float* frames = At + (mats ? (size_t)KC * OC : 0);
  const int nctx = n + L + R;
  ft_stage_frames(frames, in, D, L, nctx, s0, b, e);
  __syncthreads();

  if (mats == nullptr) {                                       // splice alone: a bit-for-bit copy
    float* dst = out + row0 * (int64_t)K;
    if ((K & 3) == 0) {
      const int q = K >> 2;
      for (int i = threadIdx.x; i < n * q; i += FT_THREADS) {
        const int r = i / q, k = (i - r * q) << 2;
        const float* src = frames + r * D + k;
        reinterpret_cast<float4*>(dst)[i] = make_float4(src[0], src[1], src[2], src[3]);
      }
    } else {
      for (int i = threadIdx.x; i < n * K; i += FT_THREADS) {
        const int r = i / K;
        dst[i] = frames[r * D + (i - r * K)];
      }
    }
    return;
  }

  int m = umat ? umat[u] : 0;
  if (m < 0 || m >= n_mats) return;
  const int ldm = K + affine;
  const float* __restrict__ A = mats + (int64_t)m * Dout * ldm;
  const int Dp = (Dout + 3) & ~3;
  for (int o0 = 0; o0 < Dp; o0 += OC) {
    const int oc = (Dp - o0) < OC ? (Dp - o0) : OC;           // a multiple of 4
    const int Q = oc >> 2;
    const int q = threadIdx.x % Q, g = threadIdx.x / Q;
    const int r0 = g * FT_RB;
    const bool active = r0 < n;
    float acc[FT_RB][4];
#pragma unroll
    for (int i = 0; i < FT_RB; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += KC) {
      const int kc = (K - k0) < KC ? (K - k0) : KC;
      if (o0 || k0) __syncthreads();                           // the previous chunk is read
      for (int i = threadIdx.x; i < oc * kc; i += FT_THREADS) {
        const int oo = i / kc, kk = i - oo * kc;
        At[kk * oc + oo] = (o0 + oo < Dout) ? A[(int64_t)(o0 + oo) * ldm + k0 + kk] : 0.f;
      }
      __syncthreads();
      if (active) {
        const float* x[FT_RB];                                 // rows past the tile: its last row,
#pragma unroll
        for (int i = 0; i < FT_RB; ++i)                        // computed and not written
          x[i] = frames + (r0 + i < n ? r0 + i : n - 1) * D + k0;
        const float4* a4 = reinterpret_cast<const float4*>(At) + q;
#pragma unroll 4
        for (int kk = 0; kk < kc; ++kk) {
          const float4 a = a4[kk * Q];
#pragma unroll
          for (int i = 0; i < FT_RB; ++i) {
            const float xv = x[i][kk];
            acc[i][0] = __builtin_fmaf(a.x, xv, acc[i][0]);
            acc[i][1] = __builtin_fmaf(a.y, xv, acc[i][1]);
            acc[i][2] = __builtin_fmaf(a.z, xv, acc[i][2]);
            acc[i][3] = __builtin_fmaf(a.w, xv, acc[i][3]);
          }
        }
      }
    }
    if (!active) continue;
    const int o = o0 + 4 * q;
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    if (affine) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (o + j < Dout) bias[j] = A[(int64_t)(o + j) * ldm + K];
    }
#pragma unroll
    for (int i = 0; i < FT_RB; ++i) {
      if (r0 + i >= n) break;
      float* dst = out + (row0 + r0 + i) * (int64_t)Dout + o;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = affine ? __fadd_rn(acc[i][j], bias[j]) : acc[i][j];
      if ((Dout & 3) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (o + j < Dout) dst[j] = v[j];
      }
    }
  }
}

}  // namespace pkc

extern "C" int pkc_feat_transform_ok(int D, int L, int R, int Dout, int has_mat) {
  const char* why;
  const pkc::FtGeom g = pkc::ft_geom(D, L, R, Dout, has_mat, &why);
  if (g.tile == 0) {
    pkc::set_error("pkc_feat_transform: D = %d, left %d, right %d, Dout = %d: %s", D, L, R, Dout,
                   why);
    return 0;
  }
  return 1;
}

extern "C" int pkc_feat_transform_tile(int D, int L, int R, int Dout, int has_mat) {
  const char* why;
  return pkc::ft_geom(D, L, R, Dout, has_mat, &why).tile;
}

extern "C" int pkc_feat_transform(const float* in, int D, int L, int R, int64_t Nout,
                                  const int32_t* src_row, const int32_t* utt_of_row,
                                  const int32_t* utt_beg, const int32_t* utt_end, int n_utts,
                                  const int32_t* utt_mat, const float* mats, int n_mats, int Dout,
                                  int affine, const int32_t* tiles, int n_tiles, float* out,
                                  void* stream) {
  using namespace pkc;
  if (pkc_feat_transform_ok(D, L, R, Dout, mats != nullptr) != 1) return PKC_ERR_UNSUPPORTED;
  PKC_CHECK_ARG(in && src_row && utt_of_row && utt_beg && utt_end && out && Nout >= 0 &&
                    n_utts >= 0 && n_tiles >= 0 && (n_tiles == 0 || tiles) &&
                    (affine == 0 || affine == 1) && (mats ? n_mats >= 1 : !affine),
                "pkc_feat_transform: bad arguments");
  if (Nout == 0 || n_tiles == 0) return PKC_OK;
  const char* why;
  const FtGeom g = ft_geom(D, L, R, Dout, mats != nullptr, &why);
  hipLaunchKernelGGL(feat_transform_kernel, dim3((unsigned)n_tiles), dim3(FT_THREADS), g.lds,
                     S(stream), in, D, L, R, Nout, src_row, utt_of_row, utt_beg, utt_end, n_utts,
                     utt_mat, mats, n_mats, Dout, affine, tiles, g.tile, g.OC, g.KC, out);
  PKC_LAUNCH_CHECK("pkc_feat_transform");
  return PKC_OK;
}
