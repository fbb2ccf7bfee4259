// pkc_kaldi_feats.hip — Kaldi's fbank / MFCC features (compute-fbank-feats, compute-mfcc-feats;
// snip-edges, no dither, no VTLN) from int16 audio in HBM: the `pkc-fbank` / `pkc-mfcc` fea_opts
// stages.  The contract and the per-frame steps are in include/pkc.h.
//
// One wavefront (a 64-thread workgroup) per output row: the frame's L samples become the N/2-point
// complex sequence z[k] = y[2k] + i y[2k+1] in LDS (stored bit-reversed), a radix-2
// decimation-in-time FFT runs in place, the real-input split step gives the power spectrum, and
// the mel dot products, the log, the DCT and the lifter follow from LDS.  The frame itself (mean
// removal, preemphasis, window) is float32, as Kaldi's is; the FFT, the power spectrum and every
// sum are carried in fp64 (a float32 radix-2 FFT measured 2x to 10x the error of numpy's float32
// FFT on a full-scale square wave, whose weak bins sit 100 dB under its harmonics), and the
// results are rounded to float32 where Kaldi holds a float: the energy, the log-mel values, the
// cepstra.
//
// Per row the kernel reads 2 L bytes of audio (each sample is re-read by L/S frames, from L2) and
// writes 4 D bytes; the window, twiddle, mel and DCT tables are a few KiB shared by every row.
// Every sum has a fixed order (a lane's strided partial sums, then the xor butterfly; the mel and
// DCT sums are sequential in one lane) and no row reads anything but its own samples, so a row's
// bits do not depend on which other rows the call computes.
#include <float.h>
#include <math.h>

#include "pkc_common.h"

namespace pkc {

constexpr int KF_MAX_N = 4096;   // FFT length; LDS: (N + N/2) doubles + bins floats <= 49 KiB
constexpr int KF_MAX_D = 256;    // output columns and mel bands

__device__ __forceinline__ int warp_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64) void kaldi_feats_kernel(pkc_kaldi_feats_args a, int logM) {
  extern __shared__ __attribute__((aligned(16))) double kf_smem[];
  const int lane = threadIdx.x;
  const int L = a.L, N = a.N, M = N >> 1, B = a.num_bins;
  double2* z = reinterpret_cast<double2*>(kf_smem);  // (M) complex
  double* pw = kf_smem + N;                          // (M) power or magnitude spectrum
  float* melv = reinterpret_cast<float*>(pw + M);    // (B) log mel energies
  const double2* tw = reinterpret_cast<const double2*>(a.twiddle);
  for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
    // u, f and everything derived from them are the same in all 64 lanes: the skips are uniform
    const int u = a.utt_of_row[r], f = a.frame_of_row[r];
    if (u < 0 || u >= a.n_utts || f < 0) continue;
    if ((int64_t)f * a.S + L > (int64_t)a.utt_len[u]) continue;
    const int16_t* s = a.samples + a.utt_beg[u] + (int64_t)f * a.S;

    float mean = 0.f;
    if (a.remove_dc) {           // an integer sum: exact, whatever its order (L * 32768 < 2^31)
      int acc = 0;
      for (int i = lane; i < L; i += 64) acc += s[i];
      mean = (float)((double)warp_sum_i(acc) / (double)L);
    }
    double e = 0.0;
    for (int i = lane; i < N; i += 64) {
      float y = 0.f;
      if (i < L) {
        const float x = (float)s[i] - mean;
        const float xp = (float)s[i > 0 ? i - 1 : 0] - mean;
        y = (x - a.preemph * xp) * a.window[i];
        e += a.raw_energy ? (double)x * x : (double)y * y;
      }
      const int k = (int)(__brev((unsigned)(i >> 1)) >> (32 - logM));
      reinterpret_cast<double*>(z + k)[i & 1] = (double)y;
    }
    float energy = (float)log(fmax(warp_sum_d(e), a.raw_energy ? (double)FLT_EPSILON
                                                               : (double)FLT_MIN));
    energy = fmaxf(energy, a.log_energy_floor);
    __syncthreads();

    for (int st = 0; st < logM; ++st) {
      const int half = 1 << st;
      for (int j = lane; j < (M >> 1); j += 64) {
        const int pos = j & (half - 1);
        const int ia = ((j >> st) << (st + 1)) + pos, ib = ia + half;
        const double2 w = tw[pos * (M >> st)];       // exp(-2 pi i pos / (2 half))
        const double2 A = z[ia], Bv = z[ib];
        const double tr = Bv.x * w.x - Bv.y * w.y, ti = Bv.x * w.y + Bv.y * w.x;
        z[ia] = make_double2(A.x + tr, A.y + ti);
        z[ib] = make_double2(A.x - tr, A.y - ti);
      }
      __syncthreads();
    }

    // X[k] = (Z[k] + conj Z[M-k]) / 2 - i/2 W_N^k (Z[k] - conj Z[M-k]), k < M; the Nyquist bin
    // X[M] enters no mel band and is not formed
    for (int k = lane; k < M; k += 64) {
      const double2 Zk = z[k], Zm = z[(M - k) & (M - 1)], w = tw[k];
      const double ex = 0.5 * (Zk.x + Zm.x), ey = 0.5 * (Zk.y - Zm.y);
      const double ox = 0.5 * (Zk.y + Zm.y), oy = -0.5 * (Zk.x - Zm.x);
      const double re = ex + (ox * w.x - oy * w.y), im = ey + (ox * w.y + oy * w.x);
      const double p = re * re + im * im;
      pw[k] = a.use_power ? p : sqrt(p);
    }
    __syncthreads();

    for (int b = lane; b < B; b += 64) {
      int first = a.mel_first[b], cnt = a.mel_count[b];
      const float* wgt = a.mel_weight + a.mel_offset[b];
      if (first < 0 || first > M) cnt = 0;
      if (cnt > M - first) cnt = M - first;
      double acc = 0.0;
      for (int i = 0; i < cnt; ++i) acc += (double)wgt[i] * pw[first + i];
      melv[b] = (float)log(fmax(acc, (double)FLT_EPSILON));
    }
    __syncthreads();

    float* o = a.out + r * (int64_t)a.D;
    if (a.mfcc) {
      for (int k = lane; k < a.num_ceps; k += 64) {
        const float* row = a.dct + (int64_t)k * B;
        double acc = 0.0;
        for (int n = 0; n < B; ++n) acc += (double)row[n] * (double)melv[n];
        o[k] = (k == 0 && a.use_energy) ? energy : (float)acc * a.lifter[k];
      }
    } else {
      const int c0 = a.use_energy ? 1 : 0;
      if (c0 && lane == 0) o[0] = energy;
      for (int b = lane; b < B; b += 64) o[c0 + b] = melv[b];
    }
    // the next row's first LDS writes are to z, last read two barriers ago
  }
}

static int kf_check(const pkc_kaldi_feats_args* a, const char* who) {
  PKC_CHECK_ARG(a != nullptr, "%s: null argument", who);
  PKC_CHECK_ARG(a->N >= 4 && a->N <= KF_MAX_N && (a->N & (a->N - 1)) == 0,
                "%s: the FFT length N = %d must be a power of two in 4..%d", who, a->N, KF_MAX_N);
  PKC_CHECK_ARG(a->L >= 2 && a->L <= a->N && a->S >= 1,
                "%s: frame length %d (2..N = %d) / frame shift %d (>= 1)", who, a->L, a->N, a->S);
  PKC_CHECK_ARG(a->num_bins >= 1 && a->num_bins <= KF_MAX_D,
                "%s: %d mel bins (1..%d)", who, a->num_bins, KF_MAX_D);
  if (a->mfcc) {
    PKC_CHECK_ARG(a->num_ceps >= 1 && a->num_ceps <= a->num_bins && a->D == a->num_ceps,
                  "%s: mfcc with %d cepstra over %d bins and D = %d (1 <= num_ceps <= bins, "
                  "D == num_ceps)", who, a->num_ceps, a->num_bins, a->D);
  } else {
    PKC_CHECK_ARG(a->D == a->num_bins + (a->use_energy ? 1 : 0),
                  "%s: fbank with %d bins, use_energy %d and D = %d", who, a->num_bins,
                  a->use_energy, a->D);
  }
  PKC_CHECK_ARG(a->D <= KF_MAX_D, "%s: D = %d output columns (<= %d)", who, a->D, KF_MAX_D);
  PKC_CHECK_ARG(a->rows >= 0 && a->n_utts >= 0, "%s: rows %lld / n_utts %d", who,
                (long long)a->rows, a->n_utts);
  return PKC_OK;
}

}  // namespace pkc

extern "C" int pkc_kaldi_feats_ok(const pkc_kaldi_feats_args* a) {
  return pkc::kf_check(a, "pkc_kaldi_feats_ok") == PKC_OK ? 1 : 0;
}

extern "C" int pkc_kaldi_feats(const pkc_kaldi_feats_args* a, void* stream) {
  using namespace pkc;
  if (int rc = kf_check(a, "pkc_kaldi_feats")) return rc;
  if (a->rows == 0) return PKC_OK;
  PKC_CHECK_ARG(a->samples && a->utt_beg && a->utt_len && a->utt_of_row && a->frame_of_row &&
                    a->window && a->twiddle && a->mel_first && a->mel_count && a->mel_offset &&
                    a->mel_weight && a->out && (!a->mfcc || (a->dct && a->lifter)),
                "pkc_kaldi_feats: null pointer");
  int logM = 0;
  while ((2 << logM) < a->N) ++logM;
  const size_t lds = sizeof(double) * (size_t)(a->N + a->N / 2) + sizeof(float) * (size_t)a->num_bins;
  const int64_t cap = 256 * 64;
  const unsigned grid = (unsigned)(a->rows < cap ? a->rows : cap);
  hipLaunchKernelGGL(kaldi_feats_kernel, dim3(grid), dim3(64), lds, S(stream), *a, logM);
  PKC_LAUNCH_CHECK("pkc_kaldi_feats");
  return PKC_OK;
}
