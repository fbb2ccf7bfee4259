// pkc_wav.hip — the reference's raw-waveform framing (save_raw_fea.py:73-104) on the GPU.
//
// TIMIT_SincNet_raw.cfg reads a `raw` stream whose every 10 ms label frame is a 200 ms window of
// the waveform (3200 samples at 16 kHz), written by save_raw_fea.py as one float64 ark row per
// frame: the windows overlap 20-fold, so the ark is an 80x copy of the audio.  Here the int16
// audio is uploaded once and the (frames x W) matrix is gathered from it in HBM.
//
// Semantics (restated from the script; S = lab_wshift, Lw = lab_wlen, all in samples):
//   signal = s / 32768 / max|s / 32768|       == (double)s / (double)peak, bit for bit: both
//                                                scalings are powers of two, the division is the
//                                                correctly rounded fp64 one
//   frames f = 0, 1, ... while f*S + Lw < len                       (strict)
//   c = int(f*S + Lw/2 - 1) = (2*f*S + Lw - 2) / 2,  b = c - W/2
//   row[j] = 0 <= b + j < len ? signal[b + j] : 0                   (zero padding at both ends)
// and the float32 cast is the one the ark reader applies to the float64 rows.
//
// Two launches: normalise every sample once into sig_work (one fp64 division per sample, not one
// per output element), then the gather.  The gather is store-bound: 4*W B written per row, its
// reads are ~W/S-fold reuse of a signal that stays in L2 / Infinity Cache.
#include "pkc_common.h"

#pragma clang fp contract(off)

namespace pkc {

// frames of a len-sample utterance: the count of f >= 0 with f*S + Lw < len
__device__ __forceinline__ int wav_nframes(int len, int Lw, int S) {
  return len > Lw ? (len - Lw + S - 1) / S : 0;
}

// One wavefront per output row in both kernels: the row's utterance, frame, length and offsets are
// wave-uniform (scalar loads), so the only per-lane memory operations are the samples themselves.
constexpr int WAV_WAVES = 4;    // rows per 256-thread block and pass

// Every sample belongs to one frame: frame min(i / S, F-1).  A row normalises the samples of its
// frame, so row maps naming every frame of an utterance normalise each of its samples once
// (a frame named twice writes the same values twice).
__global__ __launch_bounds__(256) void wav_norm_kernel(
    const int16_t* __restrict__ samples, const int64_t* __restrict__ utt_beg,
    const int32_t* __restrict__ utt_len, const int32_t* __restrict__ utt_peak,
    const int32_t* __restrict__ utt_of_row, const int32_t* __restrict__ frame_of_row,
    int64_t Nout, int Lw, int S, float* __restrict__ sig_work) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t r = (int64_t)blockIdx.x * WAV_WAVES + wv; r < Nout;
       r += (int64_t)gridDim.x * WAV_WAVES) {
    const int u = utt_of_row[r], f = frame_of_row[r];
    const int len = utt_len[u];
    const int F = wav_nframes(len, Lw, S);
    if (f < 0 || f >= F) continue;
    const int64_t base = utt_beg[u];
    const double peak = (double)utt_peak[u];
    const int i0 = f * S;
    const int i1 = f == F - 1 ? len : i0 + S;
    for (int i = i0 + lane; i < i1; i += 64)
      sig_work[base + i] = (float)((double)samples[base + i] / peak);
  }
}

typedef float wav_f4 __attribute__((ext_vector_type(4)));
typedef float wav_f4u __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned 16 B load

// V consecutive columns per lane (V = 4: one 16-byte store, consecutive lanes on consecutive 16 B,
// fed by one dword-aligned 16-byte load where the four samples lie inside the signal; V = 1: the
// scalar path for W % 4 != 0).
template <int V>
__global__ __launch_bounds__(256) void wav_gather_kernel(
    const float* __restrict__ sig_work, const int64_t* __restrict__ utt_beg,
    const int32_t* __restrict__ utt_len, const int32_t* __restrict__ utt_of_row,
    const int32_t* __restrict__ frame_of_row, int64_t Nout, int W, int Lw, int S,
    float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t r = (int64_t)blockIdx.x * WAV_WAVES + wv; r < Nout;
       r += (int64_t)gridDim.x * WAV_WAVES) {
    const int u = utt_of_row[r], f = frame_of_row[r];
    const int len = utt_len[u];
    const float* sig = sig_work + utt_beg[u];
    const int b = (2 * f * S + Lw - 2) / 2 - W / 2;
    float* dst = out + r * (int64_t)W;
#pragma unroll 2
    for (int j = lane * V; j < W; j += 64 * V) {
      const int i = b + j;
      if constexpr (V == 4) {
        wav_f4 v;
        if (i >= 0 && i + 4 <= len) {
          v = *reinterpret_cast<const wav_f4u*>(sig + i);
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = (i + t >= 0 && i + t < len) ? sig[i + t] : 0.f;
        }
        // written once and far larger than the caches: a non-temporal 16-byte store (on the
        // 210 k-row chunk of DESIGN 5 the whole call took 551 us against 690 us with plain stores)
        __builtin_nontemporal_store(v, reinterpret_cast<wav_f4*>(dst + j));
      } else {
        dst[j] = (i >= 0 && i < len) ? sig[i] : 0.f;
      }
    }
  }
}

}  // namespace pkc

extern "C" int pkc_wav_frames(const int16_t* samples, const int64_t* utt_beg,
                              const int32_t* utt_len, const int32_t* utt_peak,
                              const int32_t* utt_of_row, const int32_t* frame_of_row, int64_t Nout,
                              int W, int lab_wlen, int lab_wshift, float* sig_work, float* out,
                              void* stream) {
  using namespace pkc;
  PKC_CHECK_ARG(samples && utt_beg && utt_len && utt_peak && utt_of_row && frame_of_row &&
                    sig_work && out,
                "pkc_wav_frames: null pointer");
  PKC_CHECK_ARG(W > 0 && W % 2 == 0, "pkc_wav_frames: the window W = %d must be positive and even",
                W);
  PKC_CHECK_ARG(lab_wlen >= 2 && lab_wshift >= 1 && Nout >= 0,
                "pkc_wav_frames: bad lab_wlen %d / lab_wshift %d / Nout %lld", lab_wlen, lab_wshift,
                (long long)Nout);
  if (Nout == 0) return PKC_OK;
  const int64_t want = (Nout + WAV_WAVES - 1) / WAV_WAVES;
  const unsigned grid = (unsigned)(want < (1 << 20) ? want : (1 << 20));
  hipLaunchKernelGGL(wav_norm_kernel, dim3(grid), dim3(256), 0, S(stream), samples, utt_beg,
                     utt_len, utt_peak, utt_of_row, frame_of_row, Nout, lab_wlen, lab_wshift,
                     sig_work);
  PKC_LAUNCH_CHECK("pkc_wav_frames (normalise)");
  if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
    hipLaunchKernelGGL(wav_gather_kernel<4>, dim3(grid), dim3(256), 0, S(stream), sig_work, utt_beg,
                       utt_len, utt_of_row, frame_of_row, Nout, W, lab_wlen, lab_wshift, out);
  else
    hipLaunchKernelGGL(wav_gather_kernel<1>, dim3(grid), dim3(256), 0, S(stream), sig_work, utt_beg,
                       utt_len, utt_of_row, frame_of_row, Nout, W, lab_wlen, lab_wshift, out);
  PKC_LAUNCH_CHECK("pkc_wav_frames (gather)");
  return PKC_OK;
}
